"""Levels 6 .. 8 of a one-output tree fit (oneprot_amd/gbt.py, max_depth 7 .. 9; ref src/saprot_fit_reg.py:26-32 under configs/saprot_sweep_xgboost_reg.yaml):
the launches of csrc/gbt.hip's node-ordered path.  A level has 2^level nodes, more than the 64 (node, feature) slots of the histogram kernel's LDS tile hold
with a whole feature each, and at 1,280 features and 256 bins more bytes than the histogram budget.  So the rows are put in node order once per level
(keys -> the stable radix sort -> segment bounds), and the level's histograms and split search run a group of nodes at a time (gbt.plan_node_groups) into one
buffer; one partition launch then moves the rows of the whole level.  Every buffer is sized when the object is built, every launch is a function of the shapes
alone and nothing is read back.  The split rule is the shallow levels': the same device code with a node offset."""
import torch

from . import hip

FIRST_LEVEL = 6                # the first level that runs through here; levels 0 .. 5 run through oneprot_gbt_hist / oneprot_gbt_split
LAST_LEVEL = 8


def node_order(pos, level, *, keys=None, sorted_keys=None, order=None, seg=None, sort_ws=None):
    """(order int32 [N], sorted keys int32 [N], seg int32 [2^level + 1]) of pos int32 [N] at a level 6 .. 8: the rows in the stable order of their node of
    the level, rows of no node of the level last (key 2^level); seg[n] is where node n begins.  Buffers are allocated unless handed over."""
    N, L = pos.numel(), 1 << level
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=pos.device)
    keys = i32(N) if keys is None else keys
    sorted_keys = i32(N) if sorted_keys is None else sorted_keys
    order = i32(N) if order is None else order
    seg = i32(L + 1) if seg is None else seg[:L + 1]
    sort_ws = hip._workspace("oneprot_sort_workspace", pos, N) if sort_ws is None else sort_ws
    hip.call("oneprot_gbt_node_keys", pos, keys, N, level)
    hip.call("oneprot_sort_i32", keys, None, N, level + 1, sorted_keys, order, sort_ws, sort_ws.numel())
    hip.call("oneprot_gbt_node_seg", sorted_keys, seg, N, level)
    return order, sorted_keys, seg


class DeepLevels:
    """the buffers of a fit's deep levels and the launch sequence of one level"""

    def __init__(self, N, F, max_bin, max_depth, groups, device):
        """groups: {level: [(node0, node1), ...]} for the levels 6 .. max_depth - 1 (gbt.plan_node_groups)"""
        self.N, self.F, self.B, self.groups = N, F, max_bin, groups
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=device)
        self.keys, self.sorted_keys, self.order, self.seg = i32(N), i32(N), i32(N), i32((1 << (max_depth - 1)) + 1)
        self.sort_ws = hip._workspace("oneprot_sort_workspace", self.keys, N)
        widest = max(n1 - n0 for g in groups.values() for n0, n1 in g)
        self.hist_bytes = hip.query("oneprot_gbt_hist_nodes_bytes", F, max_bin, widest)
        self.split_ws = hip._workspace("oneprot_gbt_split_nodes_workspace", self.keys, F, widest)

    def run(self, level, hist, bins, gq, hq, pos, cuts, ncuts, feat_keep, expo, tf, tb, tt, tl, NN, mcw, gamma, alpha, lam, lr):
        """histogram -> split search per node group of `level`, then the level's partition; gq / hq / pos [1, N], tree arrays [1, NN], hist an int64 buffer of
        at least hist_bytes"""
        N, F, B = self.N, self.F, self.B
        order, skeys, seg = node_order(pos.view(-1), level, keys=self.keys, sorted_keys=self.sorted_keys, order=self.order, seg=self.seg, sort_ws=self.sort_ws)
        for n0, n1 in self.groups[level]:
            hip.call("oneprot_gbt_hist_nodes", bins, gq, hq, order, skeys, seg, hist, N, F, B, level, n0, n1 - n0, 0)
            hip.call("oneprot_gbt_split_nodes", hist, cuts, ncuts, feat_keep, expo, tf, tb, tt, tl, None, self.split_ws, self.split_ws.numel(), F, B, level, n0, n1 - n0, NN,
                     mcw, gamma, alpha, lam, lr)
        hip.call("oneprot_gbt_partition", bins, tf, tb, pos, N, F, level, 1, NN)
