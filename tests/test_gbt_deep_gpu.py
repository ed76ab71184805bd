"""The deep tree levels on the GPU (XGBRegressor max_depth 7 .. 9; csrc/gbt.hip's node-ordered path, oneprot_amd/gbt_deep.py): node order and segments,
oneprot_gbt_hist_nodes and oneprot_gbt_split_nodes against numpy and the restatement, the end-to-end fixtures of tests/gbt_deep_cases.py, and the properties of a
depth-9 fit.  Every comparison but the gains (1e-12 relative, the bound of tests/test_gbt_gpu.py) is of integers or bits: none has a tolerance."""
import functools
import math

import numpy as np
import pytest
import torch

from oneprot_amd import gbt, gbt_deep, hip
from tests import gbt_cases as C
from tests import gbt_deep_cases as D
from tests import gbt_ref as R
from tests.gbt_cases import DEV, assert_same_trees, dev, hist_reference

pytestmark = pytest.mark.gpu
GUARD = 64                     # int64 words behind a group's histogram that must stay as they were


# ================================================================================================================== node order
@pytest.mark.parametrize("level", [6, 7, 8])
def test_node_order_and_segments(level):
    """order = the stable argsort of the keys (rows of no node of the level last), seg = searchsorted: N = 1, one run, one run and a row, several runs"""
    rng = np.random.default_rng(level)
    for N in (1, 2047, 2048, 5000):
        pos = D.level_pos(rng, N, level)
        want_order, want_keys, want_seg = D.order_reference(pos, level)
        order, skeys, seg = gbt_deep.node_order(dev(pos), level)
        assert np.array_equal(order.cpu().numpy(), want_order), (level, N)
        assert np.array_equal(skeys.cpu().numpy(), want_keys), (level, N)
        assert np.array_equal(seg.cpu().numpy(), want_seg), (level, N)


# ================================================================================================================== histograms of a node group
def run_hist_nodes(d, level, B, node0, nodes, tile=0, ordered=None):
    """d = (bins, gq, hq, pos) device tensors of one output -> int64 [nodes F B 2 + GUARD], prefilled with -7 (overwritten, not accumulated)"""
    bins, gq, hq, pos = d
    N, F = bins.shape
    order, skeys, seg = gbt_deep.node_order(pos, level) if ordered is None else ordered
    buf = torch.full((nodes * F * B * 2 + GUARD,), -7, dtype=torch.int64, device=DEV)
    assert hip.query("oneprot_gbt_hist_nodes_bytes", F, B, nodes) == (buf.numel() - GUARD) * 8
    hip.call("oneprot_gbt_hist_nodes", bins, gq, hq, order, skeys, seg, buf, N, F, B, level, node0, nodes, tile)
    return buf


def check_group(buf, want, node0, nodes, label):
    """want int64 [L, F, B, 2] of the whole level"""
    body = buf[:-GUARD].view(nodes, *want.shape[1:]).cpu().numpy()
    assert (buf[-GUARD:] == -7).all(), label
    bad = np.argwhere(body != want[node0:node0 + nodes])
    assert len(bad) == 0, (label, bad[:5], body[tuple(bad[0])], want[node0:node0 + nodes][tuple(bad[0])])


def test_hist_nodes_level_6_random_rows():
    """level 6, N = 5000 (three runs), F = 12, B = 16: random nodes, rows that stopped above, rows with g = h = 0; every tile shape gives the same integers"""
    rng = np.random.default_rng(60)
    N, F, B, level = 5000, 12, 16, 6
    bins, gq, hq = D.random_rows(rng, N, F, B)
    pos = D.level_pos(rng, N, level)
    want = hist_reference(bins, gq[None].astype(np.int64), hq[None].astype(np.int64), pos[None], level, B)[0]
    d = (dev(bins), dev(gq), dev(hq), dev(pos))
    for tile in (0, 64, 32, 16, 8, 4, 2, 1):
        check_group(run_hist_nodes(d, level, B, 0, 64, tile), want, 0, 64, f"tile {tile}")
    check_group(run_hist_nodes(d, level, B, 5, 13), want, 5, 13, "group (5, 13)")


@pytest.mark.parametrize("F,B", [(1, 2), (1, 256), (65, 2), (65, 256), (130, 2), (130, 256)])
def test_hist_nodes_level_8_hand_written_segments(F, B):
    """the hand-written level-8 segments (gbt_deep_cases.hand_case): empty first and last node, a node of one row, nodes of exactly 2047 and 2048 rows whose
    counter would wrap int32 without a flush, a node of three runs; B = 256 uses the 128 KB tile, F = 65 and 130 end in a tile of 1 resp. 2 features"""
    h = D.hand_case(F, B)
    want = D.hand_reference(F, B)
    d = (dev(h["bins"]), dev(h["gq"]), dev(h["hq"]), dev(h["pos"]))
    ordered = gbt_deep.node_order(d[3], 8)
    for tile in (0, 64, 16, 1):
        check_group(run_hist_nodes(d, 8, B, 0, 256, tile, ordered), want, 0, 256, f"F {F} B {B} tile {tile}")


def test_hist_nodes_level_7_thirty_five_runs():
    rng = np.random.default_rng(70)
    N, F, B, level = 70001, 8, 4, 7
    assert -(-N // D.GBT_ROWS) == 35
    bins, gq, hq = D.random_rows(rng, N, F, B)
    pos = D.level_pos(rng, N, level)
    want = hist_reference(bins, gq[None].astype(np.int64), hq[None].astype(np.int64), pos[None], level, B)[0]
    d = (dev(bins), dev(gq), dev(hq), dev(pos))
    for tile in (0, 8):
        check_group(run_hist_nodes(d, level, B, 0, 128, tile), want, 0, 128, f"tile {tile}")


@pytest.mark.parametrize("node0,nodes", [(0, 256), (0, 1), (255, 1), (96, 32), (40, 2), (3, 1)])
def test_hist_node_groups_equal_the_slices_of_the_level(node0, nodes):
    """a group of the hand-written level-8 case equals the matching slice of the whole level, and nothing behind the group is written"""
    F, B = 65, 2
    h = D.hand_case(F, B)
    d = (dev(h["bins"]), dev(h["gq"]), dev(h["hq"]), dev(h["pos"]))
    for tile in (0, 16):
        check_group(run_hist_nodes(d, 8, B, node0, nodes, tile), D.hand_reference(F, B), node0, nodes, f"group ({node0}, {nodes}) tile {tile}")


# ================================================================================================================== split search of a node group
def split_buffers(NN):
    tf = torch.full((1, NN), -5, dtype=torch.int32, device=DEV)
    return tf, torch.full_like(tf, -5), torch.full((1, NN), -5.0, device=DEV), torch.full((1, NN), -5.0, device=DEV), torch.full((NN,), -5.0, dtype=torch.float64, device=DEV)


def run_split_nodes(H, cuts, ncuts, keep, expo, level, node0, nodes, NN, B, params, out=None):
    """H int64 [nodes, F, B, 2] of the group -> (feat, bin, thr, leaf, gain) device tensors, every entry the call does not write left at -5"""
    F = H.shape[1]
    tf, tb, tt, tl, gain = split_buffers(NN) if out is None else out
    ws = torch.empty(hip.query("oneprot_gbt_split_nodes_workspace", F, nodes), dtype=torch.uint8, device=DEV)
    assert ws.numel() == nodes * F * 48
    hip.call("oneprot_gbt_split_nodes", dev(H), cuts, ncuts, keep, expo, tf, tb, tt, tl, gain.view(torch.uint8), ws, ws.numel(), F, B, level, node0, nodes, NN, *params)
    return tf, tb, tt, tl, gain


def test_split_nodes_of_a_whole_shallow_level_is_oneprot_gbt_split():
    """levels 0, 3 and 5 with node0 = 0 and nodes = 2^level: every output, the gains included, bit-equal to oneprot_gbt_split on the same histogram -- the two
    launches share their device code"""
    rng = np.random.default_rng(31)
    for level, F, B, params in ((0, 5, 8, (1.0, 0.0, 0.0, 1.0, 0.3)), (3, 33, 256, (2.0, 0.1, 0.1, 10.0, 0.1)), (5, 130, 16, (1.0, 0.0, 0.0, 1.0, 0.3))):
        L, NN = 1 << level, (4 << level) - 1
        ncuts = rng.integers(1, B, F)
        bins = np.stack([rng.integers(0, ncuts[f] + 1, 300 * L) for f in range(F)], axis=1).astype(np.uint8)
        _, gq, hq = D.random_rows(rng, 300 * L, F, B)
        pos = (L - 1 + rng.integers(0, L, 300 * L)).astype(np.int32)
        if L > 1:
            pos[pos == L] = L - 1                                               # node 1 of the level is empty
        H = hist_reference(bins, gq[None].astype(np.int64), hq[None].astype(np.int64), pos[None], level, B)
        cuts = torch.arange(F * (B - 1), dtype=torch.float32, device=DEV).view(F, B - 1).contiguous()
        keep = rng.random(F) < 0.8
        keep[0] = True
        args = (cuts, dev(ncuts.astype(np.int32)), dev(keep.astype(np.uint8)), dev(np.zeros(1, dtype=np.int32)))
        a = split_buffers(NN)
        ws = torch.empty(hip.query("oneprot_gbt_split_workspace", F, level, 1), dtype=torch.uint8, device=DEV)
        hip.call("oneprot_gbt_split", dev(H), *args, a[0], a[1], a[2], a[3], a[4].view(torch.uint8), ws, ws.numel(), F, B, level, 1, NN, *params)
        b = run_split_nodes(H[0], *args, level, 0, L, NN, B, params)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32), y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32)), level
        assert (a[0][0, L - 1:] != -5).all() and (a[0][0, :L - 1] == -5).all()


@functools.lru_cache(maxsize=None)
def d9_level8():
    """(H int64 [256, F, B, 2], expo, ref): the level-8 histograms of round 1 of fixture d9, from the restatement's node ids.  A row's level-8 node is its final
    node if that is of level 8 (the node did not split), the parent of its final node if that is of level 9."""
    ref = D.reference("d9")
    X, y = D.fit_data("d9")
    N, F, B = D.FITS["d9"][:3]
    tr = ref["trees"][0][0]
    m0 = np.full((N, 1), R.initial_margin(R.SQUARED, 0.5), dtype=np.float32)
    g, h = R.gradients(m0, y.reshape(N, 1), R.SQUARED)
    kept = np.ones(N, dtype=bool)
    e = R.exponent(g[:, 0], kept, R.SQUARED)
    assert e == tr["expo"]
    gq, hq = R.quantise(g[:, 0], h[:, 0], kept, e)
    p = tr["pos"]
    p8 = np.where(p >= 511, (p - 1) // 2, p).astype(np.int32)
    return hist_reference(ref["bins"], gq[None], hq[None], p8[None], 8, B)[0], e, ref


def test_split_nodes_level_8_in_two_groups():
    """fixture d9's level-8 nodes of round 1, searched as groups (0, 128) and (128, 128): each group writes the heap ids 255 + node0 + n, the children
    2 id + 1 and 2 id + 2 and nothing else; gains within 1e-12 (relative) of gbt_ref.best_split, decisions and leaf values the restatement's"""
    H, e, ref = d9_level8()
    N, F, B, depth, mcw = D.FITS["d9"][:5]
    NN, tr = 1023, ref["trees"][0][0]
    cuts = np.full((F, B - 1), np.inf, dtype=np.float32)
    for f, c in enumerate(ref["cuts"]):
        cuts[f, :len(c)] = c
    args = (dev(cuts), dev(np.asarray(ref["ncuts"], dtype=np.int32)), dev(np.ones(F, dtype=np.uint8)), dev(np.array([e], dtype=np.int32)))
    params = (mcw, 0.0, 0.0, 1.0, D.LR)
    second = run_split_nodes(H[128:], *args, 8, 128, 128, NN, B, params)
    tf = second[0][0].cpu().numpy()
    written = np.zeros(NN, dtype=bool)
    written[255 + 128:511], written[2 * (255 + 128) + 1:] = True, True
    assert (tf[~written] == -5).all() and (tf[written] != -5).all()
    for t in second[1:]:
        assert (t.view(-1)[torch.from_numpy(~written).to(DEV)] == -5).all()
    both = run_split_nodes(H[:128], *args, 8, 0, 128, NN, B, params, out=second)
    tf, tb, tt, tl, gain = (t.view(-1).cpu().numpy() for t in both)
    assert (tf[:255] == -5).all() and (tl[:255] == -5).all() and (gain[:255] == -5).all() and (tf[255:] != -5).all()
    seen = splits = 0
    for n in range(256):
        nid = 255 + n
        d = R.best_split(H[n], ref["ncuts"], np.ones(F, dtype=bool), e, min_child_weight=mcw)
        if not d["valid"]:
            assert tf[nid] == -1 and gain[nid] == -math.inf, n
            continue
        seen += 1
        assert abs(gain[nid] - d["gain"]) <= 1e-12 * abs(d["gain"]), (n, gain[nid], d["gain"])
        assert tf[nid] == tr["feat"][nid] and (tf[nid] < 0 or (tb[nid] == tr["bin"][nid] and tt[nid] == tr["thr"][nid])), n
        splits += int(tf[nid] >= 0)
        if tf[nid] >= 0:
            assert tl[2 * nid + 1] == tr["leaf"][2 * nid + 1] and tl[2 * nid + 2] == tr["leaf"][2 * nid + 2], n
    print(f"level 8 of d9, round 1: {seen} nodes with a valid candidate, {splits} split")
    assert seen >= 40 and splits == int((tr["feat"][255:511] >= 0).sum()) >= 20          # (the restatement has 50 such nodes: the comparison is not vacuous)


# ================================================================================================================== fits
def device_kwargs(name, **over):
    kw = D.fit_params(name)
    if D.FITS[name][6]:
        kw.update(subsample=D.SAMPLE_RATE, colsample_bytree=D.SAMPLE_RATE, random_state=D.SAMPLE_SEED)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def fitted(name):
    """the device fit of a fixture, computed once and shared (callers must not change it)"""
    X, y = D.fit_data(name)
    return gbt.XGBRegressor(**device_kwargs(name)).fit(X, y)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", sorted(D.FITS))
def test_deep_fit_against_the_restatement(name):
    """tree structure exactly the restatement's, the node of every row after the last level of the last round, and the margin after EVERY round bit for bit
    (reg:squarederror is single IEEE fp32 operations on both sides; measured difference 0).  The margin after round r is the walk of the first r trees over the
    training rows, which the last assertion ties to the margin the fit itself ended with."""
    ref = D.reference(name)
    model = fitted(name)
    X, _ = D.fit_data(name)
    assert model.tree_nodes == (2 << D.FITS[name][3]) - 1
    assert_same_trees(model, ref, name)
    assert np.array_equal(model.train_pos_[0].cpu().numpy(), ref["trees"][-1][0]["pos"])
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    xd = dev(X)
    for r, want in enumerate(ref["margins"]):
        part = dict(sd, **{k: sd[k][:r + 1] for k in ("tree_feat", "tree_bin", "tree_thr", "tree_leaf")})
        got = gbt.XGBRegressor().load_state_dict(part).predict_margin(xd).cpu().numpy()
        diff = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"{name} round {r + 1}: max |device margin - restatement margin| = {diff:.3e}")
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, r, diff)
    assert np.array_equal(model.train_margin_.cpu().numpy().view(np.int32), ref["margin"].view(np.int32))


@pytest.mark.parametrize("name", ["d9", "d9s"])
def test_depth_9_properties(name, monkeypatch):
    model = fitted(name)
    N, F, B = D.FITS[name][:3]
    X, y = D.fit_data(name)
    xd = dev(X)
    state = [bits(v) for v in model.state_dict().values()]
    again = gbt.XGBRegressor(**device_kwargs(name)).fit(xd, y)                                  # a second fit: the same bits
    assert torch.equal(bits(again.train_margin_), bits(model.train_margin_)) and all(torch.equal(a, bits(b)) for a, b in zip(state, again.state_dict().values()))
    monkeypatch.setenv("ONEPROT_GBT_HIST_BYTES", str(F * B * 16))                               # a budget of exactly one node: 256 groups at level 8
    assert len(gbt.plan_node_groups(F, B, 8)) == 256
    small = gbt.XGBRegressor(**device_kwargs(name)).fit(xd, y)
    monkeypatch.delenv("ONEPROT_GBT_HIST_BYTES")
    assert torch.equal(bits(small.train_margin_), bits(model.train_margin_)) and all(torch.equal(a, bits(b)) for a, b in zip(state, small.state_dict().values()))
    assert torch.equal(small.train_pos_, model.train_pos_)
    pm = model.predict_margin(xd)
    assert torch.equal(bits(pm), bits(model.train_margin_))                                     # the walk on raw rows against the fit's own margin
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    other = gbt.XGBRegressor().load_state_dict(sd)
    assert other.max_depth == 9 and torch.equal(bits(other.predict_margin(xd)), bits(pm)) and torch.equal(other.predict(xd), pm[:, 0])
    rng = np.random.default_rng(1000 + D.FITS[name][7])                                         # 400 rows the fit has not seen, half of them scaled by 3
    Xh = rng.standard_normal((400, F)).astype(np.float32)
    Xh[200:] *= np.float32(3.0)
    want = C.walk(Xh, sd["tree_feat"].numpy(), sd["tree_thr"].numpy(), sd["tree_leaf"].numpy(), model.init_margin())
    assert np.array_equal(model.predict_margin(Xh).cpu().numpy().view(np.int32), want.view(np.int32))
    assert len(np.unique(want)) > 100


def test_depth_9_decides_its_first_six_levels_as_depth_6_does():
    """round 1 of d9 against round 1 of a depth-6 fit of the same data: the same features, cuts, thresholds and node values at heap nodes 0 .. 62"""
    deep = fitted("d9").state_dict()
    X, y = D.fit_data("d9")
    shallow = gbt.XGBRegressor(**device_kwargs("d9", max_depth=6, n_estimators=1)).fit(X, y).state_dict()
    for k in ("tree_feat", "tree_bin", "tree_thr", "tree_leaf"):
        assert torch.equal(bits(deep[k][0, 0, :63]), bits(shallow[k][0, 0, :63])), k
    assert (deep["tree_feat"][0, 0, :63] >= 0).sum() >= 32


def test_classifier_and_depth_10_stay_refused():
    with pytest.raises(NotImplementedError):
        gbt.XGBClassifier(max_depth=7)
    with pytest.raises(NotImplementedError):
        gbt.XGBRegressor(max_depth=10)
    bins = torch.zeros(4, 1, dtype=torch.uint8, device=DEV)
    z = torch.zeros(4, dtype=torch.int32, device=DEV)
    for level in (5, 9):                                                       # the deep entry points take levels 6 .. 8 only
        with pytest.raises(hip.HipKernelError):
            hip.call("oneprot_gbt_node_keys", z, z.clone(), 4, level)
    with pytest.raises(hip.HipKernelError):                                    # a group that leaves the level
        hip.call("oneprot_gbt_hist_nodes", bins, z, z, z, z, torch.zeros(65, dtype=torch.int32, device=DEV), torch.zeros(64, dtype=torch.int64, device=DEV), 4, 1, 2, 6, 60, 5, 0)
