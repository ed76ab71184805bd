"""ProNet, the graph tower of the pocket / struct_graph modalities (ref src/models/components/struct_graph_encoder.py:5-42 wraps
`dig.threedgraph.method.ProNet`; configs/model/components/{pocket,struct_graph}.yaml), on the HIP kernels of csrc/pronet.hip in both directions.

DIG is not vendored and its parity is UNPINNED: the arithmetic is the published model's (Wang et al., "Learning Hierarchical Protein Representations
via Complete 3D Graph Networks", ICLR 2023) restated, and tests/pronet_ref.py -- an fp64 plain-torch restatement under autograd -- is the oracle
(DESIGN.md section 7 lists every unpinned choice).  Built: level='backbone', num_spherical == 2, max_num_neighbors <= 32, hidden_channels a multiple of
64 up to 256, mid_emb <= 128, num_radial <= 8; everything else raises NotImplementedError before the device is touched.

`ProNet(...)(batch) -> fp32 [num_graphs, out_channels]`; `batch` is an oneprot_amd.graph_data.GraphBatch or anything with the attribute names of the PyG
Batch the reference builds (x, coords_ca, coords_n, coords_c, bb_embs, batch, num_graphs).  It is a torch.nn.Module with plain fp32 parameters under
the published module names; the arithmetic of a call is ONE torch.autograd.Function whose forward records a tape of kernel launches and whose backward
replays it in reverse: node linears on oneprot_sgemm (their weight gradients, which contract over the nodes, on oneprot_wgrad_f32), everything per edge in the fused convolution kernels, which never write the [E, h] edge weights
or messages.  No float atomics and no host read-back: a step is a pure function of (inputs, parameters, RNG position).

Train-mode noise and dropout (module in train mode only) draw from the library's Philox streams under rng.py's domain "pronet"; `rng_state()` / `set_rng_state()`
carry the position.  Same distribution as torch's, another draw."""
import math

import torch
from torch import nn

from . import hip
from .rng import DOMAINS, StreamOwner

SLOTS = hip._consts["PRONET_SLOTS"]
ACT_NONE, ACT_SWISH, ACT_RELU = 0, 1, 2
RNG_DOMAIN_PRONET = DOMAINS["pronet"]
NOISE_SIGMA, NOISE_CLIP = 0.025, 0.1


# ---- the radial basis' constants, fp64 on the host ----------------------------------------------------------------------------------------------------
def _sph_jn(l, x):
    if l == 0:
        return math.sin(x) / x
    if l == 1:
        return math.sin(x) / (x * x) - math.cos(x) / x
    return 3.0 / x * _sph_jn(1, x) - _sph_jn(0, x)        # l == 2, by the recurrence


def bessel_constants(num_radial):
    """(zeros [2][num_radial], norms [2][num_radial]): z_{l,n} the n-th positive zero of the spherical Bessel function j_l (l = 0, 1) and
    sqrt(2) / |j_{l+1}(z_{l,n})|, which makes the radial functions orthonormal on [0, 1] under the weight d^2."""
    zeros = [[(n + 1) * math.pi for n in range(num_radial)], []]
    for n in range(1, num_radial + 1):                   # j_1(x) = 0  <=>  tan x = x: one root in (n pi, (n + 1/2) pi)
        lo, hi = n * math.pi, (n + 0.5) * math.pi
        f = lambda x: math.sin(x) - x * math.cos(x)     # noqa: E731  (x^2 j_1(x))
        flo = f(lo)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if (f(mid) > 0) == (flo > 0):
                lo = mid
            else:
                hi = mid
        zeros[1].append(0.5 * (lo + hi))
    norms = [[math.sqrt(2.0) / abs(_sph_jn(l + 1, z)) for z in zeros[l]] for l in (0, 1)]
    return zeros, norms


def feature_constants(num_radial, num_pos_emb):
    """the fp32 table oneprot_pronet_edge_features reads: zeros, normalisers, then the num_pos_emb / 2 frequencies exp(-2 k ln(10000) / num_pos_emb)"""
    zeros, norms = bessel_constants(num_radial)
    freq = [math.exp(-2.0 * k * math.log(10000.0) / num_pos_emb) for k in range(num_pos_emb // 2)]
    return torch.tensor(zeros[0] + zeros[1] + norms[0] + norms[1] + freq, dtype=torch.float64).to(torch.float32)


# ---- parameter containers: the published module names, nothing else ------------------------------------------------------------------------------------
class _TwoLinear(nn.Module):
    def __init__(self, f, mid, h):
        super().__init__()
        self.lin1 = nn.Linear(f, mid, bias=False)
        self.lin2 = nn.Linear(mid, h, bias=False)


class _EdgeGraphConv(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.lin_l = nn.Linear(h, h)
        self.lin_r = nn.Linear(h, h, bias=False)


class _InteractionBlock(nn.Module):
    def __init__(self, h, mid, widths, int_emb_layers):
        super().__init__()
        for c, f in enumerate(widths):
            setattr(self, f"conv{c}", _EdgeGraphConv(h))
            setattr(self, f"lin_feature{c}", _TwoLinear(f, mid, h))
        self.lin_1, self.lin_2 = nn.Linear(h, h), nn.Linear(h, h)
        self.lin0, self.lin1, self.lin2 = nn.Linear(h, h), nn.Linear(h, h), nn.Linear(h, h)
        self.lins_cat = nn.ModuleList([nn.Linear(3 * h, h)] + [nn.Linear(h, h) for _ in range(int_emb_layers - 1)])
        self.lins = nn.ModuleList([nn.Linear(h, h) for _ in range(int_emb_layers - 1)])
        self.final = nn.Linear(h, h)


# ---- the graph of a batch ------------------------------------------------------------------------------------------------------------------------------
class Graph:
    """device-side geometry of one batch: nbr / deg by target, src_off / src_list by source, the three feature arrays [32 N, width]"""

    def __init__(self, batch, cutoff, max_num_neighbors, consts, num_radial, num_pos_emb, euler=None):
        dev = batch.coords_ca.device
        self.N, self.G = int(batch.coords_ca.shape[0]), int(batch.num_graphs)
        self.batch32 = batch.batch.to(torch.int32).contiguous()
        ptr = getattr(batch, "ptr", None)
        if ptr is None:                                                       # a non-decreasing `batch`: per-graph offsets without a host read-back
            ptr = torch.searchsorted(batch.batch.contiguous(), torch.arange(self.G + 1, device=dev, dtype=batch.batch.dtype))
        self.ptr32 = ptr.to(torch.int32).contiguous()
        N = self.N
        self.ca, self.cn, self.cc = (getattr(batch, k).to(torch.float32).contiguous() for k in ("coords_ca", "coords_n", "coords_c"))
        self.nbr = torch.empty(N, SLOTS, dtype=torch.int32, device=dev)
        self.deg = torch.empty(N, dtype=torch.int32, device=dev)
        hip.call("oneprot_radius_graph", self.ca, self.ptr32, self.batch32, self.nbr, self.deg, N, self.G, float(cutoff), int(max_num_neighbors))
        self.src_off = torch.empty(N + 1, dtype=torch.int32, device=dev)
        self.src_list = torch.empty(N * SLOTS, dtype=torch.int32, device=dev)
        count_ws = torch.empty(N, dtype=torch.int32, device=dev)
        hip.call("oneprot_graph_by_source", self.ptr32, self.batch32, self.nbr, self.deg, count_ws, self.src_off, self.src_list, N, self.G)
        self.widths = (4 * num_radial, 6 * num_radial, num_pos_emb)
        self.feat = [torch.empty(N * SLOTS, w, dtype=torch.float32, device=dev) for w in self.widths]
        noise, seed, stream = (1, euler[0], euler[1]) if euler is not None else (0, 0, 0)
        hip.call("oneprot_pronet_edge_features", self.ca, self.cn, self.cc, self.nbr, self.deg, consts, self.feat[0], self.feat[1], self.feat[2], N, num_radial,
                 num_pos_emb, float(cutoff), noise, NOISE_SIGMA, NOISE_CLIP, seed, stream)


# ---- the tape: every forward op appends the closure that is its backward ---------------------------------------------------------------------------------
class _Tape:
    def __init__(self, record):
        self.record, self.ops, self.grads, self.pgrads = record, [], {}, {}

    def acc(self, t, g):
        cur = self.grads.get(id(t))
        if cur is None:
            self.grads[id(t)] = g
        else:
            hip.call("oneprot_dropout_add_f32", g, cur, cur, cur.numel(), 0.0, 0, 0)          # p = 0: the plain sum

    def backward(self):
        for op in reversed(self.ops):
            op()


def _colsum(x, out):
    M, n = x.shape
    ws = torch.empty(hip.query("oneprot_colsum_f32_workspace", M, n), dtype=torch.uint8, device=x.device)
    hip.call("oneprot_colsum_f32", x, out, ws, ws.numel(), M, n)


def _sgemm(A, B, C, M, N, K, transA, b_is_kn, accumulate=0):
    hip.call("oneprot_sgemm", A, B, C, M, N, K, transA, b_is_kn, 1.0, accumulate)


def _wgrad(dz, x, dW):
    """dW = dz^T x over every row of the batch, blocked over the rows: one sgemm chain of N terms rounds 6 to 36 times worse at N = 8193"""
    M, n, k = dz.shape[0], dz.shape[1], x.shape[1]
    ws = torch.empty(hip.query("oneprot_wgrad_f32_workspace", M, n, k), dtype=torch.uint8, device=dz.device)
    hip.call("oneprot_wgrad_f32", dz, x, dW, ws, ws.numel(), M, n, k)


def _linear(tape, pairs, bias, act, resid=None, into=None, needs_dx=True):
    """y = act(sum_k x_k W_k^T + bias) (+ resid).  pairs: [(x [M, K], W parameter [n, K])]; into = (buffer [M, ld], column offset): y is that column
    block (torch.cat by placement).  Returns y, or the buffer."""
    x0, W0 = pairs[0]
    M, n = x0.shape[0], W0.shape[0]
    z = torch.empty(M, n, dtype=torch.float32, device=x0.device)
    for k, (x, W) in enumerate(pairs):
        _sgemm(x, W, z, M, n, x.shape[1], 0, 0, accumulate=int(k > 0))
    plain = act == ACT_NONE and resid is None and into is None
    if into is not None:
        ybuf, off = into
    else:
        ybuf, off = (z if plain else torch.empty_like(z)), 0
    ld = ybuf.shape[1]
    if not plain or bias is not None:
        hip.call("oneprot_pronet_bias_act", z, bias, resid, None if plain else ybuf.data_ptr() + 4 * off, M, n, ld, act)
    if tape.record:
        def bwd():
            g = tape.grads[id(ybuf)]
            if plain:
                dz = g
            else:
                dz = torch.empty_like(z)
                hip.call("oneprot_pronet_act_bwd", g.data_ptr() + 4 * off, z, dz, M, n, ld, act)
                if resid is not None:
                    tape.acc(resid, g)
            if bias is not None:
                db = torch.empty_like(bias)
                _colsum(dz, db)
                tape.pgrads[bias] = db
            for x, W in pairs:
                K = x.shape[1]
                dW = torch.empty_like(W)
                _wgrad(dz, x, dW)                                             # dW = dz^T x
                tape.pgrads[W] = dW
                if needs_dx:
                    dx = torch.empty_like(x)
                    _sgemm(dz, W, dx, M, K, n, 0, 1)                          # dx = dz W
                    tape.acc(x, dx)
        tape.ops.append(bwd)
    return ybuf


def _edge_conv(tape, graph, c, a, two):
    """m_i = sum_e (W2 W1 f_e) * a_j, the TwoLinear folded into one [F, h] operand on the host GEMM"""
    W1, W2 = two.lin1.weight, two.lin2.weight
    N, h, F, mid = graph.N, a.shape[1], W1.shape[1], W1.shape[0]
    feat = graph.feat[c]
    WfT = torch.empty(F, h, dtype=torch.float32, device=a.device)
    _sgemm(W1, W2, WfT, F, h, mid, 1, 0)                                      # (W2 W1)^T = W1^T W2^T
    m = torch.empty_like(a)
    hip.call("oneprot_edge_conv_fwd", feat, WfT, a, graph.nbr, graph.deg, m, N, h, F)
    if tape.record:
        def bwd():
            dm = tape.grads.pop(id(m))
            da = torch.empty_like(a)
            hip.call("oneprot_edge_conv_bwd_x", feat, WfT, dm, graph.src_off, graph.src_list, da, N, h, F)
            tape.acc(a, da)
            ws = torch.empty(hip.query("oneprot_edge_conv_bwd_w_workspace", N, h, F), dtype=torch.uint8, device=a.device)
            dWfT = torch.empty_like(WfT)
            hip.call("oneprot_edge_conv_bwd_w", feat, a, dm, graph.nbr, graph.deg, dWfT, ws, ws.numel(), N, h, F)
            dW2, dW1 = torch.empty_like(W2), torch.empty_like(W1)
            _sgemm(dWfT, W1, dW2, h, mid, F, 1, 0)                            # dW2 = dWf W1^T
            _sgemm(W2, dWfT, dW1, mid, F, h, 1, 0)                            # dW1 = W2^T dWf
            tape.pgrads[W1], tape.pgrads[W2] = dW1, dW2
        tape.ops.append(bwd)
    return m


def _dropout(tape, x, p, seed, stream):
    y = torch.empty_like(x)
    hip.call("oneprot_dropout_f32", x, y, x.numel(), float(p), seed, stream)
    if tape.record:
        def bwd():
            g = tape.grads.pop(id(y))
            dx = torch.empty_like(g)
            hip.call("oneprot_dropout_f32", g, dx, g.numel(), float(p), seed, stream)       # the same mask and scale
            tape.acc(x, dx)
        tape.ops.append(bwd)
    return y


def _noise_add(tape, x, seed, stream):
    y = torch.empty_like(x)
    hip.call("oneprot_clipped_normal_add_f32", x, y, x.numel(), NOISE_SIGMA, NOISE_CLIP, seed, stream)
    if tape.record:
        tape.ops.append(lambda: tape.acc(x, tape.grads.pop(id(y))))
    return y


class _ProNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tower, batch, rng, record, *params):
        tape = _Tape(record)
        out = tower._run(tape, batch, rng)
        ctx.tape, ctx.params, ctx.out = tape, params, out
        return out.clone()                                                     # the tape keys gradients by buffer identity: keep `out` its own

    @staticmethod
    def backward(ctx, dout):
        tape = ctx.tape
        if not tape.record:
            raise RuntimeError("ProNet: backward of a forward that recorded no tape, or a second backward through the same forward (the tape is played once)")
        tape.grads[id(ctx.out)] = dout.contiguous().to(torch.float32)
        tape.backward()
        grads = tuple(tape.pgrads.get(p) if p.requires_grad else None for p in ctx.params)
        tape.ops, tape.grads, tape.pgrads, tape.record = [], {}, {}, False
        return (None, None, None, None) + grads


class ProNet(StreamOwner, nn.Module):
    def __init__(self, level="aminoacid", num_blocks=4, hidden_channels=128, out_channels=1, mid_emb=64, num_radial=6, num_spherical=2, cutoff=10.0,
                 max_num_neighbors=32, int_emb_layers=3, out_layers=2, num_pos_emb=16, dropout=0, data_augment_eachlayer=False, euler_noise=False):
        super().__init__()
        if level != "backbone":
            raise NotImplementedError(f"ProNet(level={level!r}): only level='backbone' is built (both shipped configs use it); 'aminoacid' feeds no "
                                      "backbone angles and 'allatom' adds side-chain torsions to the node input")
        if num_spherical != 2:
            raise NotImplementedError(f"ProNet(num_spherical={num_spherical}): the feature kernel writes the l = 0, 1 harmonics in closed form; only 2 is built")
        if not 1 <= max_num_neighbors <= SLOTS:
            raise NotImplementedError(f"ProNet(max_num_neighbors={max_num_neighbors}): the edge table is {SLOTS} slots wide")
        if hidden_channels % 64 or not 64 <= hidden_channels <= 256:
            raise NotImplementedError(f"ProNet(hidden_channels={hidden_channels}): the convolution kernels run one thread per channel, a multiple of 64 up to 256")
        if not 1 <= mid_emb <= 128:
            raise NotImplementedError(f"ProNet(mid_emb={mid_emb}): built for mid_emb <= 128")
        if not 1 <= num_radial <= 8:
            raise NotImplementedError(f"ProNet(num_radial={num_radial}): the feature widths 4 and 6 num_radial must fit the kernels' 48 registers: <= 8")
        if num_pos_emb % 2 or not 2 <= num_pos_emb <= 48:
            raise NotImplementedError(f"ProNet(num_pos_emb={num_pos_emb}): an even width up to 48")
        if num_blocks < 1 or int_emb_layers < 1 or out_layers < 1 or out_channels < 1:
            raise NotImplementedError("ProNet: num_blocks, int_emb_layers, out_layers and out_channels must be at least 1")
        if not 0 <= float(dropout) < 1:
            raise NotImplementedError(f"ProNet(dropout={dropout}): a probability in [0, 1)")
        h = hidden_channels
        self.level, self.num_blocks, self.hidden_channels, self.out_channels, self.mid_emb = level, num_blocks, h, out_channels, mid_emb
        self.num_radial, self.num_spherical, self.cutoff, self.max_num_neighbors = num_radial, num_spherical, float(cutoff), max_num_neighbors
        self.int_emb_layers, self.out_layers, self.num_pos_emb, self.dropout = int_emb_layers, out_layers, num_pos_emb, float(dropout)
        self.data_augment_eachlayer, self.euler_noise = bool(data_augment_eachlayer), bool(euler_noise)
        widths = (4 * num_radial, 6 * num_radial, num_pos_emb)
        self.embedding = nn.Linear(26 + 6, h)
        self.interaction_blocks = nn.ModuleList([_InteractionBlock(h, mid_emb, widths, int_emb_layers) for _ in range(num_blocks)])
        self.lins_out = nn.ModuleList([nn.Linear(h, h) for _ in range(out_layers - 1)])
        self.lin_out = nn.Linear(h, out_channels)
        self.register_buffer("feature_consts", feature_constants(num_radial, num_pos_emb), persistent=False)
        self._init_streams(fixed_seed=True)

    # ---- RNG position ----
    def stream_of(self, call, site):
        """the Philox stream of draw `site` of forward call `call`: site 0 the Euler noise, 1 + 2 b the node noise of block b, 2 + 2 b its dropout,
        1 + 2 num_blocks + k the dropout of readout layer k"""
        return self._rng_stream(RNG_DOMAIN_PRONET, call * (2 * self.num_blocks + self.out_layers + 1) + site)

    # ---- forward ----
    @staticmethod
    def check_input(batch):
        for k in ("x", "coords_ca", "coords_n", "coords_c", "bb_embs", "batch", "num_graphs"):
            if not hasattr(batch, k):
                raise TypeError(f"ProNet: the batch has no attribute {k!r} (a GraphBatch or a PyG Batch of the reference's struct graphs)")
        n = batch.coords_ca.shape[0]
        if n < 1 or batch.x.shape[0] != n or batch.bb_embs.shape != (n, 6) or batch.batch.shape != (n,):
            raise ValueError("ProNet: x [N, 1], coords_* [N, 3], bb_embs [N, 6] and batch [N] must agree on N >= 1")

    def forward(self, batch):
        self.check_input(batch)
        rng = None
        if self.training and (self.dropout > 0 or self.data_augment_eachlayer or self.euler_noise):
            rng = (self._drop_seed, self._next_call())
        params = tuple(self.parameters())
        record = torch.is_grad_enabled() and any(p.requires_grad for p in params)       # grad mode is off inside Function.forward: decided here
        return _ProNetFn.apply(self, batch, rng, record, *params)

    def _run(self, tape, batch, rng):
        h, G = self.hidden_channels, int(batch.num_graphs)
        seed, call = rng if rng is not None else (0, 0)
        euler = (seed, self.stream_of(call, 0)) if rng is not None and self.euler_noise else None
        graph = Graph(batch, self.cutoff, self.max_num_neighbors, self.feature_consts, self.num_radial, self.num_pos_emb, euler)
        N, dev = graph.N, graph.ca.device
        # a. node input
        z = batch.x[:, 0].to(torch.int64).contiguous()
        bb = batch.bb_embs.to(torch.float32).contiguous()
        x = torch.empty(N, h, dtype=torch.float32, device=dev)
        emb = self.embedding
        feat32 = torch.empty(N, 32, dtype=torch.float32, device=dev) if tape.record else None
        hip.call("oneprot_pronet_embed_fwd", z, bb, emb.weight, emb.bias, x, feat32, N, h)
        if tape.record:
            x0 = x

            def embed_bwd():
                g = tape.grads.pop(id(x0))
                dW, db = torch.empty_like(emb.weight), torch.empty_like(emb.bias)
                _wgrad(g, feat32, dW)
                _colsum(g, db)
                tape.pgrads[emb.weight], tape.pgrads[emb.bias] = dW, db
            tape.ops.append(embed_bwd)
        # e. interaction blocks
        for b, blk in enumerate(self.interaction_blocks):
            if rng is not None and self.data_augment_eachlayer:
                x = _noise_add(tape, x, seed, self.stream_of(call, 1 + 2 * b))
            a = _linear(tape, [(x, blk.lin_1.weight)], blk.lin_1.bias, ACT_SWISH)
            s = _linear(tape, [(x, blk.lin_2.weight)], blk.lin_2.bias, ACT_SWISH)
            H = torch.empty(N, 3 * h, dtype=torch.float32, device=dev)
            for c in range(3):
                conv = getattr(blk, f"conv{c}")
                m = _edge_conv(tape, graph, c, a, getattr(blk, f"lin_feature{c}"))
                g = _linear(tape, [(m, conv.lin_l.weight), (a, conv.lin_r.weight)], conv.lin_l.bias, ACT_NONE)
                lin = getattr(blk, f"lin{c}")
                _linear(tape, [(g, lin.weight)], lin.bias, ACT_SWISH, into=(H, c * h))
            if rng is not None and self.dropout > 0:
                H = _dropout(tape, H, self.dropout, seed, self.stream_of(call, 2 + 2 * b))
            t = H
            last = len(blk.lins_cat) - 1
            for k, lin in enumerate(blk.lins_cat):
                t = _linear(tape, [(t, lin.weight)], lin.bias, ACT_SWISH, resid=s if k == last else None)
            for lin in blk.lins:
                t = _linear(tape, [(t, lin.weight)], lin.bias, ACT_SWISH)
            x = _linear(tape, [(t, blk.final.weight)], blk.final.bias, ACT_NONE)
        # f. readout
        y = torch.empty(G, h, dtype=torch.float32, device=dev)
        hip.call("oneprot_segment_sum_f32", x, graph.ptr32, y, G, h)
        if tape.record:
            xin, y0 = x, y

            def pool_bwd():
                g = tape.grads.pop(id(y0))
                dx = torch.empty_like(xin)
                hip.call("oneprot_segment_sum_bwd_f32", g, graph.batch32, dx, N, h)
                tape.acc(xin, dx)
            tape.ops.append(pool_bwd)
        for k, lin in enumerate(self.lins_out):
            y = _linear(tape, [(y, lin.weight)], lin.bias, ACT_RELU)
            if rng is not None and self.dropout > 0:
                y = _dropout(tape, y, self.dropout, seed, self.stream_of(call, 1 + 2 * self.num_blocks + k))
        return _linear(tape, [(y, self.lin_out.weight)], self.lin_out.bias, ACT_NONE)

    def extra_repr(self):
        return (f"level={self.level!r}, num_blocks={self.num_blocks}, hidden_channels={self.hidden_channels}, out_channels={self.out_channels}, "
                f"cutoff={self.cutoff}, max_num_neighbors={self.max_num_neighbors}, dropout={self.dropout}")
