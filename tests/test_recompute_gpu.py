"""Activation recomputation of trainable ESM towers on the MI355X: the same module state on the same batch, once with every layer's activations kept and once
with `k`-layer segments recomputed inside the backward.  The recompute pass issues the forward's own launches on the forward's own inputs, so every
comparison below is torch.equal -- features, loss and every gradient -- never a tolerance."""
import functools

import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.esm import recompute_plan
from oneprot_amd.packing import PackedTokens
from tests.cases import esm_dir

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = {            # name: (layers, hidden, heads, ffn)
    "hd16": (6, 320, 20, 1280),
    "hd32": (4, 640, 20, 2560),
    "hd24": (4, 480, 20, 1920),
    "hd64": (3, 1280, 20, 5120),
    "hd16x12": (12, 320, 20, 1280),
}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.delenv("ONEPROT_RECOMPUTE_LAYERS", raising=False)
    monkeypatch.delenv("ONEPROT_FFN2_LN", raising=False)


def _ffn2(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("ONEPROT_FFN2_LN", raising=False)
    else:
        monkeypatch.setenv("ONEPROT_FFN2_LN", mode)


def _esm_dir(tmp, shape):
    return esm_dir(tmp, shape, *SHAPES[shape])


def _row(n, L, gen):
    """one padded row of n real tokens: cls, residues, eos, then pad"""
    ids = torch.full((L,), 1, dtype=torch.int64)
    ids[:n] = torch.randint(4, 24, (n,), generator=gen)
    ids[0] = 0
    if n > 1:
        ids[n - 1] = 2
    return ids


def _padded(lengths, L, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([_row(n, L, gen) for n in lengths]).to(DEV)


def _packed(lengths, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return PackedTokens.from_list([_row(n, n, gen) for n in lengths]).to(DEV)


def _encoder(tmp, shape, seed=0, **kw):
    from oneprot_amd.encoders import SequenceEncoder
    torch.manual_seed(seed)
    args = dict(output_dim=128, pooling_type="mean", proj_type="mlp", use_logit_scale=True, learnable_logit_scale=True, use_lora=False, frozen=False)
    args.update(kw)
    enc = SequenceEncoder(_esm_dir(tmp, shape), **args)
    with torch.no_grad():      # biases and LayerNorm gains off their initial 0 / 1, so that every gradient is a generic number
        for name, v in enc.transformer.named_views().items():
            if name.endswith(".bias"):
                v.normal_(0, 0.02)
            elif name.endswith("LayerNorm.weight"):
                v.add_(torch.randn_like(v) * 0.05)
    return enc.to(DEV).train()


class _Spy:
    """counts the recompute passes of a tower and keeps the `saved` record of its last application"""

    def __init__(self, tr):
        self.tr, self.segments, self.saved, self.bounds = tr, [], None, None
        rec, run = tr._recompute_segment, tr.run_layers

        def recompute(saved, lo, hi):
            self.segments.append((lo, hi))
            return rec(saved, lo, hi)

        def run_layers(ids, save):
            x, saved = run(ids, save)
            self.saved = saved
            self.bounds = dict(saved["bounds"]) if saved is not None and "bounds" in saved else None      # as the forward left them (the backward drops them)
            return x, saved

        tr._recompute_segment, tr.run_layers = recompute, run_layers

    def remove(self):
        del self.tr._recompute_segment, self.tr.run_layers


def _side(enc, batches, weights, k, rng=None):
    """features, loss and every gradient of sum_b <enc(batch_b), weight_b> with recomputation set to k"""
    tr = enc.transformer
    if rng is not None:
        tr.set_rng_state(rng)
    enc.set_activation_recompute(k)
    enc.zero_grad(set_to_none=True)
    feats = [enc(b) for b in batches]
    loss = sum((f * w).sum() for f, w in zip(feats, weights))
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone()}
    for j, f in enumerate(feats):
        out[f"features{j}"] = f.detach().clone()
    for name, p in enc.named_parameters():
        if p.grad is not None:
            out["grad:" + name] = p.grad.detach().clone()
    enc.set_activation_recompute(None)
    return out


def _assert_equal(on, off, need):
    assert set(on) == set(off)
    for key in need:
        assert any(k_ == "grad:" + key or k_.startswith("grad:" + key) for k_ in on), (key, sorted(on))
    for key in off:
        assert torch.isfinite(off[key]).all(), key
        assert torch.equal(on[key], off[key]), (key, float((on[key].double() - off[key].double()).abs().max()))
    g = off["grad:transformer.flat"]
    assert float(g.abs().max()) > 0


HEAD_GRADS = ("transformer.flat", "proj.", "norm.1.log_logit_scale")
_cache = {}


def _case(tmp_path_factory, shape, mode, batch, build=_encoder, **kw):
    """(encoder, batch, weight, reference side) -- built and run with recomputation off ONCE per (shape, FFN-2 form, batch), shared by every k"""
    key = (shape, mode, batch, tuple(sorted(kw.items())))
    if key not in _cache:
        enc = build(tmp_path_factory.mktemp("esm"), shape, **kw)
        ids = BATCHES[batch]()
        torch.manual_seed(11)
        w = torch.randn(len(ids) if isinstance(ids, PackedTokens) else ids.shape[0], 128, device=DEV)
        rng = enc.transformer.rng_state()
        _cache[key] = (enc, ids, w, rng, _side(enc, [ids], [w], 0, rng))
    return _cache[key]


BATCHES = {
    "t512": lambda: _padded([128, 127, 65, 3], 128),            # T = 512
    "t256": lambda: _padded([128, 65], 128),                    # T = 256
    "packed": lambda: _packed([1, 127, 128, 129, 300]),         # T_pad = 768
    "t2048": lambda: _padded([256, 255, 129, 3, 256, 200, 64, 17], 256),
}


def _check_against_off(tmp_path_factory, shape, mode, batch, k, need=HEAD_GRADS, **kw):
    enc, ids, w, rng, off = _case(tmp_path_factory, shape, mode, batch, **kw)
    spy = _Spy(enc.transformer)
    try:
        on = _side(enc, [ids], [w], k, rng)
    finally:
        spy.remove()
    plan = recompute_plan(enc.transformer.n_layers, k)
    assert spy.segments == list(reversed(plan[:-1]))            # every lower segment re-run once, from the top down; the top one never
    _assert_equal(on, off, need)
    return enc, spy, on, off


# ------------------------------------------------------------------------------------------------------------------ 1. hd 16
@pytest.mark.parametrize("k", [1, 2, 4, 6, 9])
@pytest.mark.parametrize("mode", [None, "force"])
def test_hd16(tmp_path_factory, monkeypatch, mode, k):
    """6 layers of 320 / 20 heads / 1280 on rows of 128, 127, 65 and 3 tokens.  Under `force` the FFN-2 launch writes the next layer's LayerNorm, so at
    k = 1 a (h1, stats) pair crosses every boundary.  (The out-projection of this width, K = 320, is no whole number of the 8-phase GEMM's 128-wide
    K-steps and keeps its LayerNorm launch; the hd 64 case below runs that form.)"""
    _ffn2(monkeypatch, mode)
    enc, spy, _, _ = _check_against_off(tmp_path_factory, "hd16", mode, "t512", k)
    if mode == "force":
        assert spy.saved["forms"] == dict(fused_ln=False, ffn2_ln=True, outproj_ln8=False)
        if k < 6:
            assert all(b["h1"] is not None and b["stats"] is not None for lo, b in spy.bounds.items() if lo > 0) and spy.bounds[0]["h1"] is None


# ------------------------------------------------------------------------------------------------------------------ 2. hd 32
@pytest.mark.parametrize("k", [1, 3])
def test_hd32_full_row_outproj(tmp_path_factory, monkeypatch, k):
    """640 wide: the full-row out-projection + LayerNorm kernel, with the FFN-2 + LayerNorm form behind it"""
    _ffn2(monkeypatch, "force")
    enc, spy, _, _ = _check_against_off(tmp_path_factory, "hd32", "force", "t512", k)
    assert spy.saved["forms"] == dict(fused_ln=True, ffn2_ln=True, outproj_ln8=False)


# ------------------------------------------------------------------------------------------------------------------ 3. hd 24 (padded heads)
def test_hd24_padded_heads(tmp_path_factory):
    enc, _, _, _ = _check_against_off(tmp_path_factory, "hd24", None, "t512", 2)
    assert enc.transformer._padded


# ------------------------------------------------------------------------------------------------------------------ 4. hd 64
def test_hd64_outproj_ln8(tmp_path_factory, monkeypatch):
    """1280 wide: the out-projection + LayerNorm through the 8-phase GEMM with four column tiles"""
    _ffn2(monkeypatch, "force")
    enc, spy, _, _ = _check_against_off(tmp_path_factory, "hd64", "force", "t256", 2)
    assert spy.saved["forms"] == dict(fused_ln=False, ffn2_ln=True, outproj_ln8=True)


# ------------------------------------------------------------------------------------------------------------------ 5. packed
@pytest.mark.parametrize("k", [1, 4])
def test_packed(tmp_path_factory, k):
    enc, ids, _, _, _ = _case(tmp_path_factory, "hd16", None, "packed")
    assert ids.T_pad == 768
    _check_against_off(tmp_path_factory, "hd16", None, "packed", k)


# ------------------------------------------------------------------------------------------------------------------ 6. LoRA
def _lora_encoder(tmp, shape, lora_dropout=0.0):
    enc = _encoder(tmp, shape, use_lora=True, frozen=True, lora_dropout=lora_dropout)
    with torch.no_grad():
        enc.transformer.lora_B.normal_(0, 0.05)                # B = 0 at construction would leave dA = 0
    return enc


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_lora(tmp_path_factory, p):
    """p = 0: the merged operand; p = 0.1 in train mode: peft's two branches, whose dropout masks the recompute pass regenerates from the forward's own
    call id -- both sides start from one rng_state(), and a forward advances the call counter once"""
    enc, ids, w, rng, off = _case(tmp_path_factory, "hd16", None, "t512", build=_lora_encoder, lora_dropout=p)
    tr = enc.transformer
    assert tr._lora_two_branch() == (p > 0)
    calls = rng["_lora_calls"]
    enc, spy, on, _ = _check_against_off(tmp_path_factory, "hd16", None, "t512", 2, need=("transformer.flat", "transformer.lora_A", "transformer.lora_B", "proj."),
                                         build=_lora_encoder, lora_dropout=p)
    assert tr._lora_calls == calls + (1 if p > 0 else 0)
    assert ("lora_call" in spy.saved) == (p > 0)
    assert float(on["grad:transformer.lora_A"].abs().max()) > 0 and float(on["grad:transformer.lora_B"].abs().max()) > 0
    if p > 0:      # the masks matter: another call id gives other gradients
        other = _side(enc, [ids], [w], 2, dict(rng, _lora_calls=calls + 5))
        assert not torch.equal(other["grad:transformer.lora_A"], off["grad:transformer.lora_A"])


# ------------------------------------------------------------------------------------------------------------------ 7. two applications
def test_two_applications_in_one_graph(tmp_path_factory):
    """the seqsim pattern: one tower applied to two batches, the losses summed, one backward"""
    enc, ids_a, w_a, rng, _ = _case(tmp_path_factory, "hd16", None, "t512")
    ids_b = _padded([90, 128, 2, 77], 128, seed=5)
    torch.manual_seed(12)
    w_b = torch.randn(4, 128, device=DEV)
    off = _side(enc, [ids_a, ids_b], [w_a, w_b], 0, rng)
    spy = _Spy(enc.transformer)
    try:
        on = _side(enc, [ids_a, ids_b], [w_a, w_b], 2, rng)
    finally:
        spy.remove()
    assert spy.segments == [(2, 4), (0, 2), (2, 4), (0, 2)]
    _assert_equal(on, off, HEAD_GRADS)


# ------------------------------------------------------------------------------------------------------------------ 8. whole sub-step
def test_training_steps_with_fused_adam(tmp_path_factory):
    from oneprot_amd.data import SyntheticPairs
    from oneprot_amd.encoders import SequenceEncoder, StructTokenEncoder
    from oneprot_amd.module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    path = _esm_dir(tmp_path_factory.mktemp("esm"), "hd16")

    def build():
        torch.manual_seed(4)
        seq = SequenceEncoder(path, output_dim=128, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
        st = StructTokenEncoder(path, output_dim=128, pooling_type="mean", proj_type="linear", use_logit_scale=True, learnable_logit_scale=True)
        return OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                                use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV).train()

    m_off, m_on = build(), build()
    m_on.load_state_dict(m_off.state_dict())
    spies = {}
    for name, enc in m_on.network.items():
        enc.set_activation_recompute(2)
        spies[name] = _Spy(enc.transformer)
    batches = [{"struct_token": tuple(t.to(DEV) if torch.is_tensor(t) else t for t in b)} for b in SyntheticPairs("struct_token", 4, 128, n_batches=2, seed=9, ragged=True)]
    for step, batch in enumerate(batches):      # the second step re-uses the persistent arena-gradient buffer of the first
        l_off = m_off.training_step(batch, step)
        l_on = m_on.training_step(batch, step)
        torch.cuda.synchronize()
        assert torch.equal(l_off.detach(), l_on.detach())
        sd_off, sd_on = m_off.state_dict(), m_on.state_dict()
        assert set(sd_off) == set(sd_on)
        for key in sd_off:
            assert torch.equal(sd_off[key], sd_on[key]), (step, key)
        for name, spy in spies.items():
            assert spy.segments == [(2, 4), (0, 2)] * (step + 1), name
    sd0 = build().state_dict()
    assert any(not torch.equal(sd0[k_], sd_on[k_]) for k_ in sd0 if "struct_token.transformer" in k_)      # the tower did train
    assert hip.sched_error() == 0


# ------------------------------------------------------------------------------------------------------------------ 9. overlap stub
class _OverlapStub:
    def __init__(self):
        self.ranges = []

    def reduce_range(self, param, grad, lo, hi):
        self.ranges.append((lo, hi))


def test_wait_free_forms_beside_gradient_overlap(tmp_path_factory, monkeypatch):
    """With an overlap object attached, the recompute pass would run beside its all-reduce channels: both passes then take the forms without waiting
    work-groups, whatever ONEPROT_FFN2_LN says, and the ranges handed to the overlap are those of a backward without recomputation."""
    _ffn2(monkeypatch, "force")
    enc, ids, w, rng, off_force = _case(tmp_path_factory, "hd16", "force", "t512")
    tr = enc.transformer
    _ffn2(monkeypatch, "0")
    off_pair = _side(enc, [ids], [w], 0, rng)
    _ffn2(monkeypatch, "force")
    monkeypatch.setattr(tr, "GRAD_CHUNK_LAYERS", 2, raising=False)      # 6 layers: ranges end at layers 4 and 2 and at the bottom
    ranges = {}
    spy = _Spy(tr)
    try:
        for k in (0, 2):
            stub = tr._grad_overlap = _OverlapStub()
            out = _side(enc, [ids], [w], k, rng)
            ranges[k] = stub.ranges
            if k == 0:
                assert spy.saved["forms"]["ffn2_ln"]      # no recompute pass: nothing to keep apart
                _assert_equal(out, off_force, HEAD_GRADS)
            else:
                assert spy.saved["forms"] == dict(fused_ln=False, ffn2_ln=False, outproj_ln8=False)
                assert spy.segments == [(2, 4), (0, 2)]
                _assert_equal(out, off_pair, HEAD_GRADS)
                # the wait-free forms were really taken: the fused statistics differ from the LayerNorm launch's in the last bits
                assert not torch.equal(out["grad:transformer.flat"], off_force["grad:transformer.flat"])
    finally:
        spy.remove()
        tr._grad_overlap = None
    r = ranges[2]
    assert r == ranges[0] and len(r) == 3
    assert r[0][1] == tr._total and r[-1][0] == 0
    assert all(lo < hi for lo, hi in r) and all(a[0] == b[1] for a, b in zip(r, r[1:]))      # disjoint, descending, covering [0, total)


# ------------------------------------------------------------------------------------------------------------------ 10. memory
def _peak(enc, ids, w, k):
    enc.set_activation_recompute(k)
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    (enc(ids) * w).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    enc.set_activation_recompute(None)
    return peak


def test_memory_released(tmp_path_factory):
    """12 layers, T = 2048, k = 3.  A layer's record is A = (32 d + 16 + 4 H) T bytes, a boundary record at most Bd = (6 d + 8) T.  With every layer kept the
    peak holds 12 A; with recomputation 3 A (the top segment, later one recomputed segment) and the boundary records, plus the non-saving forward's
    working buffers (18 d T shared activations, a 4 d T work copy of the stream, 4 d T scratch for the gelu' codes: 26 d T < A): the peaks differ by at
    least (12 - 3 - 1) A - 4 Bd.  Measured on the MI355X: 182.8 MB against the bound of 153.6 MB."""
    n, d, H, k = 12, 320, 20, 3
    enc = _encoder(tmp_path_factory.mktemp("esm"), "hd16x12")
    ids = BATCHES["t2048"]()
    T = ids.numel()
    assert T == 2048
    torch.manual_seed(3)
    w = torch.randn(ids.shape[0], 128, device=DEV)
    _peak(enc, ids, w, 0)                                           # first use: operand mirrors, tables and the arena-gradient buffer come to stay
    peak_off = _peak(enc, ids, w, 0)
    peak_on = _peak(enc, ids, w, k)
    A, Bd = (32 * d + 16 + 4 * H) * T, (6 * d + 8) * T
    print(f"peak off {peak_off} on {peak_on} difference {peak_off - peak_on} bound {(n - k - 1) * A - 4 * Bd} (A {A}, Bd {Bd})")
    assert peak_off - peak_on >= (n - k - 1) * A - 4 * Bd


# ------------------------------------------------------------------------------------------------------------------ 11. where nothing is recomputed
def test_no_effect_without_saved_activations(tmp_path_factory, monkeypatch):
    """under no_grad the features are the same and nothing is recomputed, in eval() the switch is ignored; the environment variable is read at call time
    and switches a training forward"""
    enc, ids, w, rng, off = _case(tmp_path_factory, "hd16", None, "t512")
    spy = _Spy(enc.transformer)
    try:
        enc.eval()
        out = _side(enc, [ids], [w], 2, rng)
        assert spy.segments == [] and "bounds" not in spy.saved
        _assert_equal(out, off, HEAD_GRADS)
        enc.train()
        monkeypatch.setenv("ONEPROT_RECOMPUTE_LAYERS", "4")
        out = _side(enc, [ids], [w], None, rng)
        assert spy.segments == [(0, 4)]
        _assert_equal(out, off, HEAD_GRADS)
        with torch.no_grad():
            assert torch.equal(enc(ids), off["features0"])
        assert spy.segments == [(0, 4)]                      # no backward, no further recompute pass
    finally:
        spy.remove()
        enc.train()
        enc.transformer._live_apps = 0                       # an application under no_grad never meets its backward; the shared encoder goes back as it came
