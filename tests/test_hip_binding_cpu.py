"""The ctypes tables derived from include/oneprot_hip.h and the keyword launchers of oneprot_amd/hip.py (no GPU, no library launch):
the awkward declarations against literals, the exact positional tuple every launcher hands to hip.call, and a header the parser cannot map."""
import ctypes
from ctypes import POINTER, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import pytest

from oneprot_amd import hip

P, I, L64, F, SZ, U64 = c_void_p, c_int, c_int64, c_float, c_size_t, c_uint64


def test_derived_signatures_of_the_awkward_declarations():
    assert len(hip._SIGS) == len(hip.exported_symbols()) >= 102
    assert hip._SIGS["oneprot_gemm_bf16_nt"] == (I, [P, P, L64, I, I, I, I, I, P, P, P, P, P, P, P, F, I, I, I, P])      # int64_t M, float q_scale, 20 in all
    assert len(hip._SIGS["oneprot_gemm_bf16_nt"][1]) == 20
    assert hip._SIGS["oneprot_attn_varlen_bwd_dropout"] == (I, [P, P, P, P, P, I, P, P, P, P, P, F, P, P, I, I, I, I, F, U64, U64, P])
    assert hip._SIGS["oneprot_alloc_uncached"] == (I, [POINTER(c_void_p), SZ])
    assert hip._SIGS["oneprot_sumsq_workspace"] == (SZ, [])
    assert hip._SIGS["oneprot_dynamic_tiles"] == (None, [P, SZ])
    assert hip._SIGS["oneprot_sched_epoch"] == (L64, [P])
    assert hip._SIGS["oneprot_layernorm_bwd"] == (I, [P, I, P, I, P, I, P, P, P, P, P, P, P, P, P, L64, I, I, P])
    assert hip._SIGS["oneprot_gemm_bf16_tn"] == (I, [P, P, L64, I, I, I, I, P, P, P, SZ, I, P])
    assert hip._SIGS["oneprot_abi_version"] == (I, [])
    assert (hip.MSA_MAX_LEN, hip.MSA_MAX_ROWS, hip.ABI_VERSION) == (1024, 128, 7)


def test_derived_pointer_letters():
    assert hip._PTR_DTYPES["oneprot_gemm_bf16_nt"] == "hhf**h*ff"
    assert hip._PTR_DTYPES["oneprot_layernorm_fwd"] == "*ffhfff"
    assert hip._PTR_DTYPES["oneprot_layernorm_bwd"] == "*f*fffffhffb"
    assert hip._PTR_DTYPES["oneprot_msa_row_context_dropout"] == "fhfhb"
    assert hip._PTR_DTYPES["oneprot_attn_dropout_keep"] == "b"                       # `keep`: one byte per element
    assert hip._PTR_DTYPES["oneprot_clip_coef"] == "fffb"                            # `sched_ws`
    assert hip._PTR_DTYPES["oneprot_sim_topk"] == "ffflb"                            # int64_t* indices
    assert hip._PTR_DTYPES["oneprot_esm_embed_packed_fwd"] == "lifffffff"            # int* cu_seqlens
    assert hip._PTR_DTYPES["oneprot_ce_fwd_bwd"] == "fff"                            # float* row_loss_ws is typed: not a byte workspace
    # the stream is no tensor slot, and every letter names a dtype the binding can check
    for name, letters in hip._PTR_DTYPES.items():
        assert set(letters) <= set("fhlib*"), name
        n_ptr = sum(a is c_void_p for a in hip._SIGS[name][1])
        assert len(letters) in (n_ptr, n_ptr - 1), name


@pytest.mark.parametrize("decl, what", [
    ("double oneprot_new_thing(const float* x, int n, void* stream);", "return type"),
    ("int oneprot_new_thing(const float* x, double alpha, void* stream);", "double alpha"),
    ("int oneprot_new_thing(const float* x, int, void* stream);", "`int`"),
    ("int oneprot_new_thing(struct thing* x, void* stream);", "struct thing"),
    ("int oneprot_new_thing(const float* x, int n) { return 0; }", "oneprot_new_thing"),
])
def test_unparseable_declaration_raises(decl, what):
    good = "int oneprot_abi_version(void);\n/* a comment; with int oneprot_not_this(int x); inside */\nsize_t oneprot_w(int d); // int oneprot_nor_this(void);\n"
    sigs, kinds, consts = hip._parse_header(good + "#define ONEPROT_SOME_MAX 12\n", "good.h")
    assert sigs == {"oneprot_abi_version": (I, []), "oneprot_w": (SZ, [I])} and kinds == {} and consts == {"SOME_MAX": 12}
    with pytest.raises(hip.HipLibraryMissing) as e:
        hip._parse_header(good + decl + "\nint oneprot_after(int n);\n", "bad.h")
    assert "bad.h" in str(e.value) and "oneprot_new_thing" in str(e.value) and what in str(e.value)


def test_missing_header_raises(monkeypatch):
    monkeypatch.setattr(hip, "HEADER_PATH", "/nonexistent/oneprot_hip.h")
    with pytest.raises(hip.HipLibraryMissing, match="/nonexistent/oneprot_hip.h"):
        hip._load_header()


# ---- the launchers: the exact positional tuple handed to hip.call, values and Python types
class _T:
    """stands for a tensor: only identity matters, except numel() of a workspace"""
    def __init__(self, name, n=0):
        self.name, self.n = name, n

    def numel(self):
        return self.n

    def __repr__(self):
        return self.name


@pytest.fixture()
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(hip, "call", lambda name, *args: rec.append((name,) + args))
    return rec


def _same(got, want):
    """equal element by element, tensors by identity, scalars by value AND type (1.0 stays a float, 0 an int: bench.py's profile records keep them apart)"""
    assert len(got) == len(want), (got, want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, _T) or w is None:
            assert g is w, (k, g, w)
        else:
            assert type(g) is type(w) and g == w, (k, g, w)


A, W, B_, O0, O1, O2, AUX, COS, SIN = (_T(n) for n in ("a", "w", "bias", "out0", "out1", "out2", "aux", "cos", "sin"))


def test_gemm_nt_tuples(calls):
    nt = "oneprot_gemm_bf16_nt"
    hip.gemm_nt(A, W, 200, 640, 64, hip.EPI_BF16, O0)                                                           # defaults only
    _same(calls[-1], (nt, A, W, 200, 640, 64, 64, 64, 0, None, O0, None, None, None, None, None, 1.0, 0, 0, 0))
    hip.gemm_nt(A, W, 512, 1920, 640, hip.EPI_QKV_ROPE, O0, bias=B_, out1=O1, out2=O2, rope=(COS, SIN, 128, 20, 32), q_scale=0.25)      # the QKV form
    _same(calls[-1], (nt, A, W, 512, 1920, 640, 640, 640, 4, B_, O0, O1, O2, None, COS, SIN, 0.25, 128, 20, 32))
    hip.gemm_nt(A, W, 512, 640, 2560, hip.EPI_BIAS_RESID, O0, bias=B_, aux=AUX)                                  # residual
    _same(calls[-1], (nt, A, W, 512, 640, 2560, 2560, 2560, 3, B_, O0, None, None, AUX, None, None, 1.0, 0, 0, 0))
    hip.gemm_nt(A, W, 512, 2560, 640, hip.EPI_BIAS_GELU, O0, bias=B_, out1=O1)                                   # GELU codes
    _same(calls[-1], (nt, A, W, 512, 2560, 640, 640, 640, 2, B_, O0, O1, None, None, None, None, 1.0, 0, 0, 0))
    hip.gemm_nt(A, W, 512, 2560, 640, hip.EPI_BIAS_GELU, O0, bias=B_, out1=None)                                 # ... the forward-only form: no second output
    _same(calls[-1], (nt, A, W, 512, 2560, 640, 640, 640, 2, B_, O0, None, None, None, None, None, 1.0, 0, 0, 0))
    hip.gemm_nt(A, W, 96, 24, 40, hip.EPI_F32, O0, lda=48, ldb=72)                                               # leading dimensions other than K
    _same(calls[-1], (nt, A, W, 96, 24, 40, 48, 72, 1, None, O0, None, None, None, None, None, 1.0, 0, 0, 0))
    hip.gemm_nt(A, W, 96, 24, 40, hip.EPI_GELU_BWD, O0, aux=AUX, lda=48)                                         # one of the two
    _same(calls[-1], (nt, A, W, 96, 24, 40, 48, 40, 5, None, O0, None, None, AUX, None, None, 1.0, 0, 0, 0))
    assert len(calls) == 7 and all(len(c) == 20 for c in calls)                                                  # one call() each; call() appends the stream
    with pytest.raises(TypeError):
        hip.gemm_nt(A, W, 96, 24, 40, hip.EPI_F32, O0, B_)                                                       # the optional operands are keyword-only


def test_gemm_tn_tuples(calls):
    tn = "oneprot_gemm_bf16_tn"
    dY, X, dW, dB, ws = _T("dY"), _T("X"), _T("dW"), _T("db"), _T("ws", 4096)
    hip.gemm_tn(dY, X, 512, 1920, 640, dW, dB, ws)
    _same(calls[-1], (tn, dY, X, 512, 1920, 640, 1920, 640, dW, dB, ws, 4096, 0))
    hip.gemm_tn(dY, X, 512, 1920, 640, dW, None, ws, accumulate=1)
    _same(calls[-1], (tn, dY, X, 512, 1920, 640, 1920, 640, dW, None, ws, 4096, 1))
    hip.gemm_tn(dY, X, 512, 8, 640, dW, None, ws, ldy=24, ldx=704)
    _same(calls[-1], (tn, dY, X, 512, 8, 640, 24, 704, dW, None, ws, 4096, 0))
    assert len(calls) == 3


def test_layernorm_fwd_tuples(calls):
    fw = "oneprot_layernorm_fwd"
    x, gam, bet, y16, y32, mean, rstd = (_T(n) for n in ("x", "gamma", "beta", "y16", "y32", "mean", "rstd"))
    hip.layernorm_fwd(x, gam, bet, 300, 640, 1e-5)                                                               # no optional output
    _same(calls[-1], (fw, x, 0, gam, bet, None, None, None, None, 300, 640, 1e-5))
    hip.layernorm_fwd(x, gam, bet, 300, 640, 1e-12, y16=y16, y32=y32, mean=mean, rstd=rstd, x_is_bf16=1)         # every one
    _same(calls[-1], (fw, x, 1, gam, bet, y16, y32, mean, rstd, 300, 640, 1e-12))
    hip.layernorm_fwd(x, gam, bet, 300, 640, 1e-5, y16=y16, mean=mean, rstd=rstd)                                # the pre-LN towers' form
    _same(calls[-1], (fw, x, 0, gam, bet, y16, None, mean, rstd, 300, 640, 1e-5))
    assert len(calls) == 3


def test_layernorm_bwd_tuples(calls):
    bw = "oneprot_layernorm_bwd"
    dy, x, gam, mean, rstd, dx, dgam, dbet, ws, wrow, add, dx16 = (_T(n) for n in ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "ws", "wrow", "add_to", "dx16"))
    hip.layernorm_bwd(dy, 0, x, gam, mean, rstd, dx, dgam, dbet, ws, 300, 640, add_to=add, dx16=dx16)            # bf16 dy, into the residual gradient
    _same(calls[-1], (bw, dy, 0, None, 0, x, 0, gam, mean, rstd, add, dx, dx16, dgam, dbet, ws, 300, 640, 0))
    hip.layernorm_bwd(dy, 1, x, gam, mean, rstd, dx, dgam, dbet, ws, 300, 640, add_to=add, dx16=dx16, accumulate=1, x_is_bf16=1)
    _same(calls[-1], (bw, dy, 1, None, 0, x, 1, gam, mean, rstd, add, dx, dx16, dgam, dbet, ws, 300, 640, 1))
    hip.layernorm_bwd(dy, 2, x, gam, mean, rstd, dx, dgam, dbet, ws, 300, 640, wrow=wrow, L=75, add_to=add, dx16=dx16)      # dy = dpooled * wrow
    _same(calls[-1], (bw, dy, 2, wrow, 75, x, 0, gam, mean, rstd, add, dx, dx16, dgam, dbet, ws, 300, 640, 0))
    hip.layernorm_bwd(dy, 1, x, gam, mean, rstd, dx, dgam, dbet, ws, 300, 640)                                   # nothing optional
    _same(calls[-1], (bw, dy, 1, None, 0, x, 0, gam, mean, rstd, None, dx, None, dgam, dbet, ws, 300, 640, 0))
    assert len(calls) == 4 and all(len(c) == 19 for c in calls)


def test_product_call_sites_use_the_launchers():
    """no product module spells out the positional form of the four wide entry points any more (tests, tools and bench.py may)"""
    import os
    import re
    pkg = os.path.dirname(hip.__file__)
    for mod in ("esm.py", "bert.py", "msa.py", "layout.py", "encoders.py"):
        src = open(os.path.join(pkg, mod)).read()
        assert not re.search(r'"oneprot_(gemm_bf16_nt|gemm_bf16_tn|layernorm_fwd|layernorm_bwd)"', src), mod
