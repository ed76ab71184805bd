"""ctypes binding of liboneprot_hip.so (the C ABI in include/oneprot_hip.h).

There is no CPU fallback: if the shared library is missing, or a kernel returns a non-zero status, this module
raises.  torch is used only as the owner of device memory and streams (tensor.data_ptr(), current stream).

The header is the single source of the ABI: the ctypes signatures (_SIGS) and the expected element type of every pointer argument (_PTR_DTYPES) are
parsed from it at import, so a new entry point is declared there, defined in csrc/, and needs nothing here unless one of its void* is not bf16
(_BYTE_PTRS / _FLAG_TYPED_PTRS).  call(name, *positional) launches any entry point; gemm_nt / gemm_tn / layernorm_fwd / layernorm_bwd / gemm_tn_ln_bwd are keyword
launchers of the widest ones and end in the same call().  sort_f32 / sort_i32 / midranks_f32 / inclusive_scan / moments / f1max are the launchers of the
downstream-metric entry points (csrc/metrics.hip): they size and allocate the workspace, and hand back device tensors (fp64 results as views of byte buffers).
probe_linear_fwd / probe_rownorm_act_fwd / probe_norm_act_bwd / probe_rownorm_act_bwd / probe_loss are the keyword launchers of the MLP probe's wide entry points
(csrc/probe.hip).  The gradient-boosted tree entry points (csrc/gbt.hip, oneprot_gbt_*) are called by name from oneprot_amd/gbt.py and oneprot_amd/gbt_deep.py, the text-input entry
point (csrc/wordpiece.hip, oneprot_wordpiece_encode) from oneprot_amd/text_data.py, the graph-input entry point (csrc/graph_feats.hip,
oneprot_graph_featurize) from oneprot_amd/graph_data.py.
"""
import ctypes
import os
import re
from ctypes import c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ONEPROT_HIP_LIB: another build of the same ABI (development: step-level A/B of a variant library, tools/ab/build_lib.sh)
LIB_PATH = os.environ.get("ONEPROT_HIP_LIB") or os.path.join(_HERE, "liboneprot_hip.so")

ABI_VERSION = 7
EPI_BF16, EPI_F32, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_QKV_ROPE, EPI_GELU_BWD = range(6)
LOG2E = 1.4426950408889634      # the attention kernels take q pre-multiplied by hd^-1/2 * log2(e) (include/oneprot_hip.h)


class HipLibraryMissing(RuntimeError):
    pass


class HipKernelError(RuntimeError):
    pass


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "oneprot_hip.h")      # where csrc/build.sh reads it too

_SCALARS = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "float": c_float, "uint64_t": c_uint64}
_RETURNS = {"int": c_int, "size_t": c_size_t, "int64_t": c_int64, "void": None}
# Element type of a pointer argument: f = float32, h = bfloat16, l = int64, i = int32, b = uint8 workspace, * = stated by a flag argument / epilogue id.
# A typed pointer says it itself and a void* is bf16 storage (the header's convention).  The void* that are not bf16 are named here, and nowhere else:
_PTR_LETTER = {"float": "f", "int64_t": "l", "int": "i", "void": "h"}
_BYTE_PTRS = {"workspace", "sched_ws", "keep", "msa_bytes", "moments_bytes", "f1_bytes", "loss_bytes", "bins", "row_keep", "feat_keep", "gain_bytes", "text_bytes", "res_type_bytes"}      # by parameter name, in every entry point (fp64 results travel as bytes)
_FLAG_TYPED_PTRS = {("oneprot_gemm_bf16_nt", "out0"), ("oneprot_gemm_bf16_nt", "out1"), ("oneprot_gemm_bf16_nt", "aux"),
                    ("oneprot_layernorm_fwd", "x"), ("oneprot_layernorm_bwd", "dy"), ("oneprot_layernorm_bwd", "x"),
                    ("oneprot_inclusive_scan", "x"), ("oneprot_inclusive_scan", "y"), ("oneprot_moments", "a"), ("oneprot_moments", "b"), ("oneprot_f1max", "target")}


def _parse_header(text, where=HEADER_PATH):
    """({entry point: (restype, [argtypes])}, {entry point: pointer letters, the trailing stream excluded}, {ONEPROT_<NAME>: int of a #define})
    of the C declarations in `text`.  A declaration it cannot map raises HipLibraryMissing: nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+ONEPROT_(\w+)\s+(\d+)\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    sigs, kinds = {}, {}
    for m in re.finditer(r"([^;{}]*?)\b(oneprot_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        decl = " ".join(m.group(0).split())
        if ret not in _RETURNS:
            raise HipLibraryMissing(f"{where}: cannot map the return type of `{decl}`")
        args, letters = [], ""
        plist = [] if params == "void" else params.split(",")
        for k, prm in enumerate(plist):
            pm = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*", prm)
            ctype, stars, pname = pm.groups() if pm else (None, "", None)
            if stars == "" and ctype in _SCALARS:
                args.append(_SCALARS[ctype])
            elif stars == "**" and ctype == "void":
                args.append(ctypes.POINTER(c_void_p))
            elif stars == "*" and ctype in _PTR_LETTER:
                args.append(c_void_p)
                if not (pname == "stream" and k == len(plist) - 1):
                    letters += "b" if pname in _BYTE_PTRS else "*" if (name, pname) in _FLAG_TYPED_PTRS else _PTR_LETTER[ctype]
            else:
                raise HipLibraryMissing(f"{where}: cannot map parameter `{prm.strip()}` of `{decl}`")
        sigs[name] = (_RETURNS[ret], args)
        if letters:
            kinds[name] = letters
    unparsed = sorted(set(re.findall(r"\b(oneprot_\w+)\s*\(", text)) - set(sigs))
    if unparsed:
        raise HipLibraryMissing(f"{where}: cannot parse the declaration of {', '.join(unparsed)}")
    return sigs, kinds, consts


def _load_header():
    try:
        with open(HEADER_PATH) as f:
            return _parse_header(f.read())
    except OSError as e:
        raise HipLibraryMissing(f"{HEADER_PATH}: the C header the binding is derived from cannot be read ({e})") from None


# name -> (restype, argtypes) and name -> pointer letters, both derived from include/oneprot_hip.h.  The C side validates shapes and alignment but cannot
# see a tensor's dtype, device or strides: a strided view or an fp16 tensor would compute garbage silently, so the binding refuses them (HipKernelError)
# before the launch.
_SIGS, _PTR_DTYPES, _consts = _load_header()
MSA_MAX_LEN, MSA_MAX_ROWS = _consts["MSA_MAX_LEN"], _consts["MSA_MAX_ROWS"]
SORT_TILE, SCAN_TILE = _consts["SORT_TILE"], _consts["SCAN_TILE"]      # keys per work-group of a radix pass / elements per chunk of the scan tree (csrc/metrics.hip)
PROBE_MAX_BATCH = _consts["PROBE_MAX_BATCH"]                            # rows of a BatchNorm (train mode) batch of the MLP probe (csrc/probe.hip)
_DT = {"f": torch.float32, "h": torch.bfloat16, "l": torch.int64, "i": torch.int32, "b": torch.uint8}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    """Load (once) and return the ctypes handle.  Raises HipLibraryMissing if the .so was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(oneprot_amd/csrc/build.sh).  There is no CPU fallback for the OneProt hot path.")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(h, name)          # AttributeError here = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        if h.oneprot_abi_version() != ABI_VERSION:
            raise HipLibraryMissing(f"{LIB_PATH} has ABI version {h.oneprot_abi_version()}, this binding needs {ABI_VERSION}: rebuild it (oneprot_amd/csrc/build.sh)")
        _lib = h
    return _lib


def ptr(t):
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _check_tensors(name, args):
    """device / layout / dtype of every tensor handed to `name` (see _PTR_DTYPES)"""
    kinds = _PTR_DTYPES.get(name)
    slot = 0
    for a in args:
        if not (a is None or isinstance(a, torch.Tensor)):
            continue
        if a is not None:
            if not a.is_cuda:
                raise HipKernelError(f"{name}: pointer argument {slot} is a {a.device} tensor; the HIP path has no CPU fallback")
            if not a.is_contiguous():
                raise HipKernelError(f"{name}: pointer argument {slot} is not contiguous (shape {tuple(a.shape)}, strides {a.stride()}); the kernels take dense row-major memory")
            if kinds is not None and slot < len(kinds) and kinds[slot] != "*" and a.dtype != _DT[kinds[slot]]:
                raise HipKernelError(f"{name}: pointer argument {slot} has dtype {a.dtype}, the entry point takes {_DT[kinds[slot]]}")
        slot += 1


def stream():
    return torch.cuda.current_stream().cuda_stream


_prof = None     # {entry point: (epilogue or None, [(start_event, end_event, scalar args), ...])}


def profile_begin(name, epilogue=None):
    """Bracket every subsequent launch of `name` (optionally: only with this GEMM epilogue id) with HIP events recorded on the
    launch stream; profile_end() returns the per-launch durations in ms.  Used by bench.py for the live roofline figure.
    `name` may be a dict {entry point: epilogue or None} to watch several entry points at once (profile_end then returns a dict of
    [(ms, scalar args), ...] lists)."""
    global _prof
    _prof = {k: (v, []) for k, v in name.items()} if isinstance(name, dict) else {name: (epilogue, [])}
    _prof["__single__"] = None if isinstance(name, dict) else name


def profile_end():
    global _prof
    if _prof is None:
        return []
    torch.cuda.synchronize()
    single = _prof.pop("__single__")
    out = {k: [(a.elapsed_time(b), sc) for a, b, sc in v[1]] for k, v in _prof.items()}
    _prof = None
    return [ms for ms, _ in out[single]] if single is not None else out


def call(name, *args):
    """Invoke an int-returning entry point on the current torch stream; raise on a non-zero status."""
    fn = getattr(lib(), name)
    _check_tensors(name, args)
    cargs = [ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
    watch = _prof.get(name) if _prof is not None else None
    if watch is not None and (watch[0] is None or args[7] == watch[0]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*cargs, stream())
        e1.record()
        # scalar arguments + the number of tensor arguments (tells e.g. a GEMM launch with the optional second output from one without)
        watch[1].append((e0, e1, tuple(a for a in args if isinstance(a, (int, float))) + (sum(isinstance(a, torch.Tensor) for a in args),)))
    else:
        rc = fn(*cargs, stream())
    if rc != 0:
        raise HipKernelError(f"{name} returned {rc} ({'invalid argument' if rc == -1 else 'launch failure'})")


def query(name, *args):
    return getattr(lib(), name)(*args)


# ---------------------------------------------------------------------------------------------------------------------------------
# Keyword launchers of the four widest entry points.  Each only orders its arguments as include/oneprot_hip.h declares them and hands them to call().
def gemm_nt(a, w, M, N, K, epi, out0, *, bias=None, out1=None, out2=None, aux=None, lda=None, ldb=None, rope=None, q_scale=1.0):
    """out0 (, out1, out2) = epilogue `epi` of a[M,K] w[N,K]^T.  lda / ldb default to K; rope = (cos, sin, L, H, hd) for EPI_QKV_ROPE."""
    cos, sin, L, H, hd = rope if rope is not None else (None, None, 0, 0, 0)
    call("oneprot_gemm_bf16_nt", a, w, M, N, K, K if lda is None else lda, K if ldb is None else ldb, epi, bias, out0, out1, out2, aux, cos, sin, q_scale, L, H, hd)


def gemm_tn(dY, X, M, N, K, dW, dbias, ws, *, ldy=None, ldx=None, accumulate=0):
    """dW[N,K] (+)= dY[M,N]^T X[M,K], dbias[N] (+)= column sums of dY (optional).  ldy defaults to N, ldx to K; ws from oneprot_gemm_bf16_tn_workspace."""
    call("oneprot_gemm_bf16_tn", dY, X, M, N, K, N if ldy is None else ldy, K if ldx is None else ldx, dW, dbias, ws, ws.numel(), accumulate)


def layernorm_fwd(x, gamma, beta, T, d, eps, *, y16=None, y32=None, mean=None, rstd=None, x_is_bf16=0):
    call("oneprot_layernorm_fwd", x, x_is_bf16, gamma, beta, y16, y32, mean, rstd, T, d, eps)


def layernorm_bwd(dy, dy_mode, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, T, d, *, wrow=None, L=0, x_is_bf16=0, add_to=None, dx16=None, accumulate=0):
    """dy_mode 0: dy bf16 [T,d]; 1: fp32 [T,d]; 2: dy[t] = dy[t // L] * wrow[t].  dx = (add_to or 0) + LN'(dy), dx16 its optional bf16 copy."""
    call("oneprot_layernorm_bwd", dy, dy_mode, wrow, L, x, x_is_bf16, gamma, mean, rstd, add_to, dx, dx16, dgamma, dbeta, ws, T, d, accumulate)


def gemm_tn_ln_bwd(dY, X, M, N, K, dW, dbias, ws, dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws_ln, ln_cus, *, add_to=None, dx16=None):
    """gemm_tn(dY, X) and layernorm_bwd(dy bf16, x fp32) on the same M rows of width K in one launch, `ln_cus` CUs given to the LayerNorm rows; ws_ln: the
    bytes of oneprot_layernorm_bwd_workspace(K)"""
    call("oneprot_gemm_tn_ln_bwd", dY, X, M, N, K, N, K, dW, dbias, ws, ws.numel(), 0, dy, x, gamma, mean, rstd, add_to, dx, dx16, dgamma, dbeta, ws_ln.view(torch.float32), 0,
         ln_cus)


# CUs of the LayerNorm role of oneprot_gemm_tn_ln_bwd by the weight gradient's N at K = 640: the fastest fused launch of tools/ab/wgrad_ln_ab.py
# (profiles/wgrad_ln_ab.txt: FFN-1 554 us at 64 against 656 for the two launches, QKV 470 us at 80 against 562); other shapes: 64
WGRAD_LN_CUS = {2560: 64, 1920: 80}


def wgrad_ln_wanted():
    """ONEPROT_WGRAD_LN=1 / 0: the FFN-1 and QKV weight gradients of a trainable ESM layer in one launch with the LayerNorm backward that follows their data
    gradient (single rank, no CU reserve).  Default: on (4.9 ms of the cfg-2 step); 0 keeps the separate launches (A/B runs, tests)."""
    return os.environ.get("ONEPROT_WGRAD_LN", "1") != "0"


def wgrad_ln_cus(N):
    """ONEPROT_WGRAD_LN_CUS=<n> (A/B runs), else the measured choice for this weight gradient"""
    v = os.environ.get("ONEPROT_WGRAD_LN_CUS")
    return int(v) if v else WGRAD_LN_CUS.get(N, 64)


def _workspace(query_name, like, *shape):
    nbytes = query(query_name, *shape)
    if nbytes == 0:
        raise HipKernelError(f"{query_name}{shape} returned 0: invalid size")
    return torch.empty(nbytes, dtype=torch.uint8, device=like.device)


# The downstream-metric entry points (csrc/metrics.hip).  Each allocates the workspace its query asks for on the tensor's device and returns device tensors;
# fp64 results come back as float64 views of the byte buffers the entry points write.
def sort_f32(keys, *, descending=False, want_keys=False):
    """(perm int32 [n], sorted keys fp32 [n] or None): the stable argsort of a flat fp32 device tensor; equal keys in ascending index in both directions"""
    n = keys.numel()
    perm = torch.empty(n, dtype=torch.int32, device=keys.device)
    out = torch.empty(n, dtype=torch.float32, device=keys.device) if want_keys else None
    ws = _workspace("oneprot_sort_workspace", keys, n)
    call("oneprot_sort_f32", keys, n, int(bool(descending)), perm, out, ws, ws.numel())
    return perm, out


def sort_i32(keys, key_bits, *, values=None, want_keys=True):
    """(sorted keys int32 [n] or None, values int32 [n]): the stable sort of int32 keys in [0, 2^key_bits); values None sorts 0 .. n-1 along (an argsort)"""
    n = keys.numel()
    vout = torch.empty(n, dtype=torch.int32, device=keys.device)
    kout = torch.empty(n, dtype=torch.int32, device=keys.device) if want_keys else None
    ws = _workspace("oneprot_sort_workspace", keys, n)
    call("oneprot_sort_i32", keys, values, n, int(key_bits), kout, vout, ws, ws.numel())
    return kout, vout


def midranks_f32(x):
    """rank2 int32 [n]: twice the average 1-based rank of every element of a flat fp32 device tensor"""
    n = x.numel()
    rank2 = torch.empty(n, dtype=torch.int32, device=x.device)
    ws = _workspace("oneprot_midranks_workspace", x, n)
    call("oneprot_midranks_f32", x, n, rank2, ws, ws.numel())
    return rank2


def inclusive_scan(x, *, seg_len=0):
    """the ordered inclusive scan of a flat int32 or float64 device tensor, restarting at every multiple of seg_len (0: one flat scan)"""
    if x.dtype not in (torch.int32, torch.float64):
        raise HipKernelError(f"oneprot_inclusive_scan: dtype {x.dtype}; the entry point takes int32 or float64")
    n = x.numel()
    y = torch.empty_like(x)
    ws = _workspace("oneprot_scan_workspace", x, n)
    call("oneprot_inclusive_scan", x, y, n, int(seg_len), int(x.dtype == torch.float64), ws, ws.numel())
    return y


def moments(a, b, *, shift_a=0.0, shift_b=0.0):
    """float64 [8] on the device: n, sum a', sum b', sum a'^2, sum b'^2, sum a'b', sum (a'-b')^2, #(a == b) of two fp32 or two int32 streams, a' = a - shift_a"""
    if a.dtype != b.dtype or a.dtype not in (torch.int32, torch.float32) or a.numel() != b.numel():
        raise HipKernelError(f"oneprot_moments: streams of {a.dtype} [{a.numel()}] and {b.dtype} [{b.numel()}]; two fp32 or two int32 streams of one length are taken")
    n = a.numel()
    out = torch.empty(64, dtype=torch.uint8, device=a.device)
    ws = _workspace("oneprot_moments_workspace", a, n)
    call("oneprot_moments", a, b, n, int(a.dtype == torch.int32), float(shift_a), float(shift_b), out, ws, ws.numel())
    return out.view(torch.float64)


def f1max(pred, target):
    """float64 [2] on the device: (F1-max, the score at which it is reached) of pred fp32 [B, N] and target int32 or fp32 [B, N]"""
    if target.dtype not in (torch.int32, torch.float32) or target.shape != pred.shape or pred.dim() != 2:
        raise HipKernelError(f"oneprot_f1max: pred {tuple(pred.shape)}, target {target.dtype} {tuple(target.shape)}; fp32 [B, N] and int32 or fp32 [B, N] are taken")
    B, N = pred.shape
    out = torch.empty(16, dtype=torch.uint8, device=pred.device)
    ws = _workspace("oneprot_f1max_workspace", pred, B, N)
    call("oneprot_f1max", pred, target, int(target.dtype == torch.float32), B, N, out, ws, ws.numel())
    return out.view(torch.float64)


# The MLP probe (csrc/probe.hip).  norm / act ids as include/oneprot_hip.h numbers them; rng = (p, seed, stream_id) of the dropout, None for no dropout.
PROBE_NORM_NONE, PROBE_NORM_BN_TRAIN, PROBE_NORM_BN_EVAL = range(3)
PROBE_ACT = {"identity": 0, "relu": 1, "gelu": 2, "leaky_relu": 3}
PROBE_LOSS_BCE, PROBE_LOSS_MSE, PROBE_LOSS_CE = range(3)


def _rng3(rng):
    p, seed, stream_id = rng if rng is not None else (0.0, 0, 0)
    return float(p), int(seed), int(stream_id)


def probe_linear_fwd(x, w, b, M, n, k, *, idx=None, z=None, y=None, resid=None, resid_idx=None, norm=0, act=0, gamma=None, beta=None, mean=None, rstd=None,
                     running_mean=None, running_var=None, rng=None):
    """z = gather(x, idx) w^T + b (pre-norm, optional), y = dropout(act(norm(z))) (+ resid) (optional)"""
    call("oneprot_probe_linear_fwd", x, idx, w, b, z, y, resid, resid_idx, gamma, beta, mean, rstd, running_mean, running_var, M, n, k, int(norm), int(act),
         *_rng3(rng))


def probe_rownorm_act_fwd(z, gamma, beta, y, M, n, *, act=0, resid=None, resid_idx=None, mean=None, rstd=None, rng=None):
    """y = dropout(act(LayerNorm(z))) (+ resid)"""
    call("oneprot_probe_rownorm_act_fwd", z, gamma, beta, y, resid, resid_idx, mean, rstd, M, n, int(act), *_rng3(rng))


def probe_norm_act_bwd(dy, z, dz, M, n, *, norm=0, act=0, gamma=None, beta=None, mean=None, rstd=None, dgamma=None, dbeta=None, rng=None):
    """dz of y = dropout(act(norm(z))); norm 2 takes the running mean and the running variance as mean / rstd"""
    call("oneprot_probe_norm_act_bwd", dy, z, gamma, beta, mean, rstd, dz, dgamma, dbeta, M, n, int(norm), int(act), *_rng3(rng))


def probe_rownorm_act_bwd(dy, z, gamma, beta, mean, rstd, dz, M, n, *, act=0, dgamma=None, dbeta=None, rng=None):
    call("oneprot_probe_rownorm_act_bwd", dy, z, gamma, beta, mean, rstd, dz, dgamma, dbeta, M, n, int(act), *_rng3(rng))


def probe_loss(logits, M, C, kind, loss_sum, ws, *, target=None, labels=None, idx=None, dlogits=None, weight=1.0):
    """loss_sum (a float64 [1] device tensor) += weight x mean loss; dlogits (optional) = its gradient.  ws from probe_loss_workspace()."""
    call("oneprot_probe_loss_fwd_bwd", logits, target, labels, idx, dlogits, loss_sum.view(torch.uint8), ws, M, C, int(kind), float(weight))


def probe_loss_workspace(device):
    return torch.empty(query("oneprot_probe_loss_workspace"), dtype=torch.uint8, device=device)


# ---------------------------------------------------------------------------------------------------------------------------------
# The sched workspace (include/oneprot_hip.h, csrc/sched_ws.h): per-device memory through which the persistent kernels hand out work and keep their launch
# bookkeeping on the device.  The host side owns it: one uncached allocation per device, zeroed once, grown when a launch needs more rows.
class _SchedWorkspace:
    def __init__(self, device, rows):
        h = lib()
        self.device, self.rows = device, rows
        self.bytes = h.oneprot_sched_workspace_bytes(rows)
        out = c_void_p()
        with torch.cuda.device(device):
            if h.oneprot_alloc_uncached(ctypes.byref(out), self.bytes) != 0 or not out.value:
                raise HipKernelError(f"oneprot_alloc_uncached({self.bytes} bytes) failed")
            self.ptr = out.value
            if h.oneprot_sched_workspace_init(self.ptr, self.bytes, stream()) != 0:
                raise HipKernelError("oneprot_sched_workspace_init failed")

    def error(self):
        return lib().oneprot_gemm_resid_ln8_error(self.ptr)

    def release(self):
        if self.ptr:
            torch.cuda.synchronize(self.device)
            lib().oneprot_free_uncached(self.ptr)
            self.ptr = 0


_sched = {}      # device index -> _SchedWorkspace
SCHED_MIN_ROWS = 131072


def dynamic_tiles_wanted():
    """ONEPROT_DYNAMIC_TILES=1 / 0; default: on when this process is one of several ranks (WORLD_SIZE > 1), off otherwise.  On = the tiles of the persistent NT GEMMs
    and the slabs of the attention forward are drawn from work queues: a co-resident kernel that holds CUs -- an RCCL channel of the overlapped gradient
    all-reduce -- then costs its share of the chip instead of 1.47 x per launch (profiles/r06_cu_occupier.txt); bit-identical results either way, a tie in
    time on a GPU that runs nothing else."""
    v = os.environ.get("ONEPROT_DYNAMIC_TILES")
    if v is not None:
        return v != "0"
    return int(os.environ.get("WORLD_SIZE", "1")) > 1


def cu_reserve_wanted():
    """ONEPROT_CU_RESERVE=<n>; default 16 when this process is one of several ranks (the overlapped gradient all-reduce's RCCL channels hold CUs), else 0"""
    v = os.environ.get("ONEPROT_CU_RESERVE")
    if v is not None:
        return int(v)
    return 16 if int(os.environ.get("WORLD_SIZE", "1")) > 1 else 0


def sched_workspace(rows=0, device=None):
    """(pointer, bytes) of the current device's sched workspace, sized for at least `rows` rows of row statistics"""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    ws = _sched.get(dev)
    if ws is None or ws.rows < rows:
        new_rows = max(rows, SCHED_MIN_ROWS, 2 * ws.rows if ws is not None else 0)
        if ws is not None:
            if ws.error() != 0:
                raise HipKernelError("oneprot_gemm_bf16_nt_resid_ln8: a bounded wait ran out in an earlier launch (NaN rows were written)")
            lib().oneprot_dynamic_tiles(None, 0)
            ws.release()
        ws = _sched[dev] = _SchedWorkspace(dev, new_rows)
        lib().oneprot_dynamic_tiles(ws.ptr if dynamic_tiles_wanted() else None, ws.bytes)
        lib().oneprot_cu_reserve(cu_reserve_wanted())
    return ws.ptr, ws.bytes


def _sched_of(device):
    if not _sched:                                       # nothing has launched through a workspace yet (also: no GPU in this process)
        return None
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    return _sched.get(dev)


def sched_error(device=None):
    """host-synchronous: 1 when a launch on this device's workspace wrote NaN rows because a bounded wait ran out (0 when no workspace exists yet)"""
    ws = _sched_of(device)
    return 0 if ws is None else ws.error()


def sched_late_draws(device=None):
    ws = _sched_of(device)
    return 0 if ws is None else lib().oneprot_sched_late_draws(ws.ptr)


def sched_error_clear(device=None):
    ws = _sched_of(device)
    if ws is not None:
        lib().oneprot_gemm_resid_ln8_error_clear(ws.ptr, stream())


def sched_ptr_or_none(device=None):
    ws = _sched_of(device)
    return None if ws is None else ws.ptr
