"""Retrieval at database scale: ranks of the matching pairs and top-k search without the N x N similarity matrix (replaces ref
src/models/components/retrieval_metric.py:83-102 beyond the size at which the matrix fits, and ref src/eval.py:158-184 `calculate_retrieval_metrics`).

The kernels (csrc/retrieval.hip) form each similarity tile with the fp32-input MFMA and consume it in registers.  Every similarity is the k-ordered fp32
fmaf chain that `oneprot_sgemm` computes, so `pair_ranks` returns the ranks of `oneprot_sgemm` + `oneprot_diag_rank` bit for bit.

Tie rules, both paths:
  * ranks count strict `>`: rank[i] is the number of candidates whose similarity is strictly greater than the matching pair's.  A candidate that ties with
    the matching pair does not push it down -- the optimistic rank, as `oneprot_diag_rank` counts it.  `pair_ranks(..., ties=True)` returns, next to it, how
    many other candidates tie with the matching pair exactly (same tile values, `==`); rank + ties is the pessimistic rank (`bound="pessimistic"`).
  * top-k orders by descending score and breaks ties by ascending database index, so the result is fully defined.

Inputs are fp32 device tensors [rows, D]; CPU tensors raise HipKernelError (there is no fallback).  Scores are expected to be finite."""
import numpy as np
import torch

from . import hip

# one launch of oneprot_sim_rank is kept below this many multiply-adds (a few tenths of a second on an MI355X), so that no single kernel runs for long
_SLAB_FMAS = 2e13


def _features(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: a [rows, D] tensor is expected")
    if not x.is_cuda:
        raise hip.HipKernelError(f"{what} is a {x.device} tensor; the HIP path has no CPU fallback")
    return x.detach().float().contiguous()


def default_slab_rows(N, D):
    rows = int(_SLAB_FMAS / (float(N) * float(D)))
    return max(128, min(N, rows // 128 * 128))


def pair_ranks(s, m, slab_rows=None, ties=False):
    """(rank_row, rank_col), int32 [N] on the device: rank_row[i] = #{j : s_i . m_j > s_i . m_i} (s -> m retrieval), rank_col[j] = #{i : s_i . m_j > s_j . m_j}
    (m -> s).  `slab_rows` rows of s per launch (default: sized by work); the result does not depend on it.  ties=True: (rank_row, rank_col, tie_row, tie_col),
    tie_row[i] = #{j != i : s_i . m_j == s_i . m_i} and tie_col likewise, counted by oneprot_sim_rank_ties on the very tile values the ranks are counted on."""
    s, m = _features(s, "pair_ranks: s"), _features(m, "pair_ranks: m")
    if s.shape != m.shape:
        raise ValueError(f"pair_ranks: s {tuple(s.shape)} and m {tuple(m.shape)} must have the same shape")
    N, D = s.shape
    step = default_slab_rows(N, D) if slab_rows is None else int(slab_rows)
    if step < 1:
        raise ValueError("pair_ranks: slab_rows must be >= 1")
    diag = torch.empty(N, device=s.device)
    hip.call("oneprot_sim_pair_dot", s, m, diag, N, D)
    rr = torch.zeros(N, dtype=torch.int32, device=s.device)
    rc = torch.zeros(N, dtype=torch.int32, device=s.device)
    if not ties:
        for row0 in range(0, N, step):
            hip.call("oneprot_sim_rank", s, m, diag, N, D, row0, min(step, N - row0), rr, rc)
        return rr, rc
    tr, tc = torch.zeros_like(rr), torch.zeros_like(rc)
    for row0 in range(0, N, step):
        hip.call("oneprot_sim_rank_ties", s, m, diag, N, D, row0, min(step, N - row0), rr, rc, tr, tc)
    return rr, rc, tr, tc


def topk(queries, database, k):
    """(scores fp32 [nq, k] descending, indices int64 [nq, k]): the k database rows with the largest dot product per query; equal scores in ascending index."""
    q, db = _features(queries, "topk: queries"), _features(database, "topk: database")
    if q.shape[1] != db.shape[1]:
        raise ValueError(f"topk: queries have {q.shape[1]} features, the database {db.shape[1]}")
    nq, D = q.shape
    N, k = db.shape[0], int(k)
    if not 1 <= k <= min(N, 256):
        raise ValueError(f"topk: k = {k} outside 1 .. min(N, 256) = {min(N, 256)}")
    nbytes = hip.query("oneprot_sim_topk_workspace", nq, N, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    scores = torch.empty(nq, k, device=q.device)
    indices = torch.empty(nq, k, dtype=torch.int64, device=q.device)
    hip.call("oneprot_sim_topk", q, db, nq, N, D, k, scores, indices, ws, nbytes)
    return scores, indices


BOUNDS = ("optimistic", "pessimistic")


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def metrics_from_ranks(rank_row, rank_col, ks, ties=None, bound="optimistic"):
    """the dict of ref retrieval_metric.py:95-102 from the two rank vectors: floor(median) + 1 and R@k = mean(rank < k), both directions.  bound
    "pessimistic" takes rank + ties (ties = (tie_row, tie_col) of pair_ranks(..., ties=True)): every candidate that ties with the matching pair is ahead of it."""
    if bound not in BOUNDS:
        raise ValueError(f"metrics_from_ranks: bound {bound!r}; one of {', '.join(BOUNDS)}")
    if bound == "pessimistic" and ties is None:
        raise ValueError("metrics_from_ranks: the pessimistic bound needs ties = (tie_row, tie_col)")
    out = {}
    for d, (name, ranks) in enumerate((("seq_to_mod", rank_row), ("mod_to_seq", rank_col))):
        r = _host(ranks)
        if bound == "pessimistic":
            r = r.astype(np.int64) + _host(ties[d])
        out[f"{name}_median_rank"] = float(np.floor(np.median(r)) + 1)
        for k in ks:
            out[f"{name}_R@{k}"] = float(np.mean(r < k))
    return out


def retrieval_table(embeddings, ks=(1, 10, 100, 500), normalize=False, slab_rows=None, bound="optimistic", tie_rows=None):
    """ref eval.py:158-184 `calculate_retrieval_metrics`: {f"{mod1}-{mod2}": metrics} for every unordered pair of modalities, in insertion order.  The
    embeddings are the encoders' outputs (already L2-normalised); normalize=True runs them through oneprot_l2norm_fwd first.  bound "pessimistic": ranks
    + tie counts (oneprot_sim_rank_ties).  tie_rows: a dict that receives {pair: (rows with a tie s -> m, rows with a tie m -> s)}; asking for it, like the
    pessimistic bound, runs the tie-counting kernel, whose ranks are those of the plain one."""
    if bound not in BOUNDS:
        raise ValueError(f"retrieval_table: bound {bound!r}; one of {', '.join(BOUNDS)}")
    feats = {}
    for name, x in embeddings.items():
        x = _features(x, f"retrieval_table: {name}")
        if normalize:
            y, inv = torch.empty_like(x), torch.empty(x.shape[0], device=x.device)
            hip.call("oneprot_l2norm_fwd", x, y, inv, x.shape[0], x.shape[1], 1.0)
            x = y
        feats[name] = x
    names = list(feats)
    want_ties = bound == "pessimistic" or tie_rows is not None
    table = {}
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            pair = f"{names[a]}-{names[b]}"
            if not want_ties:
                rr, rc = pair_ranks(feats[names[a]], feats[names[b]], slab_rows=slab_rows)
                table[pair] = metrics_from_ranks(rr, rc, ks)
                continue
            rr, rc, tr, tc = pair_ranks(feats[names[a]], feats[names[b]], slab_rows=slab_rows, ties=True)
            tr, tc = _host(tr), _host(tc)
            table[pair] = metrics_from_ranks(rr, rc, ks, ties=(tr, tc), bound=bound)
            if tie_rows is not None:
                tie_rows[pair] = (int((tr > 0).sum()), int((tc > 0).sum()))
    return table
