"""Streaming retrieval (oneprot_amd/retrieval.py, csrc/retrieval.hip) on the MI355X: ranks and top-k without the N x N matrix.

Everything here is an equality.  On grid inputs (small integers stored as fp32) every dot product is exact in fp32 in any summation order, so numpy int64
gives the expected ranks and top-k lists, ties included.  On random features the similarity must be the k-ordered fmaf chain of `oneprot_sgemm`, so ranks
and scores are compared bit for bit with the matrix path (`oneprot_sgemm` + `oneprot_diag_rank`): a mismatch means another summation order.
Shapes: below one 128 x 128 tile, one past a tile / a 32-deep K slice, D odd and D = 1, slab edges inside a tile, k = 1 / N / 256, database-split edges."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip, retrieval  # noqa: E402
from oneprot_amd.metrics import RetrievalMetric  # noqa: E402
from oracle import oneprot_oracle as O  # noqa: E402

DEV = "cuda"


def _grid(rows, D, lim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, (rows, D), generator=g).float()


def _expected_ranks(s, m):
    sim = s.numpy().astype(np.int64) @ m.numpy().astype(np.int64).T
    d = np.diag(sim)
    return (sim > d[:, None]).sum(1), (sim > d[None, :]).sum(0)


_grid_cache = {}


def _grid_case(N, D):
    if (N, D) not in _grid_cache:
        s, m = _grid(N, D, 8, 100 + N), _grid(N, D, 8, 200 + N)
        m[: N // 3] = s[: N // 3]                       # a third of the pairs are near the top, like trained towers; the rest are anywhere
        m[N - 1] = m[N - 2]                             # two equal candidates: rows N-2 and N-1 each see an entry equal to their diagonal
        er, ec = _expected_ranks(s, m)
        sim = s.numpy().astype(np.int64) @ m.numpy().astype(np.int64).T
        ties = int((sim == np.diag(sim)[:, None]).sum()) - N
        _grid_cache[(N, D)] = (s, m, torch.from_numpy(er).int(), torch.from_numpy(ec).int(), ties)
    return _grid_cache[(N, D)]


@pytest.mark.parametrize("N,D", [(5, 1), (64, 16), (257, 37), (1000, 100), (2049, 129)])
def test_ranks_exact_on_grid(N, D):
    s, m, er, ec, ties = _grid_case(N, D)
    assert ties > 0, "the case is meant to have off-diagonal entries equal to the diagonal"
    rr, rc = retrieval.pair_ranks(s.to(DEV), m.to(DEV))
    assert rr.dtype == torch.int32 and rc.dtype == torch.int32 and rr.is_cuda
    assert torch.equal(rr.cpu(), er), (N, D, int((rr.cpu() != er).sum()))
    assert torch.equal(rc.cpu(), ec), (N, D, int((rc.cpu() != ec).sum()))


@pytest.mark.parametrize("N,D", [(257, 37), (2049, 129)])
@pytest.mark.parametrize("slab_rows", [1, 100, 1024])
def test_ranks_do_not_depend_on_slab(N, D, slab_rows):
    s, m, er, ec, _ = _grid_case(N, D)
    rr, rc = retrieval.pair_ranks(s.to(DEV), m.to(DEV), slab_rows=slab_rows)
    assert torch.equal(rr.cpu(), er) and torch.equal(rc.cpu(), ec), (N, D, slab_rows)


def _random_pair(N, D, seed=15):
    g = torch.Generator().manual_seed(seed)
    s = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    m = torch.nn.functional.normalize(s + 0.6 * torch.randn(N, D, generator=g), dim=-1) * (1 / 0.07)
    return s, m


def _matrix_ranks(s, m):
    N, D = s.shape
    logits = torch.empty(N, N, device=DEV)
    hip.call("oneprot_sgemm", s, m, logits, N, N, D, 0, 0, 1.0, 0)
    rr = torch.empty(N, dtype=torch.int32, device=DEV)
    rc = torch.empty(N, dtype=torch.int32, device=DEV)
    hip.call("oneprot_diag_rank", logits, rr, rc, N)
    return rr, rc, logits


@pytest.mark.parametrize("N,D", [(300, 32), (1537, 256), (4097, 1024)])
def test_ranks_bit_identical_with_matrix_path(N, D):
    s, m = _random_pair(N, D)
    s, m = s.to(DEV), m.to(DEV)
    wr, wc, logits = _matrix_ranks(s, m)
    rr, rc = retrieval.pair_ranks(s, m)
    print(f"N {N} D {D}: rank_row differs at {int((rr != wr).sum())}, rank_col at {int((rc != wc).sum())} of {N}")
    diag = torch.empty(N, device=DEV)
    hip.call("oneprot_sim_pair_dot", s, m, diag, N, D)
    assert torch.equal(diag, logits.diagonal().contiguous()), "the diagonal is not the chain oneprot_sgemm computes"
    assert torch.equal(rr, wr) and torch.equal(rc, wc)


def test_metric_streaming_equals_reference_golden(golden_dir, monkeypatch):
    monkeypatch.setenv("ONEPROT_RETRIEVAL_STREAM", "1")
    cases = torch.load(os.path.join(golden_dir, "retrieval.pt"), weights_only=False)
    for name, c in cases.items():
        met = RetrievalMetric()
        assert met.uses_streaming(c["s"].shape[0])
        o = 0
        for n in c["cuts"]:
            met.update(c["s"][o:o + n].to(DEV), c["m"][o:o + n].to(DEV))
            o += n
        got = met.compute()
        assert set(got) == set(c["expected"]), name
        for k, v in c["expected"].items():
            assert got[k] == v, (name, k, got[k], v)


def test_metric_both_paths_agree(monkeypatch):
    s, m = _random_pair(1537, 256)
    out = {}
    for force in ("0", "1"):
        monkeypatch.setenv("ONEPROT_RETRIEVAL_STREAM", force)
        met = RetrievalMetric(k=(1, 10, 100, 500))
        for i in range(0, 1537, 500):
            met.update(s[i:i + 500].to(DEV), m[i:i + 500].to(DEV))
        out[force] = met.compute()
    assert list(out["0"]) == list(out["1"])
    for k in out["0"]:
        assert out["0"][k] == out["1"][k], (k, out["0"][k], out["1"][k])


def test_metric_streams_past_threshold_without_environment(monkeypatch):
    monkeypatch.delenv("ONEPROT_RETRIEVAL_STREAM", raising=False)
    from oneprot_amd import metrics
    called = []
    real = metrics._ranks_streaming
    monkeypatch.setattr(metrics, "_ranks_streaming", lambda s, m: (called.append(s.shape[0]), real(s, m))[1])
    monkeypatch.setattr(metrics, "_ranks_matrix", lambda s, m: pytest.fail("the matrix path ran with max_logits_bytes=0"))
    s, m = _random_pair(300, 32)
    met = RetrievalMetric(max_logits_bytes=0)
    met.update(s.to(DEV), m.to(DEV))
    got = met.compute()
    assert called == [300]
    ref = O.retrieval_metrics(s, m)
    for k in ref:
        assert abs(got[k] - ref[k]) <= (1.0 if "median" in k else 0.011), (k, got[k], ref[k])


def test_streaming_allocates_no_matrix(monkeypatch):
    """N = 8192: the matrix would be 256 MiB; the streaming compute() may add less than 32 MiB to the peak"""
    monkeypatch.setenv("ONEPROT_RETRIEVAL_STREAM", "1")
    N, D = 8192, 64
    s, m = _random_pair(N, D, seed=3)
    met = RetrievalMetric()
    met.update(s.to(DEV), m.to(DEV))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = met.compute()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise over the inputs: {rise / 2**20:.2f} MiB")
    assert rise < 32 * 2**20, rise
    assert 0.0 <= got["seq_to_mod_R@1"] <= 1.0 and got["seq_to_mod_median_rank"] >= 1.0


def _expected_topk(q, db, k):
    sim = q.numpy().astype(np.int64) @ db.numpy().astype(np.int64).T
    idx = np.arange(sim.shape[1])
    order = np.stack([np.lexsort((idx, -row))[:k] for row in sim])            # stable: descending score, then ascending index
    return torch.from_numpy(np.take_along_axis(sim, order, 1)).float(), torch.from_numpy(order)


@pytest.mark.parametrize("nq,N,D,k", [(1, 7, 4, 7), (3, 300, 4, 1), (65, 1000, 37, 10), (130, 5000, 16, 100), (33, 20000, 64, 256)])
def test_topk_exact_on_grid(nq, N, D, k):
    lim = 2 if D == 4 else 8
    q, db = _grid(nq, D, lim, 300 + N), _grid(N, D, lim, 400 + N)
    es, ei = _expected_topk(q, db, k)
    if D == 4:
        assert (es[:, 1:] == es[:, :-1]).any() or k == 1, "the case is meant to have tied scores"
    scores, indices = retrieval.topk(q.to(DEV), db.to(DEV), k)
    assert scores.shape == (nq, k) and scores.dtype == torch.float32 and indices.dtype == torch.int64
    assert torch.equal(scores.cpu(), es), (nq, N, D, k, int((scores.cpu() != es).sum()))
    assert torch.equal(indices.cpu(), ei), (nq, N, D, k, int((indices.cpu() != ei).sum()))


def test_topk_random_features_match_sgemm_scores():
    nq, N, D, k = 257, 4097, 1024, 100
    g = torch.Generator().manual_seed(23)
    q = torch.nn.functional.normalize(torch.randn(nq, D, generator=g), dim=-1).to(DEV)
    db = (torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1) * (1 / 0.07)).to(DEV)
    logits = torch.empty(nq, N, device=DEV)
    hip.call("oneprot_sgemm", q, db, logits, nq, N, D, 0, 0, 1.0, 0)
    want = torch.sort(logits, dim=1, descending=True).values[:, :k].contiguous()
    scores, indices = retrieval.topk(q, db, k)
    print(f"top-k scores differ at {int((scores != want).sum())} of {scores.numel()}")
    assert torch.equal(scores, want)
    assert int(indices.min()) >= 0 and int(indices.max()) < N
    assert torch.equal(torch.gather(logits, 1, indices), scores)


def test_retrieval_table_three_modalities():
    N, D = 300, 32
    g = torch.Generator().manual_seed(31)
    base = torch.randn(N, D, generator=g)
    embs = {n: torch.nn.functional.normalize(base + 0.6 * torch.randn(N, D, generator=g), dim=-1) for n in ("a", "b", "c")}
    dev = {n: x.to(DEV) for n, x in embs.items()}
    table = retrieval.retrieval_table(dev)
    assert list(table) == ["a-b", "a-c", "b-c"]
    for key, got in table.items():
        n1, n2 = key.split("-")
        rr, rc = retrieval.pair_ranks(dev[n1], dev[n2])
        assert got == retrieval.metrics_from_ranks(rr, rc, (1, 10, 100, 500)), key
        assert {f"{d}_R@500" for d in ("seq_to_mod", "mod_to_seq")} <= set(got)
        ref = O.retrieval_metrics(embs[n1], embs[n2])
        for k in ref:
            assert abs(got[k] - ref[k]) <= (1.0 if "median" in k else 0.011), (key, k, got[k], ref[k])
    # normalize=True on un-normalised inputs gives the table of the normalised ones up to the rounding of the norm
    raw = {n: x * 3.0 for n, x in dev.items()}
    t2 = retrieval.retrieval_table(raw, normalize=True)
    for key in table:
        for k in table[key]:
            assert abs(t2[key][k] - table[key][k]) <= (1.0 if "median" in k else 0.011), (key, k)
