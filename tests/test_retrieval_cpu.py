"""Host side of the streaming retrieval path (no GPU): argument validation of the new entry points, the top-k workspace size, the refusal of CPU tensors,
metrics_from_ranks on hand-written ranks, and RetrievalMetric's choice between the matrix path and the streaming path."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from oneprot_amd import hip as h
    if not os.path.exists(h.LIB_PATH):
        subprocess.check_call(["bash", os.path.join(ROOT, "oneprot_amd", "csrc", "build.sh")])
    h.lib()
    return h


@pytest.fixture(scope="module")
def bufs():
    """non-NULL host addresses: an entry point that rejects its arguments never reads them"""
    keep = [ctypes.create_string_buffer(64) for _ in range(5)]
    return keep, [ctypes.addressof(b) for b in keep]


def test_pair_dot_and_rank_reject_bad_arguments(hip, bufs):
    h = hip.lib()
    _, (a, b, c, d, e) = bufs
    assert h.oneprot_sim_pair_dot(None, b, c, 8, 4, None) == -1
    assert h.oneprot_sim_pair_dot(a, None, c, 8, 4, None) == -1
    assert h.oneprot_sim_pair_dot(a, b, None, 8, 4, None) == -1
    assert h.oneprot_sim_pair_dot(a, b, c, 0, 4, None) == -1
    assert h.oneprot_sim_pair_dot(a, b, c, -3, 4, None) == -1
    assert h.oneprot_sim_pair_dot(a, b, c, 8, 0, None) == -1
    good = [a, b, c, 8, 4, 0, 8, d, e]
    for slot in (0, 1, 2, 7, 8):                                   # each pointer NULL in turn
        args = list(good)
        args[slot] = None
        assert h.oneprot_sim_rank(*args, None) == -1, slot
    for slot, bad in ((3, 0), (3, -1), (4, 0), (4, -5), (5, -1), (6, 0), (6, 9), (5, 8)):      # N, D, row0, rows; a slab past the end
        args = list(good)
        args[slot] = bad
        assert h.oneprot_sim_rank(*args, None) == -1, (slot, bad)
    assert h.oneprot_sim_rank(a, b, c, 8, 4, 4, 5, d, e, None) == -1       # rows [4, 9) of 8


def test_topk_rejects_bad_arguments(hip, bufs):
    h = hip.lib()
    _, (a, b, c, d, e) = bufs
    nq, N, D, k = 3, 300, 4, 10
    need = h.oneprot_sim_topk_workspace(nq, N, k)
    assert need > 0
    good = [a, b, nq, N, D, k, c, d, e, need]
    for slot in (0, 1, 6, 7, 8):
        args = list(good)
        args[slot] = None
        assert h.oneprot_sim_topk(*args, None) == -1, slot
    for slot, bad in ((2, 0), (3, 0), (3, -2), (4, 0), (4, -1), (5, 0), (5, -1), (5, 257), (5, 301), (9, need - 1), (9, 0)):
        args = list(good)
        args[slot] = bad
        assert h.oneprot_sim_topk(*args, None) == -1, (slot, bad)
    assert h.oneprot_sim_topk(a, b, 3, 5, 4, 6, c, d, e, 1 << 20, None) == -1      # k > N
    assert h.oneprot_sim_topk(a, b, 3, 1000, 4, 257, c, d, e, 1 << 30, None) == -1  # k > 256 with room in N
    for bad in ((0, 10, 1), (3, 0, 1), (3, 10, 0), (3, 10, 11), (3, 1000, 257)):
        assert h.oneprot_sim_topk_workspace(*bad) == 0, bad


def test_topk_workspace_is_at_most_linear_in_queries(hip):
    h = hip.lib()
    for N, k in ((1000, 10), (1 << 20, 100), (20000, 256)):
        sizes = {nq: h.oneprot_sim_topk_workspace(nq, N, k) for nq in (1, 2, 64, 65, 1000, 4096, 8192, 100000)}
        assert all(v > 0 for v in sizes.values())
        per_query = [sizes[nq] / nq for nq in sorted(sizes)]
        assert all(b <= a for a, b in zip(per_query, per_query[1:])), (N, k, per_query)        # bytes per query never grow with nq
        assert sizes[8192] <= 2 * sizes[4096]
        # O(splits * nq * k): far below one float per (query, database row) once the database is large
        if N >= 1 << 20:
            assert sizes[4096] < 4096 * N * 4 // 16


def test_cpu_tensors_raise(hip):
    from oneprot_amd import retrieval
    s, m = torch.randn(6, 4), torch.randn(6, 4)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        retrieval.pair_ranks(s, m)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        retrieval.topk(s, m, 2)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        retrieval.retrieval_table({"a": s, "b": m})


def test_metrics_from_ranks_hand_written():
    """ref retrieval_metric.py:95-102: floor(median) + 1, R@k = mean(rank < k)"""
    from oneprot_amd.retrieval import metrics_from_ranks
    rr = torch.tensor([0, 3, 1, 12], dtype=torch.int32)        # even length: median (1 + 3) / 2 = 2 -> 3
    rc = torch.tensor([0, 1, 2, 5, 100, 7], dtype=torch.int32)  # even length, fractional median (2 + 5) / 2 = 3.5 -> floor 3 -> 4
    got = metrics_from_ranks(rr, rc, (1, 10, 100))
    assert got == {
        "seq_to_mod_median_rank": 3.0, "seq_to_mod_R@1": 0.25, "seq_to_mod_R@10": 0.75, "seq_to_mod_R@100": 1.0,
        "mod_to_seq_median_rank": 4.0, "mod_to_seq_R@1": 1 / 6, "mod_to_seq_R@10": 5 / 6, "mod_to_seq_R@100": 5 / 6,
    }
    assert list(got) == ["seq_to_mod_median_rank", "seq_to_mod_R@1", "seq_to_mod_R@10", "seq_to_mod_R@100",
                         "mod_to_seq_median_rank", "mod_to_seq_R@1", "mod_to_seq_R@10", "mod_to_seq_R@100"]
    odd = metrics_from_ranks(torch.tensor([4, 0, 9]), torch.tensor([0, 0, 0]), (1,))
    assert odd["seq_to_mod_median_rank"] == 5.0 and odd["mod_to_seq_median_rank"] == 1.0 and odd["mod_to_seq_R@1"] == 1.0


@pytest.fixture
def paths(monkeypatch):
    from oneprot_amd import metrics
    monkeypatch.delenv("ONEPROT_RETRIEVAL_STREAM", raising=False)
    monkeypatch.delenv("ONEPROT_RETRIEVAL_LOGITS_BYTES", raising=False)
    calls = []

    def fake(name):
        def f(s, m):
            calls.append((name, tuple(s.shape)))
            n = s.shape[0]
            return torch.zeros(n, dtype=torch.int32), torch.arange(n, dtype=torch.int32)
        return f
    monkeypatch.setattr(metrics, "_ranks_matrix", fake("matrix"))
    monkeypatch.setattr(metrics, "_ranks_streaming", fake("stream"))

    def run(N=4, **kw):
        met = metrics.RetrievalMetric(**kw)
        met.update(torch.randn(N, 3), torch.randn(N, 3))
        del calls[:]
        out = met.compute()
        assert len(calls) == 1 and calls[0][1] == (N, 3)
        return calls[0][0], out
    return run


def test_metric_selects_path_by_matrix_size(paths):
    from oneprot_amd import metrics
    assert metrics.RetrievalMetric().max_logits_bytes == 1 << 30 == 16384 * 16384 * 4
    assert metrics.RetrievalMetric(k=(1, 5)).k == [1, 5]
    assert paths()[0] == "matrix"                                  # 4 x 4 x 4 = 64 bytes against 1 GiB
    assert paths(max_logits_bytes=64)[0] == "matrix"               # equal to the threshold: not exceeded
    assert paths(max_logits_bytes=63)[0] == "stream"
    assert paths(max_logits_bytes=0)[0] == "stream"
    m = metrics.RetrievalMetric()
    assert not m.uses_streaming(16384) and m.uses_streaming(16385)
    name, out = paths(k=(1, 3), max_logits_bytes=0)
    assert out == {"seq_to_mod_median_rank": 1.0, "seq_to_mod_R@1": 1.0, "seq_to_mod_R@3": 1.0,
                   "mod_to_seq_median_rank": 2.0, "mod_to_seq_R@1": 0.25, "mod_to_seq_R@3": 0.75}


def test_metric_environment_overrides(paths, monkeypatch):
    monkeypatch.setenv("ONEPROT_RETRIEVAL_STREAM", "1")
    assert paths()[0] == "stream"
    monkeypatch.setenv("ONEPROT_RETRIEVAL_STREAM", "0")
    assert paths(max_logits_bytes=0)[0] == "matrix"
    monkeypatch.delenv("ONEPROT_RETRIEVAL_STREAM")
    monkeypatch.setenv("ONEPROT_RETRIEVAL_LOGITS_BYTES", "10")
    assert paths()[0] == "stream"                                  # the default threshold comes from the environment ...
    assert paths(max_logits_bytes=1 << 20)[0] == "matrix"          # ... an explicit argument wins
