"""Ranks with tie counts (oneprot_sim_rank_ties, retrieval.pair_ranks(..., ties=True)) on the MI355X.

Everything here is an equality.  Integer features in [-3, 3] make every dot product exact in fp32 in any summation order, so int64 numpy gives the expected
ranks `(sim > diag).sum()` and ties `(sim == diag).sum() - 1` (the matching pair removed by its index) in both directions.  On random fp32 features the ranks
must be oneprot_sim_rank's bit for bit and the ties are `==` counted on the host in the oneprot_sgemm matrix, which the header promises is bit-equal to the tiles.

The grid inputs are built as two groups so that a case holds both kinds of rows.  Group A (the first third): s_i = m_i = a random vector of +-3, whose
matching similarity 9 D is the largest value any pair of such vectors can reach and is reached by an equal vector only -- no tie in either direction once
D is large enough for the sign vectors to be distinct.  Group B: random integers with planted duplicate pairs, which tie.  "At least a quarter of the rows
tie and at least a quarter do not" is asserted where arithmetic allows it, D >= 64 and N >= 127.  It cannot hold elsewhere: at D = 1 and D = 3 there are 7 and
343 distinct rows, so past a handful of rows every matching similarity is met again (pigeonhole), and N = 1, 2 have no or one other candidate.  Those cases
still check ranks and ties against numpy exactly, and assert of their input what it does hold (ties present from N = 127 on)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oneprot_amd import hip, retrieval  # noqa: E402

DEV = "cuda"
NS = (1, 2, 127, 128, 129, 300, 2100)          # 2100: 17 row tiles, past the 16 that run together
DS = (1, 3, 64, 130)
_cache = {}


def _grid_case(N, D):
    if (N, D) not in _cache:
        g = torch.Generator().manual_seed(1000 * N + D)
        s = torch.randint(-3, 4, (N, D), generator=g).float()
        m = torch.randint(-3, 4, (N, D), generator=g).float()
        a = N // 3
        s[:a] = (torch.randint(0, 2, (a, D), generator=g) * 6 - 3).float()
        m[:a] = s[:a]
        b0 = a + (N - a) // 2                     # the second half of group B repeats the first half, pair by pair: ties in both directions
        for i in range(b0, N):
            src = a + (i - b0)
            if src < b0:
                s[i], m[i] = s[src], m[src]
        sim = s.numpy().astype(np.int64) @ m.numpy().astype(np.int64).T
        d = np.diag(sim)
        want = ((sim > d[:, None]).sum(1), (sim > d[None, :]).sum(0), (sim == d[:, None]).sum(1) - 1, (sim == d[None, :]).sum(0) - 1)
        _cache[(N, D)] = (s, m, tuple(torch.from_numpy(w).int() for w in want))
    return _cache[(N, D)]


@pytest.mark.parametrize("slab_rows", [None, 128, 200])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("N", NS)
def test_ranks_and_ties_exact_on_integer_features(N, D, slab_rows):
    s, m, want = _grid_case(N, D)
    for name, t in (("row", want[2]), ("col", want[3])):
        tied = int((t > 0).sum())
        if D >= 64 and N >= 127:
            assert 4 * tied >= N and 4 * (N - tied) >= N, (N, D, name, tied)
        elif N >= 127:
            assert 4 * tied >= N, (N, D, name, tied)
    got = retrieval.pair_ranks(s.to(DEV), m.to(DEV), slab_rows=slab_rows, ties=True)
    assert len(got) == 4
    for name, g, w in zip(("rank_row", "rank_col", "tie_row", "tie_col"), got, want):
        assert g.dtype == torch.int32 and g.is_cuda and g.shape == (N,)
        assert torch.equal(g.cpu(), w), (N, D, slab_rows, name, int((g.cpu() != w).sum()))


def test_zero_diagonal_gets_no_ties_from_padding():
    """N = 129, D = 3: the second column tile holds one real column and 127 zero-padded ones, the second row tile likewise.  Rows whose matching similarity
    is exactly 0 -- by a zero row, and by orthogonal non-zero rows -- must count the real candidates only."""
    N, D = 129, 3
    g = torch.Generator().manual_seed(7)
    s = torch.randint(-3, 4, (N, D), generator=g).float()
    m = torch.randint(-3, 4, (N, D), generator=g).float()
    for i in (0, 5, 127, 128):
        s[i] = 0.0                                   # every similarity of the row is 0: N - 1 ties, not 255
    for i in (1, 64, 126):
        s[i], m[i] = torch.tensor([1.0, 1.0, 0.0]), torch.tensor([2.0, -2.0, 3.0])
    m[128] = 0.0                                     # a zero column: diag 0, every similarity of the column is 0
    sim = s.numpy().astype(np.int64) @ m.numpy().astype(np.int64).T
    d = np.diag(sim)
    assert (d == 0).sum() >= 7
    want_tr, want_tc = (sim == d[:, None]).sum(1) - 1, (sim == d[None, :]).sum(0) - 1
    assert want_tr[0] == N - 1 and want_tc[128] == N - 1
    for slab_rows in (None, 100):
        rr, rc, tr, tc = retrieval.pair_ranks(s.to(DEV), m.to(DEV), slab_rows=slab_rows, ties=True)
        assert torch.equal(tr.cpu(), torch.from_numpy(want_tr).int()), (slab_rows, tr.cpu()[[0, 5, 127, 128]].tolist())
        assert torch.equal(tc.cpu(), torch.from_numpy(want_tc).int()), (slab_rows, int(tc[128]))
        assert torch.equal(rr.cpu(), torch.from_numpy((sim > d[:, None]).sum(1)).int())
        assert torch.equal(rc.cpu(), torch.from_numpy((sim > d[None, :]).sum(0)).int())


def _random_pair_with_duplicates(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=-1)
    m = torch.nn.functional.normalize(s + 0.6 * torch.randn(N, D, generator=g), dim=-1) * (1 / 0.07)
    for i in range(0, N - 1, 5):                     # every fifth pair is repeated by its neighbour: bit-identical rows, exact ties in both directions
        s[i + 1], m[i + 1] = s[i], m[i]
    return s.to(DEV), m.to(DEV)


@pytest.mark.parametrize("N,D", [(2100, 130), (513, 1024)])
def test_random_features_ranks_equal_plain_kernel_and_ties_equal_sgemm(N, D):
    s, m = _random_pair_with_duplicates(N, D, 15 + N)
    pr, pc = retrieval.pair_ranks(s, m)
    rr, rc, tr, tc = retrieval.pair_ranks(s, m, ties=True)
    assert torch.equal(rr, pr) and torch.equal(rc, pc), (int((rr != pr).sum()), int((rc != pc).sum()))
    logits = torch.empty(N, N, device=DEV)
    hip.call("oneprot_sgemm", s, m, logits, N, N, D, 0, 0, 1.0, 0)
    sim = logits.cpu().numpy()
    d = np.diag(sim)
    want_tr, want_tc = (sim == d[:, None]).sum(1) - 1, (sim == d[None, :]).sum(0) - 1
    assert want_tr.sum() > 0 and want_tc.sum() > 0 and (want_tr == 0).sum() > N // 4
    assert torch.equal(tr.cpu(), torch.from_numpy(want_tr).int()), int((tr.cpu().numpy() != want_tr).sum())
    assert torch.equal(tc.cpu(), torch.from_numpy(want_tc).int()), int((tc.cpu().numpy() != want_tc).sum())


def test_deterministic_and_independent_of_slab():
    s, m = _random_pair_with_duplicates(2100, 130, 2115)
    first = retrieval.pair_ranks(s, m, ties=True)
    again = retrieval.pair_ranks(s, m, ties=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for slab_rows in (1, 128, 200, 1024):
        other = retrieval.pair_ranks(s, m, slab_rows=slab_rows, ties=True)
        assert all(torch.equal(a, b) for a, b in zip(first, other)), slab_rows


def test_pessimistic_bound_is_rank_plus_ties():
    s, m, want = _grid_case(300, 64)
    rr, rc, tr, tc = retrieval.pair_ranks(s.to(DEV), m.to(DEV), ties=True)
    ks = (1, 10, 100, 500)
    opt = retrieval.metrics_from_ranks(rr, rc, ks)
    assert opt == retrieval.metrics_from_ranks(rr, rc, ks, ties=(tr, tc)) == retrieval.metrics_from_ranks(want[0], want[1], ks)
    pes = retrieval.metrics_from_ranks(rr, rc, ks, ties=(tr, tc), bound="pessimistic")
    assert pes == retrieval.metrics_from_ranks(want[0] + want[2], want[1] + want[3], ks)
    assert pes["seq_to_mod_R@100"] < opt["seq_to_mod_R@100"] and pes["mod_to_seq_median_rank"] > opt["mod_to_seq_median_rank"]      # of this input, on the host
    assert all(pes[k] <= opt[k] for k in opt if "R@" in k)
    embs = {"a": s.to(DEV), "b": m.to(DEV)}
    rows = {}
    assert retrieval.retrieval_table(embs, ks) == {"a-b": opt}
    assert retrieval.retrieval_table(embs, ks, bound="pessimistic", tie_rows=rows) == {"a-b": pes}
    assert rows == {"a-b": (int((want[2] > 0).sum()), int((want[3] > 0).sum()))}
    with pytest.raises(ValueError):
        retrieval.metrics_from_ranks(rr, rc, ks, bound="pessimistic")
