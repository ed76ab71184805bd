"""The MSA input path on the device (csrc/msa_select.hip through oneprot_amd/msa_data.py): oneprot_msa_select bit for bit against the restatement of the
exact rule (tests/msa_select_ref.py) at every edge of N, L and num_seqs, on tie-heavy inputs, in batches and at one large size; the refusals;
oneprot_msa_tokenize in both layouts; MSADataset.collate_fn into a two-layer MsaEncoder."""
import functools

import numpy as np
import pytest
import torch

from tests import msa_select_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# N in {2, 3, 63, 64, 65, 257, 1000} crossed sparsely with L in {1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023}: every N and every L at least twice
NL = [(2, 1), (64, 1), (3, 3), (257, 3), (63, 15), (1000, 15), (64, 16), (2, 16), (65, 17), (1000, 17), (257, 63), (3, 63), (1000, 64), (63, 64),
      (2, 65), (257, 65), (3, 255), (64, 255), (63, 256), (1000, 256), (64, 257), (65, 257), (65, 1023), (3, 1023), (257, 1023)]


def _rows(seed, N, L, letters=21):
    return np.random.default_rng(seed).integers(65, 65 + letters, (N, L), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _full_order(key, mode):
    """the restatement's picks down to the last row: the picks for any num_seqs are a prefix (greedy never looks ahead)"""
    return R.greedy(_CASES[key], len(_CASES[key]), mode)[1]


_CASES = {}


def _want(key, rows, k, mode):
    _CASES[key] = rows
    picks = _full_order(key, mode)[:min(k, len(rows))]
    return sorted(picks), picks


def _select(arrays, ks, mode):
    from oneprot_amd import msa_data as D
    arrays, ks = D._check_batch(arrays, ks)
    idx, order = D.DeviceMsaBatch(arrays, ks, DEV).select(mode, want_order=True)
    return idx.cpu().tolist(), order.cpu().tolist()


def _padded(picks, k_max):
    return picks + [-1] * (k_max - len(picks))


@pytest.mark.parametrize("N,L", NL, ids=[f"N{n}-L{l}" for n, l in NL])
def test_select_equals_the_restatement_at_every_edge(N, L):
    rows = _rows(1000 * N + L, N, L)
    for mode in ("max", "min"):
        for k in sorted({1, 2, N - 1, N, N + 1, 50}):
            if k < 1:
                continue
            want, picks = _want(("edge", N, L), rows, k, mode)
            idx, order = _select([rows], k, mode)
            assert idx == [_padded(want, k)] and order == [_padded(picks, k)], (N, L, k, mode)


@pytest.mark.parametrize("mode", ["max", "min"])
def test_select_on_tie_heavy_inputs(mode):
    cases = {"two letters": _rows(5, 300, 8, letters=2), "two letters, short": _rows(6, 65, 3, letters=2),
             "duplicated rows": np.tile(_rows(7, 20, 130), (7, 1)), "all identical": np.tile(_rows(8, 1, 77), (130, 1))}
    for name, rows in cases.items():
        N = len(rows)
        assert not R.greedy(rows, 8, mode)[2]                                 # a tie at the top within the first steps
        for k in (2, 50, N):
            want, picks = _want(("ties", name), rows, k, mode)
            idx, order = _select([rows], k, mode)
            assert idx == [_padded(want, k)] and order == [_padded(picks, k)], (name, k)
    idx, order = _select([cases["all identical"]], 130, mode)
    assert order == [list(range(130))] and idx == order                     # every step a tie: 0, 1, 2, ...


@pytest.mark.parametrize("mode", ["max", "min"])
def test_a_batch_equals_its_solo_calls_in_any_place(mode):
    shapes = [(257, 63, 50), (5, 1023, 9), (1000, 17, 3), (64, 16, 64), (2, 1, 1), (300, 130, 128), (66, 255, 1)]
    arrays = [_rows(40 + i, N, L, letters=3 if i % 2 else 21) for i, (N, L, _) in enumerate(shapes)]
    ks = [k for _, _, k in shapes]
    solo = [_select([a], k, mode) for a, k in zip(arrays, ks)]
    for b, (a, k) in enumerate(zip(arrays, ks)):
        want, picks = _want(("batch", b), a, k, mode)
        assert solo[b] == ([_padded(want, k)], [_padded(picks, k)])
    for perm in (list(range(7)), [6, 5, 4, 3, 2, 1, 0], [2, 0, 6, 3, 5, 1, 4]):
        idx, order = _select([arrays[p] for p in perm], [ks[p] for p in perm], mode)
        for at, p in enumerate(perm):
            assert idx[at] == _padded(solo[p][0][0][:ks[p]], 128) and order[at] == _padded(solo[p][1][0][:ks[p]], 128), (perm, at)


def test_select_at_twenty_thousand_rows():
    """the chip-wide reduction (313 work-groups leave keys), int32 sums and int64 offsets"""
    rng = np.random.default_rng(2024)
    query = rng.integers(65, 86, 512, dtype=np.uint8)
    rows = np.tile(query, (20000, 1))
    hit = rng.random((20000, 512)) < rng.random((20000, 1)) * 0.6
    hit[0] = False
    rows[hit] = rng.integers(65, 86, int(hit.sum()), dtype=np.uint8)
    want, picks, _ = R.greedy(rows, 50, "max")
    idx, order = _select([rows], 50, "max")
    assert order == [picks] and idx == [want]


def test_refused_arguments_return_einval_without_a_launch():
    from oneprot_amd import hip
    rows = _rows(3, 10, 20)                                                   # stride 32: 320 bytes
    data = torch.zeros(320, dtype=torch.uint8, device=DEV)
    good = [0, 10, 20, 4]
    ws_bytes = hip.query("oneprot_msa_select_workspace", 1, 4, 10, 10)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes + 16, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 1024), 77, dtype=torch.int32, device=DEV)

    def call(table=good, n=1, k_max=4, n_bytes=320, mode=0, wsb=ws_bytes, data=data, ws=ws):
        th = torch.tensor([table], dtype=torch.int64)
        hip.call("oneprot_msa_select", data, th.to(DEV), ws, out, None, th.data_ptr(), wsb, n_bytes, n, k_max, mode)

    bad = [dict(table=[0, 0, 20, 4]), dict(table=[0, 10, 0, 4]), dict(table=[0, 10, 65536, 4]), dict(table=[0, 10, 20, 0]), dict(table=[0, 10, 20, 5]),
           dict(table=[8, 10, 20, 4]), dict(table=[16, 10, 20, 4]), dict(table=[-16, 10, 20, 4]), dict(table=[0, 11, 20, 4]), dict(n=0), dict(n=65536),
           dict(k_max=1025), dict(k_max=0), dict(mode=2), dict(wsb=ws_bytes - 1), dict(data=data[1:]), dict(ws=ws[1:]), dict(n_bytes=319)]
    for kw in bad:
        with pytest.raises(hip.HipKernelError, match="returned -1"):
            call(**kw)
    torch.cuda.synchronize()
    assert (out == 77).all()                                                  # nothing ran
    assert hip.query("oneprot_msa_select_workspace", 1, 4, 10, 11) == 0 and hip.query("oneprot_msa_select_workspace", 65536, 4, 65536, 1) == 0
    call()                                                                    # and the good call goes through
    assert out[0, :4].tolist() == R.greedy(np.zeros((10, 20), np.uint8), 4, "max")[0]
    # the tokenizer's refusals
    from oneprot_amd import msa_data as D
    batch = D.DeviceMsaBatch([rows], [4], DEV)
    idx = batch.select()
    bm = torch.from_numpy(D._byte_map()).to(DEV)
    tok = torch.full((4 * 21,), 77, dtype=torch.int64, device=DEV)

    def tokenize(R_max=4, Lt_max=21, Ls_max=22, max_length=1024, seq=None):
        hip.call("oneprot_msa_tokenize", batch.bytes, batch.table, idx, bm, tok, None, seq, batch.table_host.data_ptr(), batch.n_bytes, 1, 4, R_max, Lt_max, Ls_max,
                 max_length, 0, 0, 1, 2)

    for kw in (dict(R_max=3), dict(Lt_max=20), dict(max_length=1), dict(Ls_max=21, seq=torch.zeros(22, dtype=torch.int64, device=DEV))):
        with pytest.raises(hip.HipKernelError, match="returned -1"):
            tokenize(**kw)
    torch.cuda.synchronize()
    assert (tok == 77).all()
    tokenize()
    assert np.array_equal(tok.view(4, 21).cpu().numpy(), R.msa_tokens(rows, R.greedy(rows, 4, "max")[0], 1024))


@pytest.mark.parametrize("max_length", [8, 1024])
def test_tokens_in_both_layouts_and_the_sequence_side(max_length):
    from oneprot_amd import msa_data as D
    from oneprot_amd.packing import PackedMsa
    every_byte = np.stack([np.arange(256, dtype=np.uint8), np.arange(255, -1, -1, dtype=np.uint8), np.full(256, ord("-"), dtype=np.uint8)])
    arrays = [every_byte, _rows(2, 6, 1030), _rows(3, 9, 1022), _rows(4, 2, 1021), _rows(5, 3, 1023), _rows(6, 40, 5), _rows(7, 1, 6)]
    ks = [3, 4, 3, 2, 2, 17, 1]
    batch = D.DeviceMsaBatch(arrays, ks, DEV)
    idx = batch.select("max")
    conv = D.MsaBatchConverter(max_length=max_length)
    seq, tokens = conv.device(batch, idx)
    picks = [R.greedy(a, k, "max")[0] for a, k in zip(arrays, ks)]
    blocks = [R.msa_tokens(a, p, max_length) for a, p in zip(arrays, picks)]
    assert blocks[1].shape == (4, min(1023, max_length)) and blocks[3].shape == (2, min(1022, max_length))     # 1022 letters and <cls>, then max_length
    assert tokens.dtype == torch.int64 and tokens.is_cuda and np.array_equal(tokens.cpu().numpy(), R.padded_batch(blocks))
    if max_length == 1024:
        assert sorted(set(tokens[0, :3, 1:257].cpu().reshape(-1).tolist())) == [3] + list(range(4, 31))              # all 256 byte values went through the table
    want_seq = R.padded_seqs([R.seq_tokens(a[0], max_length) for a in arrays])
    assert seq.dtype == torch.int64 and np.array_equal(seq.cpu().numpy(), want_seq)
    seq2, pk = conv.device(batch, idx, packed=True)
    ref = PackedMsa.from_padded(tokens)
    assert isinstance(pk, PackedMsa) and pk.ids.is_cuda and torch.equal(seq2, seq) and pk.shapes == ref.shapes and pk.T_pad % 256 == 0
    assert all(torch.equal(u, v) for u, v in zip(pk.unpack(), ref.unpack()))
    assert (pk.ids[pk.n_tokens:] == 1).all() and pk.cu_tokens.tolist() == ref.cu_tokens.tolist()
    # the host path gives the same tokens
    seq_h, tokens_h = conv.host(arrays, idx.cpu())
    assert torch.equal(seq_h, seq.cpu()) and torch.equal(tokens_h, tokens.cpu())


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_collate_into_the_encoder(tmp_path, packed):
    from oneprot_amd.packing import PackedMsa
    from src.data.datasets.msa_dataset import MSADataset
    from src.models.components.msa_encoder import MsaEncoder
    from tests.msa_cases import _checkpoint
    fams = [R.draw(21, 5, 30), R.draw(22, 40, 64, kind="mutated"), R.draw(23, 200, 130)]
    files = []
    for i, seqs in enumerate(fams):
        p = tmp_path / f"fam{i}.a3m"
        p.write_text("".join(f">s{j}\n{s}\n" for j, s in enumerate(seqs)))
        files.append(str(p))
    (tmp_path / "train_msa.csv").write_text("".join(f"{i},{f}\n" for i, f in enumerate(files)))
    ds = MSADataset(str(tmp_path), "train", max_length=1024, msa_depth=16)
    ds.packed_msa = packed
    ds.device = "cpu"
    seq_h, msa_h, _, names_h = ds.collate_fn(files)
    ds.device = DEV
    seq_d, msa_d, modality, names_d = ds.collate_fn(files)
    assert modality == "msa" and names_d == names_h == [f[0] for f in fams]
    assert seq_d.is_cuda and torch.equal(seq_d.cpu(), seq_h) and tuple(seq_d.shape) == (3, 132)
    arrays = [R.to_bytes(f) for f in fams]
    blocks = [R.msa_tokens(a, R.greedy(a, 16, "max")[0], 1024) for a in arrays]
    if packed:
        assert isinstance(msa_d, PackedMsa) and msa_d.shapes == msa_h.shapes == [(5, 31), (16, 65), (16, 131)]
        assert all(np.array_equal(u.cpu().numpy(), v) for u, v in zip(msa_d.unpack(), blocks)) and torch.equal(msa_d.ids.cpu(), msa_h.ids)
    else:
        assert tuple(msa_d.shape) == (3, 16, 131) and np.array_equal(msa_d.cpu().numpy(), R.padded_batch(blocks)) and torch.equal(msa_d.cpu(), msa_h)
    enc = MsaEncoder(_checkpoint(tmp_path), output_dim=64, pooling_type="mean", proj_type="linear", use_logit_scale=False, use_all_msa=True).to(DEV)
    with torch.no_grad():
        got = enc(msa_d)
        want = enc(msa_h.to(DEV))
    assert tuple(got.shape) == (3, 64) and torch.isfinite(got).all() and torch.equal(got, want)         # identical tokens: identical bits


def test_greedy_select_chooses_the_device_by_size():
    from oneprot_amd import msa_data as D
    big, small = R.draw(31, 300, 130, kind="mutated"), R.draw(32, 20, 30)
    assert D._want_device(None, [R.to_bytes(big)]) == torch.device("cuda", torch.cuda.current_device())      # 39 000 row bytes: above DEVICE_MIN_BYTES
    assert D._want_device(None, [R.to_bytes(small)]) is None and D._want_device("cpu", [R.to_bytes(big)]) is None
    for seqs, k in ((big, 50), (small, 7)):
        msa = [(f"d{i}", s) for i, s in enumerate(seqs)]
        want = [msa[i] for i in R.greedy(R.to_bytes(seqs), k, "min")[0]]
        assert D.greedy_select(msa, k, mode="min") == want == D.greedy_select(msa, k, mode="min", device=DEV)
    assert D.select_batch([R.to_bytes(big)], 5).is_cuda and not D.select_batch([R.to_bytes(small)], 5).is_cuda
