"""Packed (variable-length) ESM batches without a GPU: the PackedTokens type, the packed synthetic batches, and the encoders' refusal of host tensors."""
import os

import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.data import SyntheticPairs
from oneprot_amd.packing import MAX_SEGMENT, PAD_MULTIPLE, PackedTokens, batch_size


def _rows(lengths, seed=0, pad=1):
    gen = torch.Generator().manual_seed(seed)
    L = max(lengths)
    ids = torch.full((len(lengths), L), pad, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = torch.randint(4, 24, (n,), generator=gen)
        ids[b, 0], ids[b, n - 1] = 0, 2
    return ids


def test_from_list_and_from_padded_agree():
    lengths = [37, 20, 37, 5, 300]
    padded = _rows(lengths)
    a = PackedTokens.from_padded(padded, pad_id=1)
    b = PackedTokens.from_list([padded[i, :n] for i, n in enumerate(lengths)], pad_id=1)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.cu_seqlens, b.cu_seqlens)
    assert a.cu_seqlens.dtype == torch.int32 and a.ids.dtype == torch.int64
    assert a.cu_seqlens.tolist() == [0, 37, 57, 94, 99, 399]
    assert a.max_len == 300 and len(a) == 5 and batch_size(a) == 5 and a.lengths == lengths
    assert torch.equal(a.to_padded(), padded)
    for s, n, i in zip(a.unpack(), lengths, range(5)):
        assert torch.equal(s, padded[i, :n])


def test_t_pad_multiple_of_256_and_pad_tail():
    for lengths in ([1], [255], [256], [257], [100, 200, 300], [1026] * 3):
        p = PackedTokens.from_list([torch.arange(n) % 20 + 4 for n in lengths])
        assert p.T_pad % PAD_MULTIPLE == 0 and p.T_pad >= sum(lengths) > p.T_pad - PAD_MULTIPLE
        assert (p.ids[sum(lengths):] == 1).all()
    p = PackedTokens.from_list([torch.arange(10) + 4], pad_id=0, t_pad=512)
    assert p.T_pad == 512 and (p.ids[10:] == 0).all()


def test_invalid_inputs_are_rejected():
    with pytest.raises(ValueError, match="empty"):
        PackedTokens.from_list([torch.arange(5), torch.zeros(0, dtype=torch.int64)])
    with pytest.raises(ValueError, match="1026"):
        PackedTokens.from_list([torch.arange(MAX_SEGMENT + 1)])
    PackedTokens.from_list([torch.arange(MAX_SEGMENT)])                        # the limit itself is fine
    with pytest.raises(ValueError, match="1-D"):
        PackedTokens.from_list([torch.zeros(2, 3, dtype=torch.int64)])
    with pytest.raises(ValueError, match="integers"):
        PackedTokens.from_list([torch.rand(7)])
    with pytest.raises(ValueError, match="integers"):
        PackedTokens.from_padded(torch.rand(2, 7))
    with pytest.raises(ValueError):
        PackedTokens.from_list([])
    with pytest.raises(ValueError, match="empty"):                            # an all-padding row is an empty sequence
        PackedTokens.from_padded(torch.tensor([[0, 5, 2], [1, 1, 1]]))
    with pytest.raises(ValueError, match="multiple"):
        PackedTokens.from_list([torch.arange(10)], t_pad=300)
    with pytest.raises(ValueError, match="int64"):
        PackedTokens(torch.zeros(256, dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), 4)


def test_batch_element_protocol():
    p = PackedTokens.from_padded(_rows([9, 4, 7]))
    q = p.to("cpu")
    assert len(q) == 3 and q.T_pad == 256 and torch.equal(q.ids, p.ids) and not q.is_cuda
    w = p.attn_work()
    assert w.dtype == torch.int32 and w.shape == (3, 2)
    assert w[:, 0].tolist() == [0, 2, 1]                                       # longest first
    long = PackedTokens.from_list([torch.arange(40) % 20 + 4, torch.arange(300) % 20 + 4])
    assert long.attn_work().tolist() == [[1, 0], [1, 1], [1, 2], [0, 0]]


def test_synthetic_packed_batches_are_the_ragged_rows():
    for modality in ("struct_token", "sequence", "text"):
        rag = list(SyntheticPairs(modality, 16, 128, n_batches=3, seed=5, ragged=True))
        pk = list(SyntheticPairs(modality, 16, 128, n_batches=3, seed=5, packed=True))
        for (rs, rm, name, _), (ps, pm, name2, _) in zip(rag, pk):
            assert name == name2
            assert isinstance(ps, PackedTokens) and len(ps) == 16
            assert torch.equal(ps.to_padded(128), rs)
            if modality == "text":                   # the BERT side stays padded
                assert torch.equal(pm, rm)
            else:
                assert torch.equal(pm.to_padded(128), rm)


def test_encoders_refuse_host_packed_input(tmp_path, monkeypatch):
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    import json
    from oneprot_amd.encoders import SequenceEncoder, StructEncoder, StructTokenEncoder
    from oneprot_amd.data import StandInGraphEncoder
    d = os.path.join(str(tmp_path), "esm")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(model_type="esm", vocab_size=33, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128), f)
    p = PackedTokens.from_padded(_rows([9, 4, 7]))
    seq = SequenceEncoder(d, output_dim=32, use_lora=False, frozen=False)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        seq(p)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        StructTokenEncoder(d, output_dim=32)(p)
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        seq.transformer(p)
    with pytest.raises(NotImplementedError, match="graph encoder"):
        StructEncoder(StandInGraphEncoder(16, 32, 32), output_dim=32)(p)


def test_text_encoder_refuses_packed_input(tmp_path, monkeypatch):
    import json
    from oneprot_amd.encoders import TextEncoder
    d = os.path.join(str(tmp_path), "bert")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                       max_position_embeddings=64, pad_token_id=0, layer_norm_eps=1e-12), f)
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    enc = TextEncoder(d, output_dim=32)
    with pytest.raises(NotImplementedError, match="packed BERT"):
        enc(PackedTokens.from_padded(_rows([9, 4]), pad_id=1))


def test_pair_size_mismatch_is_a_clear_error():
    from oneprot_amd.module import OneProtLitModule
    a = PackedTokens.from_padded(_rows([9, 4, 7]))
    with pytest.raises(ValueError, match="same number"):
        OneProtLitModule._check_pair(a, _rows([5, 5]), "struct_token")
    OneProtLitModule._check_pair(a, _rows([5, 5, 6]), "text")                 # a padded text side of the same N is fine
