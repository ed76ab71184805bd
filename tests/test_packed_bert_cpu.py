"""Packed caption streams for the BERT text tower, the host side that needs no GPU: what SyntheticPairs hands out, what TextEncoder refuses and in
which order (pad id of the stream, caption length, device)."""
import json
import os

import pytest
import torch

from oneprot_amd import hip
from oneprot_amd.data import SyntheticPairs
from oneprot_amd.packing import PackedTokens


def _rows(lengths, pad=0, vocab=120):
    """right-padded caption ids: [CLS] = 2, body 5 .. vocab-1, [SEP] = 3"""
    gen = torch.Generator().manual_seed(sum(lengths))
    ids = torch.full((len(lengths), max(lengths)), pad, dtype=torch.int64)
    for b, n in enumerate(lengths):
        ids[b, :n] = torch.randint(5, vocab, (n,), generator=gen)
        ids[b, 0] = 2
        if n > 1:
            ids[b, n - 1] = 3
    return ids


@pytest.fixture
def text_encoder(tmp_path, monkeypatch):
    from oneprot_amd.encoders import TextEncoder
    d = os.path.join(str(tmp_path), "bert")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=120, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                       max_position_embeddings=64, pad_token_id=0, layer_norm_eps=1e-12), f)
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    return TextEncoder(d, output_dim=32)


def test_synthetic_pairs_pack_the_text_side():
    rag = next(iter(SyntheticPairs("text", 12, 200, seed=4, ragged=True, text_vocab=1000)))
    pk = next(iter(SyntheticPairs("text", 12, 200, seed=4, packed=True, packed_text=True, text_vocab=1000)))
    assert isinstance(pk[0], PackedTokens) and isinstance(pk[1], PackedTokens)
    assert pk[1].pad_id == 0 and pk[0].pad_id == 1
    assert len(pk[1]) == 12 and pk[1].T_pad % 256 == 0
    padded = pk[1].to_padded()
    assert torch.equal(padded, rag[1][:, :padded.shape[1]])
    assert (rag[1][:, padded.shape[1]:] == 0).all()
    # without packed_text (and without packed) nothing changes
    assert torch.equal(next(iter(SyntheticPairs("text", 12, 200, seed=4, packed=True, text_vocab=1000)))[1], rag[1])
    assert torch.equal(next(iter(SyntheticPairs("text", 12, 200, seed=4, ragged=True, packed_text=True, text_vocab=1000)))[1], rag[1])
    st = next(iter(SyntheticPairs("struct_token", 6, 64, seed=4, packed=True, packed_text=True)))
    assert st[1].pad_id == 1


def test_cpu_stream_with_the_towers_pad_id_reaches_the_device_check(text_encoder):
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):
        text_encoder(PackedTokens.from_padded(_rows([9, 4]), pad_id=0))


def test_stream_with_another_pad_id_is_refused(text_encoder):
    with pytest.raises(NotImplementedError, match="packed BERT") as e:
        text_encoder(PackedTokens.from_padded(_rows([9, 4], pad=1), pad_id=1))
    assert "from_padded(ids, pad_id=0)" in str(e.value)


def test_caption_longer_than_the_position_table_is_refused(text_encoder):
    with pytest.raises(ValueError, match="max_position_embeddings"):
        text_encoder(PackedTokens.from_padded(_rows([9, 70]), pad_id=0))
    with pytest.raises(hip.HipKernelError, match="no CPU fallback"):      # 64 = max_position_embeddings still fits
        text_encoder(PackedTokens.from_padded(_rows([9, 64]), pad_id=0))


def test_struct_encoder_keeps_refusing_packed_input():
    from oneprot_amd.encoders import StructEncoder
    enc = StructEncoder(torch.nn.Linear(4, 8), output_dim=8)
    with pytest.raises(NotImplementedError):
        enc(PackedTokens.from_padded(_rows([9, 4]), pad_id=0))
