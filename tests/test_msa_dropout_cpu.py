"""The MSA tower's train-mode dropout without a device: the fp64 restatement with masks (tests/msa_dropout_ref.py) against the eval-mode one, the dropout
probabilities read from a fair-esm file, the stream numbering, the checkpointed stream state and the statistics of the mask hash in the column layout."""
import argparse
import itertools
import os

import numpy as np
import pytest
import torch

from tests import msa_dropout_ref as DR
from tests import msa_ref as MR
from tests import philox_ref as PR
from tests.msa_cases import ARCH, _tower  # noqa: F401

F64 = torch.float64
@pytest.mark.parametrize("R", [3, 1])
def test_all_ones_masks_reproduce_the_eval_forward_exactly(R):
    tr = _tower()
    with torch.no_grad():
        tr.flat.normal_(0.0, 0.08)
    sd = {k: v.detach().to(F64) for k, v in tr.state_dict().items()}
    g = torch.Generator().manual_seed(8)
    B, L = 2, 11
    tok = torch.randint(4, 30, (B, R, L), generator=g)
    tok[:, :, 0] = 0
    tok[1, :, 8:] = 1
    tok[0, R - 1, 4] = 1
    ones = lambda *s: (torch.ones(*s, dtype=torch.bool), 1.0)
    masks = {(-1, 0): ones(B, R, L, 128)}
    for i in range(2):
        masks.update({(i, 0): ones(B, 2, L, L), (i, 2): ones(B, 2, L, R, R), (i, 1): ones(B, R, L, 128), (i, 3): ones(B, R, L, 128),
                      (i, 4): ones(B, R, L, 256), (i, 5): ones(B, R, L, 128)})
    ref = MR.forward(tok, sd, 2)
    assert torch.equal(DR.forward(tok, sd, 2, masks), ref) and torch.equal(DR.forward(tok, sd, 2, {}), ref)
    assert float(ref.abs().max()) > 0.1
    # ... and a real mask moves it, at every site on its own
    for key in masks:
        if key[1] == 2 and R == 1:
            continue                                      # the one-row shortcut has no probabilities to drop
        keep = torch.rand(masks[key][0].shape, generator=g) >= 0.5
        assert float((DR.forward(tok, sd, 2, {key: (keep, 2.0)}) - ref).abs().max()) > 1e-6, key
    if R == 1:
        keep = torch.zeros(B, 2, L, 1, 1, dtype=torch.bool)
        assert torch.equal(DR.forward(tok, sd, 2, {(0, 2): (keep, 2.0)}), ref)


def _write(path, tr, **entry):
    sw = lambda k: k.replace("row", "\0").replace("column", "row").replace("\0", "column")
    torch.save({**entry, "model": {"encoder." + sw(k): v.clone() for k, v in tr.state_dict().items()}}, path)


def test_dropout_probabilities_from_args_cfg_and_default(tmp_path):
    from oneprot_amd.msa import MsaTransformer
    tr = _tower()
    path = os.path.join(str(tmp_path), "m.pt")
    _write(path, tr, args=argparse.Namespace(arch="msa_transformer", dropout=0.2, attention_dropout=0.05, activation_dropout=0.0, **ARCH))
    assert MsaTransformer.from_pretrained(path)._drop_probs() == (0.2, 0.05, 0.0)
    _write(path, tr, cfg={"model": dict(ARCH, dropout=0.3, attention_dropout=0.25, activation_dropout=0.125)})
    assert MsaTransformer.from_pretrained(path)._drop_probs() == (0.3, 0.25, 0.125)
    _write(path, tr, args=argparse.Namespace(arch="msa_transformer", **ARCH))
    got = MsaTransformer.from_pretrained(path)
    assert got._drop_probs() == (0.1, 0.1, 0.1) and (got.n_layers, got.d) == (2, 128)


def test_stream_ids_are_distinct_and_in_their_own_domain():
    from oneprot_amd.bert import BertTransformer
    from oneprot_amd.esm import ArenaModule
    tr = _tower()
    assert ArenaModule.RNG_DOMAIN_MSA == 3 and len({ArenaModule.RNG_DOMAIN_BERT, ArenaModule.RNG_DOMAIN_LORA, ArenaModule.RNG_DOMAIN_MSA}) == 3
    ids = [tr._drop_stream(c, -1, 0) for c in range(3)] + [tr._drop_stream(c, i, s) for c, i, s in itertools.product(range(3), range(tr.n_layers), range(6))]
    assert len(set(ids)) == len(ids) == 3 * (1 + 6 * tr.n_layers)
    assert all(i >> 60 == 3 and (i >> 44) & 0xFFFF == tr._rng_uid for i in ids)
    assert tr._drop_stream(1, 0, 2) == (3 << 60) | (tr._rng_uid << 44) | ((1 * 3 + 1) * 8 + 2)
    # the other consumers of the same tower id live in other domains
    other = {tr._rng_stream(dom, loc) for dom in (ArenaModule.RNG_DOMAIN_BERT, ArenaModule.RNG_DOMAIN_LORA) for loc in range(4096)}
    other |= {BertTransformer._drop_stream(tr, c, i, s) for c, i, s in itertools.product(range(3), range(-1, tr.n_layers), range(4))}
    assert not other & set(ids)


def test_rng_state_round_trips_seed_and_call_counter():
    tr = _tower()
    assert tr.rng_state() == {}                           # nothing drawn yet: nothing to carry
    torch.manual_seed(77)
    assert [tr._next_drop_call() for _ in range(3)] == [0, 1, 2]
    st = tr.rng_state()
    assert st == {"_drop_seed": 77, "_drop_calls": 3, "_rng_uid": tr._rng_uid}
    other = _tower()
    other.set_rng_state(st)
    assert other.rng_state() == st and other._next_drop_call() == 3 and other._drop_stream(3, 0, 1) == tr._drop_stream(3, 0, 1)


def test_switch_defaults_off_and_follows_the_environment(monkeypatch):
    tr = _tower()
    monkeypatch.delenv("ONEPROT_MSA_DROPOUT", raising=False)
    assert tr.train_dropout is None and not tr.dropout_enabled()
    monkeypatch.setenv("ONEPROT_MSA_DROPOUT", "1")
    assert tr.dropout_enabled()
    tr.train_dropout = False
    assert not tr.dropout_enabled()
    monkeypatch.setenv("ONEPROT_MSA_DROPOUT", "0")
    tr.train_dropout = True
    assert tr.dropout_enabled()
    tr.train()
    assert not tr.training                                # the tower's own mode never follows .train()


STREAMS = [(3 << 60) | (7 << 44) | 5, (3 << 60) | (7 << 44) | 6, (3 << 60) | (0xBEEF << 44) | 1169]


@pytest.mark.parametrize("stream", STREAMS, ids=[hex(s) for s in STREAMS])
def test_column_layout_of_the_hash_is_statistically_sound(stream):
    """attn_keep(B * H * L, 1, R, ...): the column attention puts (b, h, l) where the BERT tower has (b, h) -- up to 2^26 slots, neighbours one apart.
    Keep fraction within 4 sigma of 0.9 over 2 * 2 * 33 * 50 * 50 = 330 000 elements, and adjacent slots agree on 0.9^2 + 0.1^2 = 0.82 of their elements,
    as independent masks do (0.82 +- 0.01).  Measured with seed 0x1234567: +0.96 / +0.68 / +0.79 sigma, agreement 0.8211 / 0.8205 / 0.8207."""
    keep = PR.attn_keep(2 * 2 * 33, 1, 50, 0.1, 0x1234567, stream).reshape(2 * 2 * 33, 50, 50)
    n = keep.size
    assert n == 330000
    thr, _ = PR.dropout_threshold(0.1)
    q = 1.0 - thr / 65536.0
    z = (keep.mean() - q) / np.sqrt(q * (1 - q) / n)
    agree = (keep[1:] == keep[:-1]).mean()
    print(f"stream {stream:#x}: keep fraction {keep.mean():.5f} ({z:+.2f} sigma), adjacent-slot agreement {agree:.4f}")
    assert abs(keep.mean() - 0.9) < 4 * np.sqrt(0.09 / n)
    assert abs(agree - 0.82) < 0.01
