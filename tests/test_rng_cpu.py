"""oneprot_amd/rng.py: the domain table, the stream-id layout, the process-wide tower numbering and the state of the four kinds of stream owner."""
import copy

import pytest
import torch

from oneprot_amd import gbt, probe, pronet, rng
from oneprot_amd.bert import BertTransformer
from oneprot_amd.esm import ESM_DEFAULTS, ArenaModule, EsmTransformer, ModelConfig

PARENT_DROP = {"_drop_seed": 5, "_drop_calls": 7, "_rng_uid": 9}          # the dicts as the commit before rng.py wrote them into checkpoints
PARENT_LORA = {"_lora_seed": 5, "_lora_calls": 7, "_rng_uid": 9}


def _bert():
    return BertTransformer(ModelConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4, vocab_size=30, max_position_embeddings=16,
                                       hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))


def _esm():
    cfg = dict(ESM_DEFAULTS)
    cfg.update(hidden_size=40, num_hidden_layers=1, num_attention_heads=2, intermediate_size=80)
    return EsmTransformer(ModelConfig(**cfg), add_pooling_layer=False)


def _pronet():
    return pronet.ProNet(level="backbone", num_blocks=1, hidden_channels=64, out_channels=4)


def _mlp():
    return probe.MLP(8, 2, hidden_dims=[4], dropout_rate=0.5)


def test_domain_table():
    assert rng.DOMAINS == {"bert": 1, "lora": 2, "msa": 3, "pronet": 4, "probe": 5, "gbt": 6} and len(set(rng.DOMAINS.values())) == 6
    assert (ArenaModule.RNG_DOMAIN_BERT, ArenaModule.RNG_DOMAIN_LORA, ArenaModule.RNG_DOMAIN_MSA) == (1, 2, 3)
    assert (pronet.RNG_DOMAIN_PRONET, probe.RNG_DOMAIN_PROBE, gbt.RNG_DOMAIN_GBT) == (4, 5, 6)


def test_stream_id_literals():
    uid = 0xBEEF
    assert rng.stream_id(3, uid, 34) == (3 << 60) | (uid << 44) | 34
    assert rng.stream_id(6, None, 7) == gbt.stream_of(7) == (6 << 60) | 7
    assert rng.stream_id(1, 0xFFFF, (1 << 44) + 5) == (1 << 60) | (0xFFFF << 44) | 5          # the local field is 44 bits wide under a tower ...
    assert rng.stream_id(6, None, (1 << 59) + (1 << 44) + 5) == (6 << 60) | (1 << 59) | (1 << 44) | 5 and rng.stream_id(6, None, 1 << 60) == 6 << 60      # ... and 60 without


def test_next_uid_numbers_every_kind_of_tower_consecutively():
    towers = [_bert(), _esm(), _pronet(), _mlp()]
    first = towers[0]._rng_uid
    assert [t._rng_uid for t in towers] == [(first + i) & 0xFFFF for i in range(4)]
    assert rng.next_uid() == (first + 4) & 0xFFFF
    assert not hasattr(ArenaModule, "_next_rng_uid")


@pytest.mark.parametrize("make, parent", [(_bert, PARENT_DROP), (_esm, PARENT_LORA), (_pronet, PARENT_DROP), (_mlp, PARENT_DROP)])
def test_rng_state_is_a_fixed_point_and_reads_the_parent_format(make, parent):
    tower = make()
    if make is _esm:
        assert tower.rng_state() == {}                      # no stream started: nothing to carry
        torch.manual_seed(31)
        tower.enable_lora(2, 4, ["query", "key", "value"], dropout=0.1)
        assert tower.rng_state() == {"_lora_seed": 31, "_lora_calls": 0, "_rng_uid": tower._rng_uid}
    elif make is _bert:
        assert tower.rng_state() == {}
        torch.manual_seed(32)
        assert [tower._next_call(), tower._next_call()] == [0, 1]            # the lazy policy: seeded from torch.initial_seed() by the first draw
        assert tower.rng_state() == {"_drop_seed": 32, "_drop_calls": 2, "_rng_uid": tower._rng_uid}
    else:
        assert tower.rng_state() == {"_drop_seed": 0x5EED0000 + tower._rng_uid, "_drop_calls": 0, "_rng_uid": tower._rng_uid}      # the fixed policy
        assert tower._next_call() == 0 and tower._drop_calls == 1
    st = tower.rng_state()
    tower.set_rng_state(st)
    assert tower.rng_state() == st
    other = make()
    if make is _esm:
        other.enable_lora(2, 4, ["query", "key", "value"], dropout=0.1)
    other.set_rng_state(dict(parent))
    assert other.rng_state() == parent
    assert all(type(getattr(other, k)) is int and getattr(other, k) == v for k, v in parent.items())      # plain attributes under the same names


def test_deepcopy_of_a_probe_keeps_its_stream_state():
    m = _mlp()
    m.set_rng_state(PARENT_DROP)
    c = copy.deepcopy(m)
    assert c.rng_state() == PARENT_DROP and c.stream_of(7, 0) == m.stream_of(7, 0) == (5 << 60) | (9 << 44) | 7
    assert c._next_call() == 7 and m._drop_calls == 7          # the copy draws on; the original's counter stays
