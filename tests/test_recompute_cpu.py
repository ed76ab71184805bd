"""Activation recomputation, host side: the segment plan, the switch (attribute / ONEPROT_RECOMPUTE_LAYERS) and the encoder-level setter."""
import json
import os

import pytest

from oneprot_amd.esm import EsmTransformer, ModelConfig, ESM_DEFAULTS, recompute_plan


def _tower(layers=6):
    cfg = dict(ESM_DEFAULTS)
    cfg.update(hidden_size=40, num_hidden_layers=layers, num_attention_heads=2, intermediate_size=80)     # head_dim 20: runs padded to 32; never launched here
    return EsmTransformer(ModelConfig(**cfg), add_pooling_layer=False)


@pytest.mark.parametrize("n", [1, 6, 30, 33])
def test_plan_covers_every_layer_once_in_order(n):
    for k in (1, 2, 4, 6, 7, n, n + 3):
        plan = recompute_plan(n, k)
        assert [i for lo, hi in plan for i in range(lo, hi)] == list(range(n)), (n, k, plan)
        assert all(lo % k == 0 and 0 < hi - lo <= k for lo, hi in plan), (n, k, plan)      # boundaries at multiples of k, only the last one short
        assert all(hi - lo == k for lo, hi in plan[:-1])
        assert len(plan) == -(-n // k)
        if k >= n:
            assert plan == [(0, n)]


def test_plan_off_is_none():
    for n in (1, 6, 33):
        assert recompute_plan(n, 0) is None


@pytest.mark.parametrize("bad", [-1, 2.0, "3", None, True, [2]])
def test_plan_rejects_bad_k(bad):
    with pytest.raises(ValueError):
        recompute_plan(6, bad)


def test_environment_parsing(monkeypatch):
    tr = _tower()
    assert tr.recompute_layers is None
    monkeypatch.delenv("ONEPROT_RECOMPUTE_LAYERS", raising=False)
    assert tr._recompute_k() == 0
    for raw, want in (("0", 0), ("3", 3), (" 6 ", 6), ("", 0)):
        monkeypatch.setenv("ONEPROT_RECOMPUTE_LAYERS", raw)
        assert tr._recompute_k() == want                     # read at call time, not at construction
    for raw in ("-1", "two", "1.5"):
        monkeypatch.setenv("ONEPROT_RECOMPUTE_LAYERS", raw)
        with pytest.raises(ValueError):
            tr._recompute_k()
    monkeypatch.setenv("ONEPROT_RECOMPUTE_LAYERS", "4")
    tr.recompute_layers = 2                                  # the attribute wins over the environment
    assert tr._recompute_k() == 2
    tr.recompute_layers = 0
    assert tr._recompute_k() == 0
    tr.recompute_layers = -2                                 # validated where it is read
    with pytest.raises(ValueError):
        tr._recompute_k()


def test_switch_is_not_part_of_the_state_dict():
    a, b = _tower(), _tower()
    b.recompute_layers = 3
    assert list(a.state_dict()) == list(b.state_dict())
    assert not any("recompute" in k for k in b.state_dict())


def _write(tmp, name, **cfg):
    path = os.path.join(str(tmp), name)
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    return path


def test_setter_on_esm_and_text_encoders(tmp_path, monkeypatch):
    from oneprot_amd.encoders import SequenceEncoder, TextEncoder, StructEncoder
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    esm = _write(tmp_path, "esm", model_type="esm", vocab_size=33, hidden_size=40, num_hidden_layers=3, num_attention_heads=2, intermediate_size=80)
    with pytest.warns(UserWarning):
        enc = SequenceEncoder(esm, output_dim=16, use_lora=False, frozen=False)
    assert enc.set_activation_recompute(2) is enc
    assert enc.transformer.recompute_layers == 2 and enc.transformer._recompute_k() == 2
    with pytest.raises(ValueError):
        enc.set_activation_recompute(-1)
    assert enc.transformer.recompute_layers == 2             # a refused value changes nothing
    enc.set_activation_recompute(None)
    assert enc.transformer.recompute_layers is None
    bert = _write(tmp_path, "bert", model_type="bert", vocab_size=100, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                  max_position_embeddings=64, pad_token_id=0, layer_norm_eps=1e-12)
    with pytest.warns(UserWarning):
        txt = TextEncoder(bert, output_dim=16, frozen=True)
    monkeypatch.setenv("ONEPROT_RECOMPUTE_LAYERS", "2")      # the environment alone leaves a non-ESM tower untouched ...
    assert not hasattr(txt.transformer, "recompute_layers")
    with pytest.raises(NotImplementedError, match="text tower"):      # ... and asking for it by name is refused
        txt.set_activation_recompute(2)
    import torch
    graph = StructEncoder(torch.nn.Linear(4, 16), output_dim=16)
    with pytest.raises(NotImplementedError, match="graph encoder"):
        graph.set_activation_recompute(2)


def test_counted_bytes_of_the_ab_tool():
    """tools/recompute_ab.py counts what esm.py allocates: 32 d + 16 + 4 H bytes per token and layer, 6 d + 8 per boundary record"""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("recompute_ab", os.path.join(root, "tools", "recompute_ab.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    off = tool.activation_bytes(256 * 512, 640, 20, 30)                     # cfg-2: ESM-2-150M, 256 rows of 512
    assert off["per_layer"] == 20576 * 131072 and round(off["per_layer"] / 1e9, 2) == 2.70 and round(off["total"] / 1e9, 1) == 80.9
    big = tool.activation_bytes(256 * 1024, 1280, 20, 33)                   # ESM-2-650M, 256 rows of 1024
    assert round(big["total"] / 1e9) == 355 and big["total"] > tool.DEVICE_BYTES
    for n, k in ((30, 3), (30, 6), (30, 10), (33, 3), (6, 4)):
        on = tool.activation_bytes(131072, 640, 20, n, k)
        plan = recompute_plan(n, k)
        assert on["boundaries"] == len(plan) - 1 and on["kept_layers"] == k
        assert on["total"] == k * on["per_layer"] + (len(plan) - 1) * on["per_boundary"] and on["per_boundary"] == (6 * 640 + 8) * 131072
        assert tool.extra_forward_share(n, k) == round(plan[-1][0] / n, 3)  # every layer below the top segment runs twice
    assert tool.activation_bytes(131072, 640, 20, 6, 9)["total"] == tool.activation_bytes(131072, 640, 20, 6)["total"] and tool.extra_forward_share(6, 9) == 0.0
