"""Embedding collection on the MI355X (oneprot_amd/collect.py): embed_sequences against the fp32 oracle and against the encoder called directly on the plan's
batches, its invariances, the esm2 baseline, ppi, the custom-model path against the reference's golden, and the chain CSV -> file -> load_data -> tree probe."""
import os
import random

import numpy as np
import pytest
import torch
import yaml

from oneprot_amd import collect as C
from oneprot_amd.msa_data import LETTERS
from oneprot_amd.packing import PackedTokens

pytestmark = pytest.mark.gpu

from oracle import oneprot_oracle as O  # noqa: E402
from tests.cases import esm_dir, golden_pair_module  # noqa: E402

DEV = "cuda"
MAX_TOKENS, MAX_SEQS = 2048, 8


def _letters(rng, n):
    return "".join(rng.choice("LAGVSERTIDPKQNFYMHWC") for _ in range(n))


def _sequence_set():
    """24 rows, 21 distinct: 0, 1, 125 .. 128, 509 .. 512 and 1 023 / 1 100 / 1 500 letters (1 024 tokens each), out-of-vocabulary letters, lower case and
    white space, three rows repeated"""
    rng = random.Random(1881)
    seqs = [_letters(rng, n) for n in (0, 1, 7, 30, 45, 60, 125, 126, 127, 128, 200, 300, 509, 510, 511, 512, 1023, 1100, 1500)]
    seqs += ["MK*J TA", "mkta"]
    seqs += [seqs[8], seqs[18], seqs[19]]
    rng.shuffle(seqs)
    return seqs


SEQS = _sequence_set()


@pytest.fixture(scope="module")
def env():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
        mp.setenv("RANK", "0")
        mp.setenv("WORLD_SIZE", "1")
        yield


def _encoder(tmp, pooling="mean", proj="mlp", layers=2, hidden=320, seed=0, **kw):
    from oneprot_amd.encoders import SequenceEncoder
    path = esm_dir(tmp, f"esm_{layers}x{hidden}", layers, hidden, 20, 4 * hidden)
    torch.manual_seed(seed)
    kw.setdefault("use_lora", False)
    return SequenceEncoder(path, output_dim=128, pooling_type=pooling, proj_type=proj, frozen=True, **kw).to(DEV).eval()


@pytest.fixture(scope="module")
def enc(env, tmp_path_factory):
    return _encoder(tmp_path_factory.mktemp("collect"))


@pytest.fixture(scope="module")
def plan():
    return C.plan_sequences(SEQS, 1024, MAX_TOKENS, MAX_SEQS)


@pytest.fixture(scope="module")
def base(enc):
    """embed_sequences of the shared set, once; the tests that read it leave it unchanged"""
    return C.embed_sequences(enc, SEQS, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)


def _oracle_cfg(e):
    c = e.config
    return dict(pad=c.pad_token_id, mask=c.mask_token_id, hidden=c.hidden_size, heads=c.num_attention_heads, layers=c.num_hidden_layers, eps=c.layer_norm_eps)


def _cpu_sd(e):
    return {k: v.detach().float().cpu() for k, v in e.state_dict().items()}


def _ids_of(plan, i):
    return torch.from_numpy(plan["flat"][plan["off"][i]:plan["off"][i + 1]].copy())


def _gate(got, ref, what):
    """the gate tests/test_packed_gpu.py holds this path to"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    cs = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    print(f"{what}: min row cosine {float(cs.min()):.6f}, max abs err {float((got - ref).abs().max()):.3e} of max |ref| {float(ref.abs().max()):.3e}")
    assert cs.min() > 0.999, (what, float(cs.min()))
    assert (got - ref).abs().max() < 0.05 * ref.abs().max(), what


def test_the_shared_plan_has_the_shapes_the_tests_need(plan):
    sizes = [[int(plan["off"][i + 1] - plan["off"][i]) for i in b] for b in plan["batches"]]
    assert len(plan["uniq"]) == 21 and len(SEQS) == 24
    assert len(sizes) >= 4 and [1024] in sizes and sum(sizes[-1]) < MAX_TOKENS
    assert any(len(b) == MAX_SEQS for b in sizes) and all(sum(b) <= MAX_TOKENS for b in sizes)
    assert {2, 3, 127, 128, 129, 130, 511, 512, 513, 514, 1024} <= {n for b in sizes for n in b}


# ------------------------------------------------------------------------------------------------------------------ 1. oneprot against the oracle
@pytest.mark.parametrize("pooling,proj,layers,hidden", [("mean", "linear", 2, 320), ("mean", "mlp", 2, 320), ("attention1d", "linear", 1, 1280),
                                                         ("attention1d", "mlp", 1, 1280)])
def test_oneprot_against_oracle(env, tmp_path, plan, pooling, proj, layers, hidden):
    """attention1d pooling is built for 1 280-wide towers only (as in the reference), so those cases run 1 layer x 1 280 x 20 heads"""
    e = _encoder(tmp_path, pooling, proj, layers, hidden, seed=3)
    got = C.embed_sequences(e, SEQS, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)
    assert got.shape == (len(SEQS), 128) and got.dtype == torch.float32 and got.is_cuda
    sd, cfg = _cpu_sd(e), _oracle_cfg(e)
    with torch.no_grad():
        ref = torch.cat([O.encoder_features("esm", _ids_of(plan, i)[None], sd, cfg, pooling, proj, False) for i in range(len(plan["uniq"]))])
    _gate(got, ref[torch.from_numpy(plan["inverse"])], f"{pooling}/{proj}")


# ------------------------------------------------------------------------------------------------------------------ 2. no arithmetic of its own
def test_rows_are_the_encoders_own_on_every_batch(enc, plan, base):
    assert len(plan["batches"]) >= 4
    row_of = {s: SEQS.index(s) for s in plan["uniq"]}
    for batch in plan["batches"]:
        p = PackedTokens.from_list([_ids_of(plan, i) for i in batch]).to(DEV)
        with torch.no_grad():
            direct = enc(p)
        mine = base[[row_of[plan["uniq"][i]] for i in batch]]
        assert torch.equal(mine, direct), [len(plan["uniq"][i]) for i in batch]


# ------------------------------------------------------------------------------------------------------------------ 3. invariance
def test_permutation_duplicates_and_repeat(enc, base):
    kept = base.clone()
    perm = list(range(len(SEQS)))
    random.Random(5).shuffle(perm)
    again = C.embed_sequences(enc, [SEQS[i] for i in perm], "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)
    assert torch.equal(again, base[perm])
    first = {}
    n_dup = 0
    for i, s in enumerate(SEQS):
        if s in first:
            n_dup += 1
            assert torch.equal(base[i], base[first[s]])
        first.setdefault(s, i)
    assert n_dup == 3
    assert torch.equal(C.embed_sequences(enc, SEQS, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS), base)
    more = C.embed_sequences(enc, SEQS + SEQS[:5], "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)          # more duplicates, the same plan
    assert torch.equal(more[:len(SEQS)], base) and torch.equal(more[len(SEQS):], base[:5])
    assert torch.equal(base, kept)


def test_training_flag_restored_and_lora_dropout_off(env, tmp_path):
    e = _encoder(tmp_path, "mean", "linear", seed=4, use_lora=True, lora_dropout=0.1)
    with torch.no_grad():
        e.transformer.lora_B.normal_(0.0, 0.05)                       # adapters that change the output: a dropout mask would show
    seqs = SEQS[:10]
    e.eval()
    in_eval = C.embed_sequences(e, seqs, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)
    assert not any(m.training for m in e.modules())
    e.train()
    flags = [m.training for m in e.modules()]
    in_train = C.embed_sequences(e, seqs, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)
    assert e.training and [m.training for m in e.modules()] == flags
    assert torch.equal(in_eval, in_train)
    with pytest.raises(ValueError):                                   # an error inside leaves the flags alone too
        C.embed_sequences(e, seqs, "oneprot", max_tokens=512)
    assert [m.training for m in e.modules()] == flags


# ------------------------------------------------------------------------------------------------------------------ 4. esm2 against the oracle
def _rel_l2_rows(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return (got - ref).norm(dim=1) / ref.norm(dim=1)


def _esm2_case(e, seqs, what):
    """new path: embed_sequences(kind="esm2"); parent's public path: transformer(padded ids).last_hidden_state, masked mean in fp64 on the host; both against the
    fp32 oracle's mean_pool(esm_forward) per sequence, in relative L2 per row"""
    p = C.plan_sequences(seqs, 1024, MAX_TOKENS, MAX_SEQS)
    sd, cfg = _cpu_sd(e), _oracle_cfg(e)
    with torch.no_grad():
        ref = torch.cat([O.mean_pool(O.esm_forward(_ids_of(p, i)[None], sd, cfg), torch.ones(1, int(p["off"][i + 1] - p["off"][i]), dtype=torch.long))
                         for i in range(len(p["uniq"]))])[torch.from_numpy(p["inverse"])]
        got = C.embed_sequences(e, seqs, "esm2", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS)
        padded = C.EsmSequenceTokenizer()(seqs).to(DEV)
        hidden = e.transformer(padded).last_hidden_state.double().cpu()
    mask = (padded != 1).double().cpu()[:, :, None]
    parent = (hidden * mask).sum(1) / mask.sum(1)
    assert got.shape == (len(seqs), e.config.hidden_size) and got.dtype == torch.float32 and got.is_cuda and torch.isfinite(got).all()
    err_new, err_parent = _rel_l2_rows(got, ref), _rel_l2_rows(parent, ref)
    print(f"{what}: relative L2 per row against the fp32 oracle: embed_sequences max {float(err_new.max()):.3e} mean {float(err_new.mean()):.3e}; "
          f"padded last_hidden_state + fp64 mean max {float(err_parent.max()):.3e} mean {float(err_parent.mean()):.3e}; "
          f"largest ratio new / parent {float((err_new / err_parent).max()):.3f}")
    assert (err_parent > 0).all() and (err_new <= 2 * err_parent).all(), (err_new / err_parent).tolist()


def test_esm2_against_oracle(enc):
    _esm2_case(enc, SEQS, "2 x 320")


def test_esm2_against_oracle_650m_shape(env, tmp_path):
    rng = random.Random(9)
    e = _encoder(tmp_path, "mean", None, 1, 1280, seed=6)
    _esm2_case(e, [_letters(rng, n) for n in (300, 509, 510, 511, 700)], "1 x 1280, head_dim 64")


# ------------------------------------------------------------------------------------------------------------------ 5. ppi
def test_ppi_halves(enc, tmp_path):
    rng = random.Random(2)
    prot = [_letters(rng, n) for n in (5, 40, 41, 130, 250, 300, 513, 600, 90, 17)]
    col1 = [prot[i % 10] for i in range(20)]
    col2 = [prot[(3 * i + 1) % 10] for i in range(20)]               # either column holds every protein: one plan for the pair and for each column
    labels = [i % 2 for i in range(20)]
    path = str(tmp_path / "normal_valid.csv")
    with open(path, "w") as f:
        f.write("sequence_1,sequence_2,label/fitness\n" + "".join(f"{a},{b},{y}\n" for a, b, y in zip(col1, col2, labels)))
    cfg = {"output_dir": str(tmp_path / "{model_name}"), "batch_size": 8, "single_batch_mode": True, "max_tokens": MAX_TOKENS, "max_seqs": MAX_SEQS,
           "tasks": {"HumanPPI": {"label_type": "ppi"}}}
    out = C.collect_task(cfg, {"name": "mine"}, "HumanPPI", path, both=True, model=(enc, "oneprot"))
    assert out == str(tmp_path / "mine" / "HumanPPI" / "valid" / "HumanPPI_valid_embeddings_labels.pt")
    both = torch.load(out, weights_only=True)
    assert both["embeddings"].shape == (20, 256) and both["embeddings"].dtype == torch.float32 and both["labels_fitness"].tolist() == labels
    assert sorted(os.listdir(os.path.dirname(out) + "/single_embs")) == [f"embeddings_rank0_batch{i}.pt" for i in range(3)]
    for half, col in ((both["embeddings"][:, :128], col1), (both["embeddings"][:, 128:], col2)):
        assert torch.equal(half, C.embed_sequences(enc, col, "oneprot", max_tokens=MAX_TOKENS, max_seqs=MAX_SEQS).cpu())


# ------------------------------------------------------------------------------------------------------------------ 6. custom-model path
def test_custom_model_path_against_reference_golden(env, golden_dir, tmp_path):
    g, module = golden_pair_module(golden_dir, "hd16", tmp_path)
    c = g["cfg"]
    ckpt = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in module.state_dict().items()}, "global_step": 0}, ckpt)
    del module
    tower = os.path.join(str(tmp_path), "esm")                       # the directory golden_pair_module built the towers from
    head = dict(model_name_or_path=tower, output_dim=c["output_dim"], pooling_type="mean")
    model = {"_target_": "src.models.oneprot_module.OneProtLitModule",
             "components": {"sequence": {"_target_": "src.models.components.sequence_encoder.SequenceEncoder", **head, "proj_type": "mlp", "use_lora": False,
                                         "frozen": False},
                            "struct_token": {"_target_": "src.models.components.struct_token_encoder.StructTokenEncoder", **head, "proj_type": "linear",
                                             "use_logit_scale": True, "learnable_logit_scale": False}},
             "optimizer": {"_target_": "oneprot_amd.optim.FusedAdam", "_partial_": True, "lr": 1e-3, "weight_decay": 0.0},
             "loss_fn": "CLIP", "use_l1_regularization": True, "local_loss": True, "gather_with_grad": True}
    config_path = str(tmp_path / "run_config.yaml")
    with open(config_path, "w") as f:
        yaml.safe_dump({"model": model}, f)
    names = {0: "<cls>", 1: "<pad>", 2: "<eos>", 3: "<unk>", 31: "<null_1>", 32: "<mask>", **{4 + i: ch for i, ch in enumerate(LETTERS)}}
    seqs = ["".join(names[int(t)] for t in row[1:n - 1]) for row, n in zip(g["seq_ids"], c["lens"])]
    assert C.EsmSequenceTokenizer()(seqs).tolist() == g["seq_ids"].tolist() and any("<mask>" in s for s in seqs)
    encoder, kind = C.load_model({"huggingface": False}, {"name": "awesome_model", "ckpt_path": ckpt, "config_path": config_path})
    assert kind == "oneprot" and not encoder.training
    got = C.embed_sequences(encoder, seqs, kind)
    _gate(got, g["sequence_features"], "custom model, golden hd16")
    # huggingface: true -- the same weights as a plain state dict
    plain = str(tmp_path / "plain.pt")
    torch.save(torch.load(ckpt, weights_only=True)["state_dict"], plain)
    encoder2, _ = C.load_model({"huggingface": True}, {"name": "awesome_model", "ckpt_path": plain, "config_path": config_path})
    assert torch.equal(C.embed_sequences(encoder2, seqs, "oneprot"), got)


# ------------------------------------------------------------------------------------------------------------------ 7. the chain
def test_csv_to_tree_probe_chain(env, tmp_path):
    from oneprot_amd import downstream
    from oneprot_amd.gbt import XGBClassifier
    rng = random.Random(11)
    tower = esm_dir(tmp_path, "esm2_tower", 2, 320, 20, 1280)
    csvs = []
    for split in ("train", "valid", "test"):
        path = str(tmp_path / f"AF2_normal_{split}.csv")
        with open(path, "w") as f:
            f.write("name,sequence,label/fitness\n" + "".join(f"p{i},{_letters(rng, rng.randint(20, 300))},{i % 2}\n" for i in range(12)))
        csvs.append(path)
    config = str(tmp_path / "collect.yaml")
    with open(config, "w") as f:
        yaml.safe_dump({"models": [{"name": "esm2"}], "tasks": {"MetalIonBinding": {"label_type": "classification", "csv_files": csvs}}, "esm_model": tower,
                        "tokenizer_name": "facebook/esm2_t33_650M_UR50D", "saprot_model": "unused", "output_dir": str(tmp_path / "emb") + "/{model_name}",
                        "batch_size": 5, "single_batch_mode": False, "huggingface": False, "num_workers": 16, "num_gpus": 4, "num_nodes": 2}, f)
    written = C.main(["--config", config, "--run", f"max_tokens={MAX_TOKENS}"])
    assert len(written) == 3 and all(os.path.isfile(p) for p in written)
    data = downstream.load_data({"emb_dir": str(tmp_path / "emb"), "model_type": "esm2", "task_name": "MetalIonBinding",
                                 "evaluate_on": ["train", "valid", "test"], "threshold": float("-inf")})
    for split in ("train", "valid", "test"):
        assert data[f"{split}_emb"].shape == (12, 320) and data[f"{split}_emb"].dtype == np.float32 and np.isfinite(data[f"{split}_emb"]).all()
        assert data[f"{split}_target"].tolist() == [i % 2 for i in range(12)]
    model = XGBClassifier(max_depth=2, n_estimators=3, objective="binary:logistic")
    model.fit(data["train_emb"], data["train_target"])
    for split in ("valid", "test"):
        pred = model.predict(data[f"{split}_emb"])
        assert tuple(pred.shape) == (12,) and bool(torch.isfinite(pred.float()).all()) and set(pred.tolist()) <= {0, 1}
