"""Cross-modal evaluation on the MI355X (oneprot_amd/evaluate.py): the reference's golden table, embed_modalities against the towers called directly on its
own batches and against the reference's 50-row loop, duplicates and ties, and main end to end from a config file and a checkpoint."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from oneprot_amd import evaluate as E, hip, retrieval
from oneprot_amd.graph_data import featurize_batch
from oneprot_amd.packing import PackedTokens
from tests.cases import esm_dir
from tests.eval_cases import VOCAB, build_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUDGET = dict(max_tokens=2048, max_seqs=4, max_graphs=8)
# 23 rows.  Sequences: 1, 7, 126 .. 129, 510 .. 513 letters and 1 100 (cut at max_sequence_length 1 024); rows 20 and 21 share row 2's text, row 22 shares
# row 3's sequence; row 12 has no pocket.  Graphs of 2 .. 120 residues.
SEQ_LENS = [1, 7, 126, 127, 128, 129, 510, 511, 512, 513, 1100, 30, 45, 60, 200, 300, 250, 90, 17, 400, 33, 64, 127]
TEXT_WORDS = [1, 4, 12, 30, 7, 60, 200, 3, 25, 9, 400, 15, 2, 44, 80, 5, 18, 33, 6, 120, 12, 12, 21]
STRUCT_LENS = [2, 9, 140, 127, 300, 64, 510, 33, 1100, 12, 700, 20, 45, 61, 210, 8, 254, 95, 19, 380, 31, 66, 128]
GRAPH_SIZES = [2, 5, 120, 37, 64, 9, 100, 3, 77, 50, 118, 21, 33, 12, 90, 6, 45, 70, 15, 110, 28, 8, 59]
POCKET_SIZES = [3, 100, 41, 2, 17, 88, 100, 64, 9, 30, 120, 5, 72, 26, 100, 13, 55, 34, 7, 99, 46, 11, 80]
MISSING = 12


def _gate(got, ref, what):
    """the gate of tests/test_collect_gpu.py::_gate, which is tests/test_packed_gpu.py's"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    cs = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    print(f"{what}: min row cosine {float(cs.min()):.6f}, max abs err {float((got - ref).abs().max()):.3e} of max |ref| {float(ref.abs().max()):.3e}")
    assert cs.min() > 0.999, (what, float(cs.min()))
    assert (got - ref).abs().max() < 0.05 * ref.abs().max(), what


@pytest.fixture(scope="module", autouse=True)
def tower_numbering():
    """This module builds a dozen towers.  Towers are numbered in construction order per process (oneprot_amd/rng.py) and ProNet's dropout seed is
    FIXED_SEED + that number, so the modules that run after this one would otherwise draw other masks than they do without it
    (tests/test_pronet_gpu.py::test_through_the_module_as_pocket trains eight steps on them).  The numbering is put back where this module found it."""
    import itertools
    from oneprot_amd import rng
    start = next(rng._uids)
    rng._uids = itertools.count(start)
    yield
    rng._uids = itertools.count(start)


@pytest.fixture(scope="module")
def env():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
        mp.setenv("RANK", "0")
        mp.setenv("WORLD_SIZE", "1")
        yield


@pytest.fixture(scope="module")
def golden(golden_dir):
    return torch.load(os.path.join(golden_dir, "eval_table.pt"), weights_only=False)


def _model_node(tmp):
    """2 layers x 320 ESM towers (sequence; struct_token over the 54-id vocabulary), a 2-layer BERT, ProNet h = 64 with one block for both graph modalities"""
    esm = esm_dir(tmp, "esm", 2, 320, 20, 1280)
    bert = os.path.join(str(tmp), "bert")
    os.makedirs(bert, exist_ok=True)
    with open(os.path.join(bert, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=len(VOCAB), hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                       max_position_embeddings=512, pad_token_id=0), f)
    enc = "src.models.components."
    graph = lambda: {"_target_": enc + "struct_graph_encoder.StructEncoder", "output_dim": 128, "proj_type": "linear", "use_logit_scale": True,
                     "encoder": {"_target_": "oneprot_amd.pronet.ProNet", "level": "backbone", "num_blocks": 1, "hidden_channels": 64, "out_channels": 128}}
    return {"_target_": "src.models.oneprot_module.OneProtLitModule", "loss_fn": "CLIP",
            "optimizer": {"_target_": "oneprot_amd.optim.FusedAdam", "_partial_": True, "lr": 1e-3},
            "components": {"sequence": {"_target_": enc + "sequence_encoder.SequenceEncoder", "model_name_or_path": esm, "output_dim": 128, "pooling_type": "mean",
                                        "proj_type": "mlp", "use_lora": False, "frozen": True},
                           "struct_token": {"_target_": enc + "struct_token_encoder.StructTokenEncoder", "model_name_or_path": esm, "output_dim": 128,
                                            "pooling_type": "mean", "proj_type": "linear", "use_logit_scale": True},
                           "text": {"_target_": enc + "text_encoder.TextEncoder", "model_name_or_path": bert, "output_dim": 128, "pooling_type": "mean",
                                    "proj_type": "linear", "use_logit_scale": True, "frozen": True, "use_lora": False},
                           "struct_graph": graph(), "pocket": graph()}}


@pytest.fixture(scope="module")
def setup(env, tmp_path_factory):
    from oneprot_amd import config as config_mod
    tmp = tmp_path_factory.mktemp("eval_gpu")
    case = build_table(tmp, SEQ_LENS, TEXT_WORDS, STRUCT_LENS, GRAPH_SIZES, POCKET_SIZES, same_text=[(2, 20, 21)], same_seq=[(3, 22)], missing_pocket=(MISSING,))
    node = _model_node(tmp)
    torch.manual_seed(1881)
    model = config_mod.instantiate(node).to(DEV).eval()
    ds = E.CombinedDataset(case["cfg"], struct_file=case["struct_file"], pocket_file=case["pocket_file"])
    ds.device = torch.device(DEV, torch.cuda.current_device())
    return dict(tmp=tmp, case=case, node=node, model=model, ds=ds)


@pytest.fixture(scope="module")
def base(setup):
    """embed_modalities of the shared table under the small budgets, once; the tests that read it leave it unchanged"""
    return E.embed_modalities(setup["model"], setup["ds"], **BUDGET)


# ------------------------------------------------------------------------------------------------------------------ the golden
def test_golden_table_and_file(golden, tmp_path):
    dev = {k: v.to(DEV) for k, v in golden["embeddings"].items()}
    got = E.calculate_retrieval_metrics(dev)
    assert dict(got) == golden["results"] and not got.any_ties and set(got.tie_rows.values()) == {(0, 0)}
    assert all(isinstance(m[k], int) for m in got.values() for k in m if k.endswith("median_rank"))
    path = tmp_path / "retrieval_metrics.csv"
    E.write_results_to_csv(got, str(path))
    assert path.read_bytes() == golden["csv"]
    assert dict(E.calculate_retrieval_metrics({k: v.numpy() for k, v in golden["embeddings"].items()})) == golden["results"]       # host arrays are copied over
    assert dict(E.calculate_retrieval_metrics(dev, bound="pessimistic")) == golden["results"]                                      # no ties: the same table


# ------------------------------------------------------------------------------------------------------------------ no arithmetic of its own
def test_shapes_rows_and_budgets(setup, base):
    kept = setup["case"]["kept"]
    assert len(kept) == 22 and MISSING not in kept and base.ids == [f"r{k}" for k in kept]
    assert list(base) == list(E.MODALITIES)
    for name, x in base.items():
        assert x.shape == (22, 128) and x.dtype == torch.float32 and x.is_cuda and torch.isfinite(x).all(), name


def _token_plan(ds, rows, name):
    if name == "text":
        return E.plan_tokens(rows[name], ds.text_tokenizer.encode_all, ds.text_max_length, BUDGET["max_tokens"], BUDGET["max_seqs"], pad_id=0)
    tok = ds.sequence_tokenizer if name == "sequence" else ds.structure_tokenizer
    return E.plan_tokens(rows[name], tok.encode_all, ds.max_sequence_length, BUDGET["max_tokens"], BUDGET["max_seqs"], pad_id=1)


@pytest.mark.parametrize("name", E.TOKEN_MODALITIES)
def test_token_rows_are_the_towers_own_on_every_plan_batch(setup, base, name):
    ds, model = setup["ds"], setup["model"]
    rows = ds.resolve(ds.data, records=True)
    plan = _token_plan(ds, rows, name)
    assert len(plan["batches"]) >= 4
    if name == "sequence":
        assert int(np.diff(plan["off"]).max()) == 1024 and {3, 128, 129, 130, 131, 512, 513, 514, 515} <= set(np.diff(plan["off"]).tolist())
    first = {}
    for r, i in enumerate(plan["inverse"].tolist()):
        first.setdefault(i, r)
    for batch in plan["batches"]:
        ids = [torch.from_numpy(plan["flat"][plan["off"][i]:plan["off"][i + 1]].copy()) for i in batch]
        p = PackedTokens.from_list(ids, pad_id=plan["pad_id"]).to(DEV)
        with torch.no_grad():
            direct = model.network[name](p)
        assert torch.equal(base[name][[first[i] for i in batch]], direct), (name, [len(t) for t in ids])


@pytest.mark.parametrize("name", E.GRAPH_MODALITIES)
def test_graph_rows_are_the_towers_own_on_every_file_order_batch(setup, base, name):
    ds, model = setup["ds"], setup["model"]
    records = ds.resolve(ds.data, records=True)[name]
    plan = E.plan_graphs([len(r[0]) for r in records], BUDGET["max_graphs"])
    assert plan == [(0, 8), (8, 16), (16, 22)]
    for lo, hi in plan:
        with torch.no_grad():
            direct = model.network[name](featurize_batch(records[lo:hi], DEV))
        assert torch.equal(base[name][lo:hi], direct), (name, lo, hi)


# ------------------------------------------------------------------------------------------------------------------ against the 50-row loop
def test_against_the_fifty_row_loop(setup, base):
    ds, model = setup["ds"], setup["model"]
    batch = ds.collate_fn([ds[k] for k in range(len(ds))])
    assert batch["ids"] == base.ids and batch["sequence"].is_cuda and batch["text"].is_cuda and batch["pocket"].x.is_cuda
    loop = E.encode_inputs(model, batch)
    assert list(loop) == list(E.MODALITIES)
    for name in E.TOKEN_MODALITIES:
        _gate(base[name], loop[name], f"{name}: whole-dataset pass against the padded 50-row batch")
    whole = E.embed_modalities(model, ds, modalities=list(E.GRAPH_MODALITIES))          # max_nodes=None, max_graphs 50: the reference's composition
    for name in E.GRAPH_MODALITIES:
        assert torch.equal(whole[name], loop[name]), name


# ------------------------------------------------------------------------------------------------------------------ duplicates and ties
def _host_tables(emb):
    """both tables from a host count: l2norm as retrieval_table runs it, similarities from oneprot_sgemm, > and == counted in numpy"""
    feats = {}
    for name, x in emb.items():
        y, inv = torch.empty_like(x), torch.empty(x.shape[0], device=x.device)
        hip.call("oneprot_l2norm_fwd", x.contiguous(), y, inv, x.shape[0], x.shape[1], 1.0)
        feats[name] = y
    names, out, tied = list(feats), {"optimistic": {}, "pessimistic": {}}, {}
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            s, m = feats[names[a]], feats[names[b]]
            N, D = s.shape
            logits = torch.empty(N, N, device=s.device)
            hip.call("oneprot_sgemm", s, m, logits, N, N, D, 0, 0, 1.0, 0)
            sim = logits.cpu().numpy()
            d = np.diag(sim)
            rr, rc = (sim > d[:, None]).sum(1), (sim > d[None, :]).sum(0)
            tr, tc = (sim == d[:, None]).sum(1) - 1, (sim == d[None, :]).sum(0) - 1
            pair = f"{names[a]}-{names[b]}"
            for bound in out:
                m_ = retrieval.metrics_from_ranks(rr, rc, E.KS, ties=(tr, tc), bound=bound)
                out[bound][pair] = {k: int(v) if k.endswith("median_rank") else v for k, v in m_.items()}
            tied[pair] = (int((tr > 0).sum()), int((tc > 0).sum()))
    return out, tied


def test_duplicates_are_bit_identical_and_ties_show_in_the_pessimistic_table(setup, base):
    rows = {k: i for i, k in enumerate(setup["case"]["kept"])}
    assert torch.equal(base["text"][rows[2]], base["text"][rows[20]]) and torch.equal(base["text"][rows[2]], base["text"][rows[21]])
    assert torch.equal(base["sequence"][rows[3]], base["sequence"][rows[22]])
    assert not torch.equal(base["text"][rows[2]], base["text"][rows[3]])
    want, tied = _host_tables(base)
    opt, pes = E.calculate_retrieval_metrics(base), E.calculate_retrieval_metrics(base, bound="pessimistic")
    assert dict(opt) == want["optimistic"] and dict(pes) == want["pessimistic"]
    assert opt.tie_rows == tied == pes.tie_rows and opt.any_ties
    assert tied["sequence-text"][0] >= 3 and tied["sequence-text"][1] >= 2               # the three rows of one text; the two rows of one sequence
    differ = {(pair, k) for pair in opt for k in opt[pair] if opt[pair][k] != pes[pair][k]}
    assert differ == {(pair, k) for pair in want["optimistic"] for k in want["optimistic"][pair] if want["optimistic"][pair][k] != want["pessimistic"][pair][k]}
    assert all(pes[pair][k] <= opt[pair][k] for pair in opt for k in opt[pair] if "R@" in k)


# ------------------------------------------------------------------------------------------------------------------ flags, read-backs
def test_training_flags_are_restored_and_nothing_is_read_back_per_batch(setup, base, monkeypatch):
    ds, model = setup["ds"], setup["model"]
    model.train()
    flags = [m.training for m in model.modules()]
    try:
        again = E.embed_modalities(model, ds, modalities=["struct_token", "pocket"], **BUDGET)
        assert [m.training for m in model.modules()] == flags and model.training
        assert torch.equal(again["struct_token"], base["struct_token"]) and torch.equal(again["pocket"], base["pocket"])       # eval mode inside
        with pytest.raises(ValueError):
            E.embed_modalities(model, ds, modalities=["sequence"], max_tokens=512)
        assert [m.training for m in model.modules()] == flags
    finally:
        model.eval()
    calls = []
    for attr in ("cpu", "item", "tolist"):
        real = getattr(torch.Tensor, attr)
        monkeypatch.setattr(torch.Tensor, attr, lambda self, *a, _real=real, _attr=attr, **k: (calls.append(_attr) if self.is_cuda else None, _real(self, *a, **k))[1])
    counts = []
    for budget in (dict(max_tokens=2048, max_seqs=4), dict(max_tokens=4096, max_seqs=22)):
        calls.clear()
        out = E.embed_modalities(model, ds, modalities=["sequence", "text"], **budget)
        counts.append(list(calls))
        assert out["sequence"].is_cuda
    print(f"device read-backs of embed_modalities(sequence, text): {counts}")
    assert counts[0] == counts[1], "the number of read-backs follows the number of batches"
    assert len(counts[0]) <= 2                                   # the text ids and lengths of the whole set, once


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_main_from_a_config_file_and_a_checkpoint(setup, base, tmp_path, monkeypatch):
    from oneprot_amd.data import save_checkpoint
    case, model = setup["case"], setup["model"]
    run_config, ckpt, config = str(tmp_path / "run_config.yaml"), str(tmp_path / "best.ckpt"), str(tmp_path / "eval.yaml")
    with open(run_config, "w") as f:
        yaml.safe_dump({"model": setup["node"]}, f)
    save_checkpoint(model, ckpt)
    out_csv = str(tmp_path / "results" / "retrieval_metrics.csv")
    with open(config, "w") as f:
        yaml.safe_dump({**case["cfg"], "model": {"config_path": run_config, "ckpt_path": "unset"}, "output": {"csv_path": "unset"},
                        "hydra": {"run": {"dir": "outputs/${now:%Y-%m-%d}"}}}, f)
    real_dataset, seen = E.CombinedDataset, {}
    monkeypatch.setattr(E, "CombinedDataset", lambda cfg: real_dataset(cfg, struct_file=case["struct_file"], pocket_file=case["pocket_file"]))      # h5py is absent
    real_embed = E.embed_modalities
    monkeypatch.setattr(E, "embed_modalities", lambda *a, **k: seen.setdefault("emb", real_embed(*a, **k)))
    results = E.main(["--config", config, f"model.ckpt_path={ckpt}", f"output.csv_path={out_csv}", "dataloader.max_tokens=2048", "dataloader.max_seqs=4",
                      "dataloader.batch_size=8"])
    emb = seen["emb"]
    assert emb.ids == base.ids and f"r{MISSING}" not in emb.ids
    for name in E.MODALITIES:
        assert emb[name].is_cuda and torch.equal(emb[name], base[name]), name          # the checkpoint's weights, the same plan
    want = tmp_path / "want.csv"
    E.write_results_to_csv(E.calculate_retrieval_metrics(base), str(want))
    with open(out_csv, "rb") as f:
        assert f.read() == want.read_bytes()
    assert dict(results) == dict(E.calculate_retrieval_metrics(base))
    E.write_results_to_csv(E.calculate_retrieval_metrics(base, bound="pessimistic"), str(want))
    with open(E.pessimistic_path(out_csv), "rb") as f:
        assert f.read() == want.read_bytes()


def test_no_pessimistic_file_for_a_table_without_duplicates(setup, tmp_path):
    case = build_table(tmp_path, [5, 40, 41, 130, 17, 64], [3, 9, 14, 2, 30, 6], [4, 30, 41, 120, 20, 60], [4, 20, 9, 33, 12, 7], [6, 10, 3, 25, 14, 8], seed=7)
    ds = E.CombinedDataset(case["cfg"], struct_file=case["struct_file"], pocket_file=case["pocket_file"])
    ds.device = setup["ds"].device
    results, emb = E.evaluate(case["cfg"], model=setup["model"], dataset=ds)
    out = case["cfg"]["output"]["csv_path"]
    assert os.path.isfile(out) and not os.path.exists(E.pessimistic_path(out)) and not results.any_ties
    assert len(emb.ids) == 6 and len(results) == 10
