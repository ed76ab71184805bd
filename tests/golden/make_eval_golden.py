"""Writes tests/golden/eval_table.pt from the reference's own evaluation functions:

    python tests/golden/make_eval_golden.py <reference checkout>/src/eval.py

The reference module is loaded by file with stand-in modules for what it imports but `calculate_retrieval_metrics` and `write_results_to_csv` never touch
(pytorch_lightning, omegaconf, hydra, esm, torch_geometric, transformers, pyrootutils, h5py, its own src.* helpers, and pandas where it is not installed);
sklearn's cosine_similarity is the real one.  Three modalities x N = 520 x D = 8 fp32: a shared latent plus noise of different strength per modality, so that
R@1 lies strictly between 0.05 and 0.9 for every pair and direction.  Rows whose matching similarity has a candidate within 1e-5 (fp64) in any pair and
direction get their noise redrawn until none is left, so that no rank can depend on the summation order or the precision of the similarity.  Recorded: the
inputs, the dict the reference's calculate_retrieval_metrics returns (as plain ints and floats) and the exact bytes its write_results_to_csv wrote.

Also recorded (pandas is needed): the bytes that save_results_to_csv of <reference checkout>/src/utils/downstream.py, loaded the same way, wrote for two calls
on one file (header + row, then an appended row) with the results and config kept beside them."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

N, D, MARGIN = 520, 8, 1e-5
NOISE = {"sequence": 0.25, "text": 0.6, "pocket": 0.9}


def load_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    anything = type("Anything", (), {"__init__": lambda self, *a, **k: None})
    stub("pytorch_lightning", LightningModule=torch.nn.Module)
    stub("omegaconf", DictConfig=dict, OmegaConf=anything)
    stub("hydra", main=lambda **kw: (lambda fn: fn))
    stub("esm")
    stub("torch_geometric")
    stub("torch_geometric.data", Batch=anything, Data=anything)
    stub("transformers", AutoTokenizer=anything)
    stub("pyrootutils", setup_root=lambda *a, **k: None)
    stub("h5py")
    try:
        import pandas  # noqa: F401
    except ImportError:
        stub("pandas")
    src = stub("src")
    src.utils = stub("src.utils", task_wrapper=None, instantiate_callbacks=None, instantiate_loggers=None, log_hyperparameters=None, extras=None, get_pylogger=None)
    stub("src.data")
    stub("src.data.utils")
    stub("src.data.utils.msa_utils", read_msa=None, filter_and_create_msa_file_list=None, greedy_select=None)
    stub("src.data.utils.struct_graph_utils", protein_to_graph=None)
    spec = importlib.util.spec_from_file_location("reference_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Cfg(dict):
    """a mapping with attribute access, what the reference reads its DictConfig as"""
    __getattr__ = dict.__getitem__


SAVE_RESULTS = [{"val_acc": 0.91234, "test_acc": 0.8, "test_f1_max": np.float64(0.61449), "n_test": 312, "note": "first"},
                {"val_acc": 1, "test_acc": np.float32(0.25), "test_f1_max": 0.5, "n_test": 7, "note": "second, with a comma"}]
SAVE_CFG = {"model_type": "oneprot", "task_name": "EC", "threshold": 0.3, "downstream_model": {"_target_": "x.Y", "name": "xgboost_cls", "max_depth": 6, "eta": 0.05,
                                                                                              "objective": "binary:logistic"}}


def saved_results_bytes(eval_path):
    path = os.path.join(os.path.dirname(eval_path), "utils", "downstream.py")
    spec = importlib.util.spec_from_file_location("reference_downstream", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as tmp:
        cfg = Cfg(SAVE_CFG, results_dir=tmp, downstream_model=Cfg(SAVE_CFG["downstream_model"]))
        for results in SAVE_RESULTS:
            mod.save_results_to_csv(dict(results), cfg)
        with open(os.path.join(tmp, "downstream_results", "EC_xgboost_cls_results.csv"), "rb") as f:
            return f.read()


def close_rows(embeddings):
    """rows that have, in some pair and direction, a candidate within MARGIN of their matching cosine similarity (fp64)"""
    unit = {k: v.double().numpy() / np.linalg.norm(v.double().numpy(), axis=1, keepdims=True) for k, v in embeddings.items()}
    names, bad = list(unit), set()
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            sim = unit[names[a]] @ unit[names[b]].T
            d = np.diag(sim).copy()
            for gap in (np.abs(sim - d[:, None]), np.abs(sim - d[None, :]).T):
                np.fill_diagonal(gap, np.inf)
                bad |= set(np.flatnonzero(gap.min(axis=1) <= MARGIN).tolist())
    return sorted(bad)


def main():
    ref = load_reference(sys.argv[1])
    gen = torch.Generator().manual_seed(2025)
    latent = torch.randn(N, D, generator=gen)
    embeddings = {name: latent + s * torch.randn(N, D, generator=gen) for name, s in NOISE.items()}
    for _ in range(100):
        bad = close_rows(embeddings)
        if not bad:
            break
        for name, s in NOISE.items():
            embeddings[name][bad] = latent[bad] + s * torch.randn(len(bad), D, generator=gen)
    assert not close_rows(embeddings)
    results = ref.calculate_retrieval_metrics({k: v.numpy() for k, v in embeddings.items()})
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "retrieval_metrics.csv")
        ref.write_results_to_csv(results, path)
        with open(path, "rb") as f:
            csv_bytes = f.read()
    plain = {pair: {k: (int(v) if k.endswith("median_rank") else float(v)) for k, v in m.items()} for pair, m in results.items()}
    for pair, m in plain.items():
        for d in ("seq_to_mod", "mod_to_seq"):
            assert 0.05 < m[f"{d}_R@1"] < 0.9, (pair, d, m[f"{d}_R@1"])
            assert isinstance(results[pair][f"{d}_median_rank"], int)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_table.pt")
    torch.save({"embeddings": embeddings, "results": plain, "csv": csv_bytes, "margin": MARGIN,
                "save_results": {"results": SAVE_RESULTS, "cfg": SAVE_CFG, "csv": saved_results_bytes(sys.argv[1])}}, out)
    print(f"{out}: {os.path.getsize(out)} bytes")
    print(csv_bytes.decode())


if __name__ == "__main__":
    main()
