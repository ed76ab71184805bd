"""The host side of the MLP probe (oneprot_amd/probe.py) without a GPU: state-dict parity with the reference's class (tests/golden/probe_mlp.pt, written by
tests/golden/make_probe_golden.py from the reference's own MLP), the restatement tests/probe_ref.py against the same golden, the plateau schedule against
torch's ReduceLROnPlateau, the stopping and best-epoch rules on hand-made sequences, the task tables, the refusals, and the derived ctypes signatures."""
import math
import os

import pytest
import torch

from oneprot_amd import hip, probe
from tests import probe_ref as R
from tests.gate import rel_l2
from tests.probe_cases import GOLDEN, make

U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, map_location="cpu", weights_only=False)


def test_state_dict_names_and_shapes_equal_the_reference(golden):
    assert len(golden["configs"]) == 27
    for cfg in golden["configs"]:
        m = make(cfg, golden)
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == cfg["names"], cfg
        assert list(m.state_dict()) == list(cfg["names"])                                    # the order too
        m.load_state_dict(cfg["state_dict"], strict=True)
        assert all(torch.equal(v, cfg["state_dict"][k]) for k, v in m.state_dict().items())
        assert ("residual_projection.weight" in cfg["names"]) == (cfg["residual"] == "projected")
        arena = m.arena()                                                                    # every parameter is a view of the one flat tensor, in order
        assert arena.numel() == sum(p.numel() for p in m.parameters()) and arena.grad.shape == arena.shape
        off = 0
        for p in m.parameters():
            assert p.data_ptr() == arena.data_ptr() + 4 * off
            off += p.numel()
    with_dropout = probe.MLP(24, 5, [16, 8], 0.25, True, False, "relu", False)
    assert {k: tuple(v.shape) for k, v in with_dropout.state_dict().items()} == golden["dropout_names"]
    assert [k for k in golden["dropout_names"] if k.startswith("hidden_layers")][0::7][:2] == ["hidden_layers.0.weight", "hidden_layers.4.weight"]
    both = probe.MLP(24, 5, [16], 0.0, True, True, "relu", False)                            # both flags: BatchNorm wins
    assert "hidden_layers.1.running_mean" in both.state_dict()
    with pytest.raises(ValueError, match="activation"):
        probe.MLP(24, 5, [16], activation="tanh")


def test_restatement_reproduces_the_reference_class(golden):
    """tests/probe_ref.py in fp64 against the values the reference's class computed with torch's fp32 CPU kernels.  The fp64 run is exact to ~1e-15, so the
    difference IS the fp32 run's rounding, and the bound is that rounding's worst case with no allowance on top: u = 2^-24; an output is a chain of at most three
    contractions of total length K = 24 + 16 + 8 = 48 and at most c = 16 elementwise roundings (bias, the norm's five, the activation, the residual sum, the
    loss), each dot product within gamma_n = n u / (1 - n u) of sum |a| |w|.  Forward values (outputs, losses, BatchNorm buffers): rel L2 <= (K + c) u = 64 u =
    3.8e-6.  Gradients run the chain twice: 128 u = 7.6e-6.  Three AdamW steps of lr 1e-3 each move a weight by at most lr and inherit the gradient's relative
    error, 3e-3 * 128 u = 2.3e-8 absolute on tensors whose rms is >= 0.07 (nn.Linear's init at fan-in <= 24, norm weights ~1, norm biases ~0.1), plus the fp32
    rounding u of the stored weight: rel L2 <= 2.3e-8 / 0.07 + u = 3.9e-7.  A restatement with another eps (1e-6 for 1e-5 moves rstd by 4.5e-6 / var, 1.5e-5 at
    these variances) or the tanh form of GELU (3e-4) is outside them.  The largest figure of each class is printed (-s): 2.0e-7, 6.5e-7, 1.4e-7."""
    fwd_tol, grad_tol, adam_tol = 64 * U, 128 * U, 3e-3 * 128 * U / 0.07 + U
    x, worst = golden["x"], {"fwd": 0.0, "grad": 0.0, "adamw": 0.0}
    for cfg in golden["configs"]:
        sp = R.spec(cfg["hidden_dims"], cfg["norm"], cfg["activation"], cfg["use_residual"])
        sd = cfg["state_dict"]
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        with torch.no_grad():
            out_eval, _ = R.forward(sd64, x.double(), sp, False)
            out_train, nb = R.forward(sd64, x.double(), sp, True)
        fw = [rel_l2(out_eval, cfg["out_eval"]), rel_l2(out_train, cfg["out_train"])]
        assert set(nb) == set(cfg["buffers_after"])
        for k, v in cfg["buffers_after"].items():
            if k.endswith("num_batches_tracked"):
                assert int(nb[k]) == int(v) == 1
            else:
                fw.append(rel_l2(nb[k], v))
        for kind in (0, 1, 2):
            _, ls, grads, _ = R.loss_and_grads(sd, x, golden["targets"][kind], sp, kind, True)
            fw.append(rel_l2(ls, cfg["loss"][kind]))
            assert set(grads) == set(cfg["grads"][kind])
            gold = cfg["grads"][kind]
            # the bias of a Linear that feeds a BatchNorm has the exact gradient 0 (the norm subtracts the column mean): fp32 leaves rounding noise there, which
            # has no relative error; it is measured against the norm of the same layer's weight gradient
            zero = {f"hidden_layers.{lin}.bias": f"hidden_layers.{lin}.weight" for lin, _ in R.layer_names(sp)} if cfg["norm"] == "batch" else {}
            gr = max(float((grads[k].double() - gold[k].double()).norm() / gold[zero[k]].double().norm()) if k in zero else rel_l2(grads[k], gold[k]) for k in grads)
            worst["grad"] = max(worst["grad"], gr)
            assert gr <= grad_tol, (cfg["norm"], cfg["activation"], cfg["residual"], kind, gr)
        worst["fwd"] = max(worst["fwd"], *fw)
        assert max(fw) <= fwd_tol, (cfg["norm"], cfg["activation"], cfg["residual"], fw)
        cur = {k: v.double() for k, v in sd.items() if R.is_param(k)}
        m, v2 = {k: torch.zeros_like(t) for k, t in cur.items()}, {k: torch.zeros_like(t) for k, t in cur.items()}
        state = dict(sd64)
        for step in (1, 2, 3):
            _, _, grads, nb = R.loss_and_grads(state, x, golden["targets"][0], sp, 0, True)
            for k in cur:
                cur[k], m[k], v2[k] = R.adamw_step(cur[k], grads[k], m[k], v2[k], step, 1e-3)
            state.update(cur)
            state.update(nb)
        # Adam divides a gradient by its own magnitude, so the rounding noise in the exactly-zero gradient of a bias in front of a BatchNorm moves that bias by
        # up to lr per step in fp32 and not at all in fp64: there only that bound holds (the bias cancels in the norm, nothing else sees it)
        for k in zero:
            assert float((cur[k] - cfg["adamw3"][k].double()).abs().max()) <= 1.1 * 3 * 1e-3, k
        ad = max(rel_l2(cur[k], cfg["adamw3"][k]) for k in cur if k not in zero)
        worst["adamw"] = max(worst["adamw"], ad)
        assert ad <= adam_tol, (cfg["norm"], cfg["activation"], cfg["residual"], ad)
    print(f"probe_ref fp64 vs the reference's fp32: forward {worst['fwd']:.3e} (bound {fwd_tol:.3e})  gradients {worst['grad']:.3e} ({grad_tol:.3e})  "
          f"AdamW x 3 {worst['adamw']:.3e} ({adam_tol:.3e})")


def _sequences():
    gen = torch.Generator().manual_seed(60)
    walk = (1.0 + 0.02 * torch.randn(60, generator=gen)).cumsum(0).flip(0) / 30                # falls, noisily
    plateaus = torch.cat([torch.linspace(2.0, 1.0, 8), torch.full((14,), 1.0) + 1e-5 * torch.randn(14, generator=gen), torch.linspace(1.0, 0.9, 5),
                          0.9 + 0.01 * torch.rand(33, generator=gen)])
    repeats = torch.tensor([0.7] * 25 + [0.69995] * 20 + [0.5] * 15)                            # exact repeats; 0.69995 is inside the relative threshold of 0.7
    with_nan = plateaus.clone()
    with_nan[20] = float("nan")
    rising = torch.linspace(0.5, 3.0, 60)
    return {"walk": walk, "plateaus": plateaus, "repeats": repeats, "nan": with_nan, "rising": rising}


@pytest.mark.parametrize("name", ["walk", "plateaus", "repeats", "nan", "rising"])
@pytest.mark.parametrize("lr", [1e-3, 1e-2])
def test_plateau_schedule_equals_torch(name, lr):
    losses = [float(v) for v in _sequences()[name]]
    assert len(losses) == 60
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=lr)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.1, patience=10)
    ours = probe.PlateauSchedule(lr)
    for v in losses:
        ref.step(v)
        assert ours.step(v) == opt.param_groups[0]["lr"]
    if name in ("repeats", "rising", "plateaus", "nan"):
        assert ours.lr < lr                                                                    # the sequence does reach a reduction


def test_early_stopping_and_best_epoch_rules():
    nan, inf = float("nan"), float("inf")
    # a tie for the best: the first among equals is kept; patience reached exactly: [.., best, worse, worse] with patience 2 stops after the second
    lrs, best, ran = probe.run_schedule([0.9, 0.5, 0.7, 0.5, 0.8, 0.4], 1e-3, 2)
    assert (best, ran) == (1, 4)                                                               # 0.7, 0.5 (a tie is no improvement): wait reaches 2 at epoch 3
    lrs, best, ran = probe.run_schedule([0.9, 0.5, 0.7, 0.5, 0.8, 0.4], 1e-3, 3)
    assert (best, ran) == (1, 5)                                                               # stops one epoch before the improvement
    lrs, best, ran = probe.run_schedule([0.9, 0.5, 0.7, 0.5, 0.8, 0.4], 1e-3, 4)
    assert (best, ran) == (5, 6) and lrs == [1e-3] * 6                                         # improvement in the last epoch is kept
    assert probe.run_schedule([0.5, 0.5, 0.5], 1e-3, 20)[1:] == (0, 3)
    assert probe.run_schedule([0.9, nan, 0.1], 1e-3, 20)[1:] == (0, 2)                         # a non-finite loss stops the fit
    assert probe.run_schedule([0.9, inf, 0.1], 1e-3, 20)[1:] == (0, 2)
    assert probe.run_schedule([nan, 0.3], 1e-3, 20)[1:] == (0, 1)                              # the first epoch is always a checkpoint
    lrs, best, ran = probe.run_schedule([1.0] * 30, 1e-2, 100)                                 # the plateau rule inside a fit: 11 bad epochs after the first
    assert ran == 30 and best == 0 and lrs[:12] == [1e-2] * 12 and lrs[12] == pytest.approx(1e-3) and lrs[23] == pytest.approx(1e-4)
    stop = probe.EarlyStopping(1)
    assert [stop.step(v) for v in (1.0, 0.9, 0.9)] == [False, False, True]


def test_task_dims_table():
    out = {"MetalIonBinding": 1, "DeepLoc2": 1, "HumanPPI": 1, "ThermoStability": 1, "EC": 585, "GO-BP": 1943, "GO-MF": 489, "GO-CC": 320, "DeepLoc10": 10, "TopEnzyme": 826}
    bce = {"MetalIonBinding", "DeepLoc2", "HumanPPI", "EC", "GO-BP", "GO-MF", "GO-CC"}
    widths = {"esm2": 1280, "saprot": 1280, "oneprot_9": 256, "oneprot_15": 1280, "oneprot_16": 1280, "prottrans": 1024, "anything": 1024}
    for task, n in out.items():
        for model_type, width in widths.items():
            kind = hip.PROBE_LOSS_BCE if task in bce else hip.PROBE_LOSS_MSE if task == "ThermoStability" else hip.PROBE_LOSS_CE
            assert probe.task_dims(task, model_type) == (width * (2 if task == "HumanPPI" else 1), n, kind), (task, model_type)
    with pytest.raises(ValueError, match="Unknown task_name"):
        probe.task_dims("Stability", "esm2")
    import src.saprot_fit_mlp as S
    assert S.MLP is probe.MLP and S.fit is probe.fit and S.evaluate is probe.evaluate and S.task_dims is probe.task_dims


def test_refusals_need_no_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(hip, "lib", no_lib)
    kw = dict(learning_rate=1e-3, batch_size=8, max_epochs=1, early_stopping_patience=2)
    x, y = torch.randn(41, 24), torch.randint(0, 10, (41,))
    bn = probe.MLP(24, 10, [16], use_batch_norm=True)
    plain = probe.MLP(24, 10, [16])
    with pytest.raises(ValueError, match="tail batch of one row"):
        probe.fit(bn, "DeepLoc10", (x, y), (x, y), **kw)                                       # 41 % 8 == 1
    with pytest.raises(ValueError, match="at most 256"):
        probe.fit(bn, "DeepLoc10", (x[:40], y[:40]), (x, y), **{**kw, "batch_size": 257})
    with pytest.raises(ValueError, match="integer class labels"):
        probe.fit(plain, "DeepLoc10", (x, y.float()), (x, y), **kw)                            # dtype
    with pytest.raises(ValueError, match="integer class labels"):
        probe.fit(plain, "DeepLoc10", (x, y[:, None]), (x, y), **kw)                           # shape
    with pytest.raises(ValueError, match="41 embeddings and 40 targets"):
        probe.fit(plain, "DeepLoc10", (x, y[:40]), (x, y), **kw)
    with pytest.raises(ValueError, match="non-empty"):
        probe.fit(plain, "DeepLoc10", (x, y), (x[:0], y[:0]), **kw)                            # an empty partition
    with pytest.raises(ValueError, match="non-empty"):
        probe.fit(plain, "DeepLoc10", (x[:0], y[:0]), (x, y), **kw)
    with pytest.raises(ValueError, match="25 wide"):
        probe.fit(plain, "DeepLoc10", (torch.randn(41, 25), y), (x, y), **kw)
    with pytest.raises(ValueError, match="585 outputs"):
        probe.fit(plain, "EC", (x, y), (x, y), **kw)                                           # the model is not the task's
    ec = probe.MLP(24, 585, [16])
    with pytest.raises(ValueError, match=r"targets \[rows, 585\]"):
        probe.fit(ec, "EC", (x, torch.zeros(41, 584)), (x, torch.zeros(41, 585)), **kw)
    with pytest.raises(ValueError, match="one target per row"):
        probe.fit(probe.MLP(24, 1, [16]), "ThermoStability", (x, torch.zeros(41, 2)), (x, torch.zeros(41)), **kw)
    with pytest.raises(ValueError, match="Unknown task_name"):
        probe.fit(plain, "Stability", (x, y), (x, y), **kw)
    with pytest.raises(ValueError, match="non-empty"):
        probe.predict(plain, "DeepLoc10", x[:0])


def test_new_entry_points_are_declared():
    P, I, L64, F, SZ, U64 = hip.c_void_p, hip.c_int, hip.c_int64, hip.c_float, hip.c_size_t, hip.c_uint64
    assert (hip.PROBE_MAX_BATCH, hip.ABI_VERSION) == (256, 7)
    assert hip._SIGS["oneprot_probe_linear_fwd"] == (I, [P] * 14 + [I] * 5 + [F, U64, U64, P])
    assert hip._SIGS["oneprot_probe_rownorm_act_fwd"] == (I, [P] * 8 + [I, I, I, F, U64, U64, P])
    assert hip._SIGS["oneprot_probe_norm_act_bwd"] == (I, [P] * 9 + [I, I, I, I, F, U64, U64, P])
    assert hip._SIGS["oneprot_probe_rownorm_act_bwd"] == (I, [P] * 9 + [I, I, I, F, U64, U64, P])
    assert hip._SIGS["oneprot_probe_linear_bwd_w"] == (I, [P] * 5 + [I, I, I, P])
    assert hip._SIGS["oneprot_probe_linear_bwd_x"] == (I, [P] * 3 + [I, I, I, P])
    assert hip._SIGS["oneprot_probe_loss_workspace"] == (SZ, [])
    assert hip._SIGS["oneprot_probe_loss_fwd_bwd"] == (I, [P] * 7 + [I, I, I, F, P])
    assert hip._SIGS["oneprot_adamw_step"] == (I, [P] * 4 + [L64, F, F, F, F, F, I, P])
    assert hip._PTR_DTYPES["oneprot_probe_linear_fwd"] == "fifffffiffffff"                    # idx and resid_idx are int32
    assert hip._PTR_DTYPES["oneprot_probe_loss_fwd_bwd"] == "fflifbb"                         # labels int64, idx int32, the fp64 sum and the workspace as bytes
    assert len(hip._SIGS["oneprot_adam_step"][1]) == 13                                        # the L2 form is as it was


def test_launchers_hand_the_declared_tuples(monkeypatch):
    rec = []
    monkeypatch.setattr(hip, "call", lambda name, *args: rec.append((name,) + args))
    hip.probe_linear_fwd("x", "w", "b", 7, 16, 24, idx="i", y="y", norm=1, act=2, gamma="g", beta="be", rng=(0.25, 3, 9))
    assert rec[-1] == ("oneprot_probe_linear_fwd", "x", "i", "w", "b", None, "y", None, None, "g", "be", None, None, None, None, 7, 16, 24, 1, 2, 0.25, 3, 9)
    assert len(rec[-1]) - 1 == len(hip._SIGS["oneprot_probe_linear_fwd"][1]) - 1
    hip.probe_norm_act_bwd("dy", "z", "dz", 7, 16, act=1)
    assert rec[-1] == ("oneprot_probe_norm_act_bwd", "dy", "z", None, None, None, None, "dz", None, None, 7, 16, 0, 1, 0.0, 0, 0)
    hip.probe_rownorm_act_fwd("z", "g", "b", "y", 7, 16, act=3, mean="m", rstd="r")
    assert rec[-1] == ("oneprot_probe_rownorm_act_fwd", "z", "g", "b", "y", None, None, "m", "r", 7, 16, 3, 0.0, 0, 0)
    hip.probe_rownorm_act_bwd("dy", "z", "g", "b", "m", "r", "dz", 7, 16, dgamma="dg", dbeta="db")
    assert rec[-1] == ("oneprot_probe_rownorm_act_bwd", "dy", "z", "g", "b", "m", "r", "dz", "dg", "db", 7, 16, 0, 0.0, 0, 0)
    import re
    src = open(probe.__file__).read()                                                          # probe.py spells out no positional tuple of the wide entry points
    assert not re.search(r'"oneprot_probe_(linear_fwd|rownorm_act_fwd|norm_act_bwd|rownorm_act_bwd|loss_fwd_bwd)"', src)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_arena_survives_deepcopy_pickle_and_a_move_to_where_it_is():
    import copy
    import pickle
    m = probe.MLP(24, 5, [16, 8], 0.25, True, False, "relu", True)
    arena = m.arena()
    m.to("cpu")
    m.float()
    assert m.arena() is arena                                                                  # nothing moved: an optimiser built on arena() stays valid
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c.arena() is not arena and torch.equal(c.arena(), arena) and c._is_flat()
        assert [type(n).__name__ for _, n in c._plan] == ["BatchNorm1d", "BatchNorm1d"] and all(lin is c.hidden_layers[i] for (lin, _), i in zip(c._plan, (0, 4)))
        assert set(c._gview) == {id(p) for p in c.parameters()}
        with torch.no_grad():
            c.arena().add_(1.0)                                                                # the copy's parameters are views of the copy's arena, not of ours
        assert torch.equal(c.output_layer.bias, m.output_layer.bias + 1.0) and torch.equal(m.arena(), arena)
        assert list(c.state_dict()) == list(m.state_dict())


def test_load_data_reads_the_reference_layout(tmp_path):
    from oneprot_amd import downstream
    import src.utils.downstream as SU
    assert SU.load_data is downstream.load_data is probe.load_data
    gen = torch.Generator().manual_seed(4)
    want = {}
    for part, rows in (("train", 6), ("valid", 3), ("test", 2)):
        d = tmp_path / "esm2" / "EC" / part
        d.mkdir(parents=True)
        want[part] = (torch.randn(rows, 8, generator=gen), torch.randint(0, 2, (rows, 5), generator=gen))
        torch.save({"embeddings": want[part][0], "labels_fitness": want[part][1]}, d / f"EC_{part}_embeddings_labels.pt")
    cfg = {"evaluate_on": ["train", "valid", "test"], "emb_dir": str(tmp_path), "model_type": "esm2", "task_name": "EC", "threshold": float("inf")}
    out = downstream.load_data(cfg)
    assert sorted(out) == sorted(f"{p}_{k}" for p in want for k in ("emb", "target"))
    for part, (e, t) in want.items():
        assert (out[f"{part}_emb"] == e.numpy()).all() and (out[f"{part}_target"] == t.numpy()).all()
    out = downstream.load_data({**cfg, "threshold": 0.25, "evaluate_on": ["valid"]})         # a finite threshold binarises the embeddings
    assert sorted(out) == ["valid_emb", "valid_target"] and (out["valid_emb"] == (want["valid"][0] > 0.25).float().numpy()).all()
    with pytest.raises(FileNotFoundError, match="GO-CC_train_embeddings_labels.pt"):
        downstream.load_data({**cfg, "task_name": "GO-CC"})


def _shipped_cfg():
    import yaml
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "saprot_mlp.yaml")) as f:
        return yaml.safe_load(f)


def test_sweep_walks_the_product_and_build_model_reads_the_config(monkeypatch):
    cfg = _shipped_cfg()
    seen = []

    def fake_evaluate(c, data):
        seen.append((c, data))
        return {"test_f1_max": float(len(seen))}
    monkeypatch.setattr(probe, "evaluate", fake_evaluate)
    loaded = []
    rows = probe.sweep(cfg, lambda c: loaded.append(c["task_name"]) or {"task": c["task_name"]})
    n = 2 * 2 * 1 * 2 * 2 * 2 * 2 * 2 * 2 * 9 * 1
    assert len(rows) == len(seen) == len(loaded) == n == 2304
    assert rows[0] == {"learning_rate": 0.001, "batch_size": 32, "max_epochs": 50, "hidden_dims": [256], "dropout_rate": 0.1, "use_batch_norm": True, "use_layer_norm": True,
                       "activation": "relu", "use_residual": True, "task_name": "HumanPPI", "model_type": "oneprot_16", "test_f1_max": 1.0}
    assert len({(tuple(r["hidden_dims"]),) + tuple(r[k] for k in probe.SWEEP_KEYS if k != "hidden_dims") for r in rows}) == n          # every combination once
    last, data = seen[-1]
    assert data == {"task": "DeepLoc10"} and last["task_name"] == "DeepLoc10" and last["model_type"] == "oneprot_16" and last["emb_dir"] == cfg["emb_dir"]
    assert last["model"] == {**cfg["model"], "learning_rate": 0.01, "batch_size": 64, "max_epochs": 50, "hidden_dims": [512, 256], "dropout_rate": 0.25,
                             "use_batch_norm": False, "use_layer_norm": False, "activation": "gelu", "use_residual": False}
    assert cfg["model"]["learning_rate"] == 0.001 and "sweep" not in last                     # the caller's config is not written to
    m = probe.build_model({"task_name": "HumanPPI", "model_type": "oneprot_16", "model": {**cfg["model"], "use_residual": True}})
    assert (m.input_dim, m.output_dim, m.hidden_dims, m.dropout_rate) == (2560, 1, [512, 256], 0.3) and m.residual_projection is not None
    assert isinstance(m.hidden_layers[1], torch.nn.BatchNorm1d) and isinstance(m.hidden_layers[2], torch.nn.ReLU)


def test_command_line_overrides(monkeypatch, capsys, tmp_path):
    import json
    import src.saprot_fit_mlp as S
    got = {}
    monkeypatch.setattr(S, "load_data", lambda c: {"loaded": c["emb_dir"]})
    monkeypatch.setattr(S, "evaluate", lambda c, d: got.update(cfg=c, data=d) or {"test_f1_max": 0.5})
    S.main(["--one", "task_name=GO-MF", "model.batch_size=64", "model.hidden_dims=[128, 64]", f"emb_dir={tmp_path}", "threshold=0.5", "seed=3"])
    c = got["cfg"]
    assert (c["task_name"], c["model"]["batch_size"], c["model"]["hidden_dims"], c["threshold"], c["seed"]) == ("GO-MF", 64, [128, 64], 0.5, 3)
    assert c["model"]["learning_rate"] == 0.001 and got["data"] == {"loaded": str(tmp_path)}   # what was not overridden is the file's
    assert json.loads(capsys.readouterr().out) == {"task_name": "GO-MF", "model_type": "esm2", "test_f1_max": 0.5}
    monkeypatch.setattr(S, "sweep", lambda c, d: [{"task_name": t} for t in c["sweep"]["task_name"]])
    S.main(["sweep.task_name=[EC, GO-BP]"])
    assert [json.loads(line) for line in capsys.readouterr().out.splitlines()] == [{"task_name": "EC"}, {"task_name": "GO-BP"}]
