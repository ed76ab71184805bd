"""Writes tests/golden/probe_mlp.pt from the reference's own MLP class:

    python tests/golden/make_probe_golden.py <reference checkout>/src/saprot_fit_mlp.py

The reference module is loaded by file with stand-in modules for what it imports but its MLP never touches (hydra, omegaconf, pytorch_lightning(.callbacks),
utils, utils.downstream, and sklearn / scipy where they are not installed).  For {none, batch, layer norm} x {relu, gelu, leaky_relu} x {no residual [16, 8],
identity residual [24], projected residual [8]} at input_dim 24, 5 outputs, 7 rows, on torch's CPU fp32 kernels, it records: the state-dict names and shapes; the
drawn state dict and input; the train-mode (dropout 0) and eval-mode outputs; the three losses as the reference's training_step calls them; every parameter
gradient of each; the BatchNorm buffers after one train-mode forward; the parameters after three torch.optim.AdamW(lr=1e-3) steps on the BCE loss.  Plus the
names and shapes of one configuration with dropout.  The file holds tensors and names only."""
import importlib.util
import os
import sys
import types

import torch
import torch.nn.functional as F

INPUT_DIM, OUTPUT_DIM, ROWS = 24, 5, 7
RESIDUALS = {"none": ([16, 8], False), "identity": ([24], True), "projected": ([8], True)}


def load_reference(path):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    anything = type("Anything", (), {"__init__": lambda self, *a, **k: None})
    stub("hydra", main=lambda **kw: (lambda fn: fn))
    stub("omegaconf", DictConfig=dict)
    pl = stub("pytorch_lightning", LightningModule=torch.nn.Module, LightningDataModule=anything, Trainer=anything)
    pl.callbacks = stub("pytorch_lightning.callbacks", EarlyStopping=anything, RichProgressBar=anything, ModelCheckpoint=anything)
    utils = stub("utils")
    utils.downstream = stub("utils.downstream", save_results_to_csv=None, load_data=None, count_f1_max=None)
    for name, attrs in (("sklearn", {}), ("sklearn.metrics", dict(accuracy_score=None, f1_score=None, roc_auc_score=None, mean_squared_error=None, r2_score=None)),
                        ("scipy", {}), ("scipy.stats", dict(spearmanr=None))):
        try:
            __import__(name)
        except ImportError:
            stub(name, **attrs)
    spec = importlib.util.spec_from_file_location("reference_saprot_fit_mlp", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clone_sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def main():
    ref = load_reference(sys.argv[1])
    gen = torch.Generator().manual_seed(2024)
    x = torch.randn(ROWS, INPUT_DIM, generator=gen)
    targets = {0: torch.randint(0, 2, (ROWS, OUTPUT_DIM), generator=gen).float(), 1: torch.randn(ROWS, OUTPUT_DIM, generator=gen),
               2: torch.randint(0, OUTPUT_DIM, (ROWS,), generator=gen)}
    loss_fns = {0: F.binary_cross_entropy_with_logits, 1: F.mse_loss, 2: F.cross_entropy}
    configs = []
    for norm in ("none", "batch", "layer"):
        for activation in ("relu", "gelu", "leaky_relu"):
            for residual, (hidden, use_residual) in RESIDUALS.items():
                torch.manual_seed(len(configs))
                model = ref.MLP(INPUT_DIM, OUTPUT_DIM, hidden, 0.0, norm == "batch", norm == "layer", activation, use_residual)
                with torch.no_grad():                                   # the defaults (gamma 1, beta 0, running 0 / 1) would hide mistakes
                    for mod in model.modules():
                        if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
                            mod.weight.copy_(1.0 + 0.2 * torch.rand(mod.weight.shape, generator=gen))
                            mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=gen))
                        if isinstance(mod, torch.nn.BatchNorm1d):
                            mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=gen))
                            mod.running_var.copy_(1.0 + 0.2 * torch.rand(mod.running_var.shape, generator=gen))
                sd0 = clone_sd(model)
                rec = dict(norm=norm, activation=activation, residual=residual, hidden_dims=hidden, use_residual=use_residual,
                           names={k: tuple(v.shape) for k, v in sd0.items()}, state_dict=sd0)
                model.eval()
                with torch.no_grad():
                    rec["out_eval"] = model(x).clone()
                model.train()
                with torch.no_grad():
                    rec["out_train"] = model(x).clone()
                rec["buffers_after"] = {k: v for k, v in clone_sd(model).items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
                rec["loss"], rec["grads"] = {}, {}
                for kind, fn in loss_fns.items():
                    model.load_state_dict(sd0)
                    model.train()
                    model.zero_grad(set_to_none=True)
                    ls = fn(model(x), targets[kind])
                    ls.backward()
                    rec["loss"][kind] = ls.detach().clone()
                    rec["grads"][kind] = {k: p.grad.clone() for k, p in model.named_parameters()}
                model.load_state_dict(sd0)
                model.train()
                opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
                for _ in range(3):
                    opt.zero_grad(set_to_none=True)
                    loss_fns[0](model(x), targets[0]).backward()
                    opt.step()
                rec["adamw3"] = {k: p.detach().clone() for k, p in model.named_parameters()}
                configs.append(rec)
    with_dropout = ref.MLP(INPUT_DIM, OUTPUT_DIM, [16, 8], 0.25, True, False, "relu", False)
    out = dict(input_dim=INPUT_DIM, output_dim=OUTPUT_DIM, x=x, targets=targets, configs=configs,
               dropout_names={k: tuple(v.shape) for k, v in with_dropout.state_dict().items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "probe_mlp.pt")
    torch.save(out, path)
    print(f"wrote {path}: {len(configs)} configurations, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
