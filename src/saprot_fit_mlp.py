"""ref src/saprot_fit_mlp.py surface -> oneprot_amd.probe (the MLP probe on the HIP kernels; no Lightning, Hydra or sklearn).

    python src/saprot_fit_mlp.py [--config configs/saprot_mlp.yaml] [--one] [key=value ...]

runs the sweep of the config (`--one`: only the fit its `model:` block describes) and prints one JSON row per combination.  key=value overrides are YAML
values on dotted keys, e.g. task_name=EC model.batch_size=64 emb_dir=/data/embeddings."""
import json
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oneprot_amd.probe import MLP, build_model, evaluate, fit, load_data, predict, sweep, task_dims  # noqa: E402,F401


def main(argv=None):
    import argparse
    import yaml
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default=os.path.join(_ROOT, "configs", "saprot_mlp.yaml"))
    ap.add_argument("--one", action="store_true", help="one fit of the `model:` block instead of the sweep")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    for ov in args.overrides:
        key, _, value = ov.partition("=")
        node, parts = cfg, key.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = yaml.safe_load(value)
    if args.one:
        print(json.dumps({"task_name": cfg["task_name"], "model_type": cfg["model_type"], **evaluate(cfg, load_data(cfg))}))
    else:
        for row in sweep(cfg, load_data):
            print(json.dumps(row))


if __name__ == "__main__":
    main()
