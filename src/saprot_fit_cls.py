"""ref src/saprot_fit_cls.py surface -> oneprot_amd.gbt (the gradient-boosted tree probe on the HIP kernels; no xgboost, Hydra or sklearn).

    python src/saprot_fit_cls.py [--config configs/saprot_sweep_xgboost_cls.yaml] [--one] [--scores labels|proba] [key=value ...]

runs the sweep of the config (`--one`: only the fit its `downstream_model:` block describes) and prints one JSON row per combination.  key=value overrides are
YAML values on dotted keys, e.g. task_name=HumanPPI downstream_model.max_depth=3 emb_dir=/data/embeddings."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oneprot_amd.gbt import XGBClassifier, build_model, cli_main, evaluate, load_data, objective_of, sweep  # noqa: E402,F401


def main(argv=None):
    cli_main(argv, os.path.join(_ROOT, "configs", "saprot_sweep_xgboost_cls.yaml"), __doc__.split("\n")[0])


if __name__ == "__main__":
    main()
