"""ref src/eval.py surface -> oneprot_amd.evaluate (one test table embedded in every modality on the HIP towers, every modality pair ranked in both directions,
retrieval_metrics.csv; no Lightning, Hydra, pandas, sklearn or HF tokenizer).

    python src/eval.py [--config configs/eval.yaml] [key=value ...]

key=value overrides are YAML values on dotted keys, e.g. model.ckpt_path=/runs/best.ckpt dataset.csv_file_path=/data/test_all.csv output.csv_path=/tmp/retrieval_metrics.csv.
When rows tie exactly with their matching pair, <stem>_pessimistic.csv is written next to output.csv_path (rank + ties)."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oneprot_amd import evaluate as _evaluate  # noqa: E402
from oneprot_amd.evaluate import (CombinedDataset, calculate_retrieval_metrics, create_dataloader, embed_modalities, encode_inputs, load_custom_model,  # noqa: E402,F401
                                  read_table, write_results_to_csv)


def main(argv=None):
    return _evaluate.main(argv, os.path.join(_ROOT, "configs", "eval.yaml"))


if __name__ == "__main__":
    main()
