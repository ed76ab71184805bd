"""ref src/collect_embeddings.py surface -> oneprot_amd.collect (task CSVs to the probes' embedding files on the HIP towers; no Lightning, Hydra, pandas or HF tokenizer).

    python src/collect_embeddings.py [--config configs/collect_embeddings.yaml] [--run] [key=value ...]

follows the config's `single_batch_mode` as the reference does (true: embed and write the shards; false: combine them); `--run` does both in one go.
key=value overrides are YAML values on dotted keys, e.g. output_dir=/data/embeddings/{model_name} esm_model=/models/esm2_t33_650M_UR50D max_tokens=65536."""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oneprot_amd import collect as _collect  # noqa: E402
from oneprot_amd.collect import (EsmSequenceTokenizer, collect_task, combine_shards, embed_sequences, load_model, plan_batches, read_task_csv,  # noqa: E402,F401
                                 split_of, write_shards)


def main(argv=None):
    return _collect.main(argv, os.path.join(_ROOT, "configs", "collect_embeddings.yaml"))


if __name__ == "__main__":
    main()
