"""`_target_: src.data.oneprot_datamodule.OneProtDataModule` (ref configs/data/default.yaml:1)."""
from oneprot_amd.datamodule import DATASET_CLASSES, OneProtDataModule  # noqa: F401
