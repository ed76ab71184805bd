"""`_target_: src.data.datasets.msa_dataset.MSADataset` (ref configs/data/modalities/msa.yaml:3)."""
from oneprot_amd.msa_data import MSADataset, MsaBatchConverter  # noqa: F401
