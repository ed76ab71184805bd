"""`_target_: src.data.datasets.seqsim_dataset.SequenceSimDataset` (ref configs/data/modalities/seqsim.yaml)."""
from oneprot_amd.token_data import SequenceSimDataset  # noqa: F401
