"""`_target_: src.data.datasets.struct_token_dataset.StructTokenDataset` (ref configs/data/modalities/struct_token.yaml:3)."""
from oneprot_amd.token_data import NEW_TOKENS, StructTokenDataset  # noqa: F401
