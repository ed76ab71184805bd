"""`_target_: src.data.datasets.text_dataset.TextDataset` (ref configs/data/modalities/text.yaml:3)."""
from oneprot_amd.text_data import BertWordPieceTokenizer, TextDataset  # noqa: F401
