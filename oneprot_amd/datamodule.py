"""`OneProtDataModule` (ref src/data/oneprot_datamodule.py:25-84) without Lightning: the datasets of every configured modality for the three splits, one
DataLoader each, combined as the reference combines them -- "min_size" for training (one dict {modality: batch} per step until the shortest loader is
exhausted), "sequential" for validation and test.  The collate functions touch the GPU, so every loader runs in the main process: `num_workers` is
accepted and forced to 0.  A modality's optional `attributes` mapping is set on its built datasets (device, packed, packed_text, packed_msa: the
switches the constructors, which keep the reference's signatures, do not take)."""
import logging
from typing import Any, Dict, Optional

from torch.utils.data import DataLoader

from .data import CombinedLoader
from .graph_data import StructDataset
from .msa_data import MSADataset
from .text_data import TextDataset
from .token_data import SequenceSimDataset, StructTokenDataset

DATASET_CLASSES = {
    "msa": MSADataset,
    "struct_graph": StructDataset,
    "pocket": StructDataset,
    "text": TextDataset,
    "struct_token": StructTokenDataset,
    "seqsim": SequenceSimDataset,
}


def _get(node, key, default=None):
    if hasattr(node, "get"):
        return node.get(key, default)
    return getattr(node, key, default)


class OneProtDataModule:
    def __init__(self, modalities, num_workers, pin_memory, default_batch_size):
        self.modalities = modalities
        self.datasets: Dict[str, Any] = {}
        self.logger = logging.getLogger(__name__)
        if num_workers:
            self.logger.info(f"num_workers = {num_workers} is forced to 0: the collate functions use the GPU and run in the main process")
        self.num_workers = 0
        self.pin_memory = pin_memory
        self.default_batch_size = default_batch_size

    def setup(self, stage: Optional[str] = None):
        if self.datasets:
            return
        for modality, modality_cfg in self.modalities.items():
            if modality not in DATASET_CLASSES:
                self.logger.error(f"Unknown modality: {modality}")
                continue
            dataset_class = DATASET_CLASSES[modality]
            for split in ["train", "val", "test"]:
                dataset_kwargs = {**_get(modality_cfg, "dataset"), "split": split}
                dataset_kwargs.pop("_target_", None)
                try:
                    dataset = dataset_class(**dataset_kwargs)
                    for name, value in (_get(modality_cfg, "attributes") or {}).items():
                        setattr(dataset, name, value)
                    self.datasets[f"{modality}_{split}"] = dataset
                except Exception as e:
                    self.logger.error(f"Error creating dataset for {modality} {split}: {str(e)}")
                    continue
            self.logger.info(f"{modality} Train/Validation/Test Dataset Size = " + " / ".join(str(len(self.datasets.get(f"{modality}_{s}", []))) for s in ("train", "val", "test")))

    def _create_dataloader(self, split: str, shuffle: bool = False):
        iterables = {}
        for modality, modality_cfg in self.modalities.items():
            if f"{modality}_{split}" not in self.datasets:
                self.logger.warning(f"Dataset for {modality} {split} not found, skipping.")
                continue
            batch_size = _get(_get(modality_cfg, "batch_size") or {}, split, self.default_batch_size)
            dataset = self.datasets[f"{modality}_{split}"]
            iterables[modality] = DataLoader(dataset=dataset, batch_size=batch_size, num_workers=self.num_workers, pin_memory=self.pin_memory,
                                             collate_fn=dataset.collate_fn, shuffle=shuffle, drop_last=False)
        return CombinedLoader(iterables, "min_size" if shuffle else "sequential")

    def train_dataloader(self):
        return self._create_dataloader("train", shuffle=True)

    def val_dataloader(self):
        return self._create_dataloader("val")

    def test_dataloader(self):
        return self._create_dataloader("test")
