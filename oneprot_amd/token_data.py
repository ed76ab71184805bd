"""The struct_token and seqsim datasets (ref src/data/datasets/struct_token_dataset.py, seqsim_dataset.py): host code, same constructors and return
tuples `(sequence_ids.long(), modality_ids.long(), modality, raw)`.  The reference's struct_token module imports h5py at the top and cannot run where
h5py is missing, so that class is restated and only its tokenizer is pinned (tests/golden/struct_token_tokenizer.json); the seqsim collate is pinned
against the reference's own class (tests/golden/seqsim_collate.json).  HDF5 inputs go through graph_data's open and leaf helpers: a path (opened with
h5py where it imports) or a nested mapping."""
import csv
import json
import os
import random

from torch.utils.data import Dataset

from .graph_data import _open, _value
from .text_data import as_str, esm_side, eval_len, sequence_tokenizer

# ref struct_token_dataset.py:39: the foldseek letters and '#', appended to the ESM table: ids 33 .. 53
NEW_TOKENS = ["p", "y", "n", "w", "r", "q", "h", "g", "d", "l", "v", "t", "m", "f", "s", "a", "e", "i", "k", "c", "#"]


class StructTokenDataset(Dataset):
    """ref struct_token_dataset.py:8-90.  `filename`: the HDF5 file of `strucseq` strings (a path or a nested mapping; may be replaced after construction).
    The sequence is the characters of `strucseq` at even positions with '#' removed, the structure string those at odd positions, with '#' removed when
    `remove_hash` is set; an id the file does not hold is skipped.  Attributes set after construction: `device` (where the batch goes; None: it stays
    on the host, the reference's layout) and `packed` (both sides as PackedTokens)."""

    def __init__(self, data_dir: str, filename: str, split: str, max_length: int = 1024, seq_tokenizer: str = "facebook/esm2_t33_650M_UR50D", remove_hash=True,
                 full=False):
        self.split, self.remove_hash, self.max_length = split, remove_hash, max_length
        txt_file = f"{data_dir}/{split}_saprot_full.txt" if split == "train" and full else f"{data_dir}/{split}_saprot.txt"
        try:
            with open(txt_file, "r") as file:
                self.ids = [line.strip() for line in file]
        except FileNotFoundError:
            print(f"File not found: {txt_file}")
            self.ids = []
        self.struct_tokenizer = sequence_tokenizer(seq_tokenizer, NEW_TOKENS)
        self.seq_tokenizer = sequence_tokenizer(seq_tokenizer)
        self.filename = filename
        self.device, self.packed = None, False

    def __len__(self) -> int:
        return eval_len(self.split, len(self.ids))

    def __getitem__(self, idx: int) -> str:
        return self.ids[idx]

    def collate_fn(self, data):
        sequences, structs = [], []
        h5_file, opened = _open(self.filename)
        try:
            for seq_id in data:
                if seq_id in h5_file:
                    strucseq = as_str(_value(h5_file[seq_id]["strucseq"]))
                    sequences.append(strucseq[0::2].replace("#", ""))
                    structure_seq = strucseq[1::2]
                    structs.append(structure_seq.replace("#", "") if self.remove_hash else structure_seq)
        finally:
            if opened:
                h5_file.close()
        sequence_input = esm_side(self.seq_tokenizer, sequences, self.max_length, self.packed)
        struct_input = esm_side(self.struct_tokenizer, structs, self.max_length, self.packed)
        if self.device is not None:
            sequence_input, struct_input = sequence_input.to(self.device), struct_input.to(self.device)
        return sequence_input, struct_input, "struct_token", sequences


class SequenceSimDataset(Dataset):
    """ref seqsim_dataset.py:10-127: per item (the sequence, its MSA row), the collate builds two lists of three strings each -- (req_seq, the sequence, a
    pathogenic mutant) and (aligned_seq, a benign mutant, another pathogenic mutant) -- with the reference's `random.choice` calls in the reference's
    order; a mutation whose first letter does not stand at its position is drawn again.  `{split}_msa_seqsim.csv` has a header row with the columns
    req_seq and aligned_seq; an item's MSA row is a dict.  Attributes set after construction: `device`, `packed` (as StructTokenDataset)."""

    def __init__(self, data_dir: str, split: str, seq_tokenizer: str = "facebook/esm2_t33_650M_UR50D", max_length: int = 1024,
                 modality: str = "combined_seqsim_msa"):
        self.data_dir, self.split, self.max_length, self.modality = data_dir, split, max_length, modality
        self.seq_tokenizer = sequence_tokenizer(seq_tokenizer)
        self.device, self.packed = None, False
        self._load_data()

    def _load_data(self):
        with open(os.path.join(self.data_dir, f"{self.split}_seqsim.txt"), "r") as f:
            self.sequence_ids = [line.strip() for line in f]
        self.benign_mutations = self._load_json("clinvar_full_benign_mutations.json")
        self.pathogenic_mutations = self._load_json("clinvar_full_pathogenic_mutations.json")
        with open(f"{self.data_dir}/{self.split}_msa_seqsim.csv", newline="", encoding="utf-8") as f:
            self.msa_data = [row for row in csv.DictReader(f)]

    def _load_json(self, filename):
        with open(os.path.join(self.data_dir, filename), "r") as f:
            return json.load(f)

    def __len__(self) -> int:
        return eval_len(self.split, len(self.msa_data))

    def __getitem__(self, idx: int):
        return self.sequence_ids[idx % len(self.sequence_ids)], self.msa_data[idx]

    @staticmethod
    def _apply_mutation(sequence: str, mutation: str) -> str:
        letter1, position, letter2 = mutation[0], int(mutation[1:-1]) - 1, mutation[-1]
        assert sequence[position] == letter1, f"Mutation mismatch: expected {letter1} at position {position}, found {sequence[position]}"
        return sequence[:position] + letter2 + sequence[position + 1:]

    def _draw(self, seq_id, table):
        while True:
            try:
                return self._apply_mutation(seq_id, random.choice(table[seq_id]))
            except AssertionError:
                continue

    def collate_fn(self, batch):
        list1, list2 = [], []
        for seq_id, msa_row in batch:
            list1 += [msa_row["req_seq"], seq_id]
            list2.append(msa_row["aligned_seq"])
            list2.append(self._draw(seq_id, self.benign_mutations))
            first, second = self._draw(seq_id, self.pathogenic_mutations), self._draw(seq_id, self.pathogenic_mutations)
            list1.append(first)
            list2.append(second)
        sequence_input1 = esm_side(self.seq_tokenizer, list1, self.max_length, self.packed)
        sequence_input2 = esm_side(self.seq_tokenizer, list2, self.max_length, self.packed)
        if self.device is not None:
            sequence_input1, sequence_input2 = sequence_input1.to(self.device), sequence_input2.to(self.device)
        return sequence_input1, sequence_input2, "seqsim", sequence_input1
