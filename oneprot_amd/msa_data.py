"""MSA input: the a3m reader, the greedy depth selection and the two tokenizations of ref src/data/datasets/msa_dataset.py:42-58 without Biopython, scipy,
fair-esm or an HF tokenizer.  The selection and the gather into token ids run on the device (csrc/msa_select.hip, include/oneprot_hip.h "MSA input"); the
same exact rule in numpy is the host path, so that a user without a GPU gets the same selection (DESIGN.md sections 3 and 7).

The rule: S_j = the sum over the rows chosen so far of the number of positions where that row and row j differ, an integer; every step picks the
unselected j with the largest ("max") or smallest ("min") S_j, the lowest j among equal S_j; it starts from row 0.  The reference averages the same
distances in fp64 and so orders equal sums by rounding noise; on inputs without such ties the two select the same rows (tests/golden/msa_select.json).
The token table is the published ESM-1b / MSA Transformer alphabet restated here; like the rest of the MSA tower it is UNPINNED against fair-esm."""
import os
import string
from typing import List, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from .packing import PAD_MULTIPLE, PackedMsa

CLS_ID, PAD_ID, EOS_ID, UNK_ID, NULL_ID, MASK_ID = 0, 1, 2, 3, 31, 32
LETTERS = "LAGVSERTIDPKQNFYMHWCXBUZO.-"             # ids 4 .. 30
MSA_TRUNCATION = 1022                                 # get_batch_converter(truncation_seq_length=1022)
MAX_PICKS = 1024                                      # k_max of oneprot_msa_select
MAX_ROW_LEN = 65535
# device=None picks the GPU for a batch with at least this many row bytes (sum of N_b * L_b) and the host path below it: a device call costs about
# 0.5 ms whatever the size (the copy and num_seqs launches), which the host path needs for one MSA of 64 x 512 -- the measured crossover; at 256 x 512 the
# device is 3 x faster, at 10 000 x 512 x 16 MSAs 640 x (profiles/msa_select.json)
DEVICE_MIN_BYTES = 1 << 15


def filter_and_create_msa_file_list(filename: str) -> List[str]:
    """ref msa_utils.py:9-19: the second comma-separated field of every line that names an .a3m file"""
    file_list = []
    with open(filename, "r") as file:
        for line in file:
            line = line.strip()
            if ".a3m" in line:
                file_list.append(line.split(",")[1])
    return file_list


_DELETE = str.maketrans(dict.fromkeys(string.ascii_lowercase + ".*"))


def remove_insertions(sequence: str) -> str:
    """ref msa_utils.py:42-49: lowercase letters, '.' and '*' are insertions relative to the query"""
    return sequence.translate(_DELETE)


def _parse_fasta(filename):
    records, desc, parts = [], None, []
    with open(filename, "r") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if desc is not None:
                    records.append((desc, "".join(parts)))
                desc, parts = line[1:].strip(), []
            elif desc is not None:
                parts.append("".join(line.split()))
    if desc is not None:
        records.append((desc, "".join(parts)))
    return records


def read_msa(filename: str) -> List[Tuple[str, str]]:
    """ref msa_utils.py:51-57: [(description, aligned sequence)] of a FASTA / a3m file, insertions removed; `filename + '.a3m'` when `filename` cannot be
    read.  Rows of unequal length after the removal raise ValueError (the reference fails inside numpy in greedy_select)."""
    try:
        records = _parse_fasta(filename)
    except OSError:
        filename = filename + ".a3m"
        records = _parse_fasta(filename)
    msa = [(desc, remove_insertions(seq)) for desc, seq in records]
    lengths = {len(seq) for _, seq in msa}
    if len(lengths) > 1:
        raise ValueError(f"{filename}: rows of unequal length after insertion removal ({sorted(lengths)[:4]} ...): not an alignment")
    return msa


def encode_rows(msa) -> np.ndarray:
    """uint8 [N, L]: the rows' letters as bytes (what the reference compares: np.bytes_ viewed as uint8); a letter outside latin-1 becomes '?'"""
    seqs = [seq for _, seq in msa]
    if not seqs:
        raise ValueError("an MSA without rows")
    L = len(seqs[0])
    if L == 0 or any(len(s) != L for s in seqs):
        raise ValueError("the rows of an MSA must have one length, at least 1")
    return np.frombuffer("".join(seqs).encode("latin-1", "replace"), dtype=np.uint8).reshape(len(seqs), L)


def _check_mode(mode):
    if mode not in ("max", "min"):
        raise ValueError(f"mode must be 'max' or 'min', got {mode!r}")


def select_host(rows: np.ndarray, num_seqs: int, mode: str = "max"):
    """(indices ascending, picks in the order made) of the exact rule on one uint8 [N, L] alignment; min(num_seqs, N) picks"""
    _check_mode(mode)
    N = rows.shape[0]
    picks = min(int(num_seqs), N)
    order = [0]
    S = np.zeros(N, dtype=np.int64)
    taken = np.zeros(N, dtype=bool)
    taken[0] = True
    worst = np.iinfo(np.int64).min if mode == "max" else np.iinfo(np.int64).max
    for _ in range(picks - 1):
        S += (rows != rows[order[-1]]).sum(1)
        masked = np.where(taken, worst, S)
        j = int(masked.argmax() if mode == "max" else masked.argmin())       # the first of equal values: the lowest index
        order.append(j)
        taken[j] = True
    return sorted(order), order


def _check_batch(arrays, num_seqs):
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if not arrays or len(arrays) > 65535:
        raise ValueError("a batch holds 1 .. 65535 MSAs")
    for b, a in enumerate(arrays):
        if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or not 1 <= a.shape[1] <= MAX_ROW_LEN:
            raise ValueError(f"MSA {b}: expected a uint8 [N >= 1, 1 <= L <= {MAX_ROW_LEN}] array, got {a.dtype} {a.shape}")
    ks = [int(num_seqs)] * len(arrays) if np.isscalar(num_seqs) else [int(k) for k in num_seqs]
    if len(ks) != len(arrays) or any(not 1 <= k <= MAX_PICKS for k in ks):
        raise ValueError(f"num_seqs must be 1 .. {MAX_PICKS} (one number, or one per MSA)")
    return arrays, ks


def _want_device(device, arrays):
    """torch.device of the HIP path, or None for the host path"""
    if device is None:
        from . import hip
        if not (os.path.exists(hip.LIB_PATH) and torch.cuda.is_available()):
            return None
        if sum(a.size for a in arrays) < DEVICE_MIN_BYTES:
            return None
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    return None if device.type == "cpu" else device


class DeviceMsaBatch:
    """The byte stream and the tables of include/oneprot_hip.h "MSA input" for a list of uint8 [N_b, L_b] arrays: rows padded to a multiple of 16 bytes
    with 0, every block at a multiple of 16."""

    def __init__(self, arrays, ks, device):
        self.device = torch.device(device)
        rows, at = [], 0
        for a, k in zip(arrays, ks):
            N, L = a.shape
            stride = (L + 15) & ~15
            rows.append([at, N, L, k])
            at += N * stride
        self.n, self.n_bytes = len(arrays), at
        self.table_host = torch.tensor(rows, dtype=torch.int64)
        self.shapes = [(N, L) for _, N, L, _ in rows]
        self.picks = [min(k, N) for _, N, _, k in rows]
        self.k_max = max(ks)
        host = torch.zeros(at, dtype=torch.uint8, pin_memory=self.device.type == "cuda")
        flat = host.numpy()
        for a, (b0, N, L, _) in zip(arrays, rows):
            stride = (L + 15) & ~15
            flat[b0:b0 + N * stride].reshape(N, stride)[:, :L] = a
        self.bytes = host.to(self.device, non_blocking=True)
        self.table = self.table_host.to(self.device, non_blocking=True)
        self._host = host                      # the pinned source of an asynchronous copy stays alive with the batch

    def select(self, mode="max", want_order=False):
        """int32 [n, k_max] on the device: every MSA's chosen rows ascending, -1 behind them (and the picks in the order made)"""
        from . import hip
        _check_mode(mode)
        total, deepest = sum(N for N, _ in self.shapes), max(N for N, _ in self.shapes)
        ws_bytes = hip.query("oneprot_msa_select_workspace", self.n, self.k_max, total, deepest)
        if ws_bytes == 0:
            raise hip.HipKernelError("oneprot_msa_select_workspace refused the batch")
        with torch.cuda.device(self.device):
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            indices = torch.empty(self.n, self.k_max, dtype=torch.int32, device=self.device)
            order = torch.empty_like(indices) if want_order else None
            hip.call("oneprot_msa_select", self.bytes, self.table, ws, indices, order, self.table_host.data_ptr(), ws_bytes, self.n_bytes, self.n, self.k_max,
                     int(mode == "min"))
        return (indices, order) if want_order else indices


def select_batch(arrays, num_seqs, mode="max", device=None, want_order=False):
    """The batched selection the collate uses.  arrays: uint8 [N_b, L_b] each; num_seqs: one number or one per MSA.  Returns the index table int32
    [n, k_max] (row b: the chosen rows of MSA b ascending, -1 behind them) on the device that computed it -- a GPU tensor from the HIP path, a CPU tensor
    from the host path (device="cpu", or device=None without a GPU, without the library or below DEVICE_MIN_BYTES).  want_order adds the picks in the order
    made."""
    _check_mode(mode)
    arrays, ks = _check_batch(arrays, num_seqs)
    dev = _want_device(device, arrays)
    if dev is not None:
        return DeviceMsaBatch(arrays, ks, dev).select(mode, want_order)
    k_max = max(ks)
    indices = torch.full((len(arrays), k_max), -1, dtype=torch.int32)
    order = torch.full_like(indices, -1)
    for b, (a, k) in enumerate(zip(arrays, ks)):
        idx, picks = select_host(a, k, mode)
        indices[b, :len(idx)] = torch.tensor(idx, dtype=torch.int32)
        order[b, :len(picks)] = torch.tensor(picks, dtype=torch.int32)
    return (indices, order) if want_order else indices


def greedy_select(msa: List[Tuple[str, str]], num_seqs: int, mode: str = "max", device=None) -> List[Tuple[str, str]]:
    """ref msa_utils.py:21-40 with the exact rule (module docstring): the chosen (description, sequence) pairs in file order"""
    assert mode in ("max", "min")
    if len(msa) <= num_seqs:
        return msa
    if num_seqs > MAX_PICKS:
        raise ValueError(f"num_seqs = {num_seqs}: the selection takes up to {MAX_PICKS} rows")
    indices = select_batch([encode_rows(msa)], max(int(num_seqs), 1), mode, device)[0].tolist()       # num_seqs < 1: row 0, as the reference's loop gives
    return [msa[i] for i in indices if i >= 0]


def _byte_map():
    table = np.full(256, UNK_ID, dtype=np.int32)
    for i, ch in enumerate(LETTERS):
        table[ord(ch)] = 4 + i
    return table


class MsaBatchConverter:
    """The token table and the two layouts.  Row r of an MSA: <cls> and its first min(L, 1022, max_length - 1) letters (fair-esm's MSA batch converter with
    truncation_seq_length=1022, then `[:, :, :max_length]`); the sequence side: <cls>, row 0's letters, <eos>, cut to max_length with <eos> kept and padded
    with 1 (the HF ESM-2 tokenizer with padding=True, truncation=True).  Ids: <cls> 0, <pad> 1, <eos> 2, <unk> 3, LETTERS 4 .. 30, <null_1> 31, <mask> 32,
    every other byte 3."""
    cls_idx, padding_idx, eos_idx, unk_idx, mask_idx = CLS_ID, PAD_ID, EOS_ID, UNK_ID, MASK_ID
    all_toks = ["<cls>", "<pad>", "<eos>", "<unk>"] + list(LETTERS) + ["<null_1>", "<mask>"]

    def __init__(self, max_length: int = 1024, truncation_seq_length: int = MSA_TRUNCATION):
        if max_length < 2:
            raise ValueError("max_length must hold <cls> and one more token")
        if truncation_seq_length != MSA_TRUNCATION:
            raise ValueError(f"the device tokenizer truncates rows to {MSA_TRUNCATION} letters, as the reference's dataset does")
        self.max_length = int(max_length)
        self.byte_map = _byte_map()
        self._dev_map = {}

    def row_tokens(self, L):
        return min(1 + min(L, MSA_TRUNCATION), self.max_length)

    def seq_tokens(self, L):
        return min(L + 2, self.max_length)

    # ------------------------------------------------------------------------------------------------------------ host
    def host(self, arrays, indices, packed=False):
        """(sequence ids int64 [n, Ls], MSA tokens) on the CPU from uint8 arrays and an index table (rows of -1-terminated ascending indices)"""
        n = len(arrays)
        blocks = []
        for a, idx in zip(arrays, indices.tolist()):
            idx = [i for i in idx if i >= 0]
            Lt = self.row_tokens(a.shape[1])
            blk = np.full((len(idx), Lt), CLS_ID, dtype=np.int64)
            blk[:, 1:] = self.byte_map[a[idx, :Lt - 1]]
            blocks.append(torch.from_numpy(blk))
        Ls = max(self.seq_tokens(a.shape[1]) for a in arrays)
        seq = torch.full((n, Ls), PAD_ID, dtype=torch.int64)
        for b, a in enumerate(arrays):
            m = self.seq_tokens(a.shape[1])
            seq[b, 0], seq[b, m - 1] = CLS_ID, EOS_ID
            seq[b, 1:m - 1] = torch.from_numpy(self.byte_map[a[0, :m - 2]].astype(np.int64))
        if packed:
            return seq, PackedMsa.from_list(blocks, pad_id=PAD_ID)
        R, Lt = max(b.shape[0] for b in blocks), max(b.shape[1] for b in blocks)
        tokens = torch.full((n, R, Lt), PAD_ID, dtype=torch.int64)
        for b, blk in enumerate(blocks):
            tokens[b, :blk.shape[0], :blk.shape[1]] = blk
        return seq, tokens

    # ------------------------------------------------------------------------------------------------------------ device
    def device(self, batch: DeviceMsaBatch, indices, packed=False):
        """the same from a DeviceMsaBatch and its index table on the GPU: int64 tensors on the batch's device, or a PackedMsa there"""
        from . import hip
        dev = batch.device
        bm = self._dev_map.get(str(dev))
        if bm is None:
            bm = self._dev_map[str(dev)] = torch.from_numpy(self.byte_map).to(dev)
        shapes = [(p, self.row_tokens(L)) for p, (_, L) in zip(batch.picks, batch.shapes)]
        R, Lt = max(r for r, _ in shapes), max(l for _, l in shapes)
        Ls = max(self.seq_tokens(L) for _, L in batch.shapes)
        with torch.cuda.device(dev):
            seq = torch.empty(batch.n, Ls, dtype=torch.int64, device=dev)
            if packed:
                cu = torch.zeros(batch.n + 1, dtype=torch.int32)
                cu[1:] = torch.tensor([r * l for r, l in shapes], dtype=torch.int64).cumsum(0).to(torch.int32)
                total = int(cu[-1])
                T_pad = (total + PAD_MULTIPLE - 1) // PAD_MULTIPLE * PAD_MULTIPLE
                tokens, cu = torch.empty(T_pad, dtype=torch.int64, device=dev), cu.to(dev)
            else:
                T_pad, cu = 0, None
                tokens = torch.empty(batch.n, R, Lt, dtype=torch.int64, device=dev)
            hip.call("oneprot_msa_tokenize", batch.bytes, batch.table, indices, bm, tokens, cu, seq, batch.table_host.data_ptr(), batch.n_bytes, batch.n,
                     batch.k_max, R, Lt, Ls, self.max_length, T_pad, CLS_ID, PAD_ID, EOS_ID)
        return seq, (PackedMsa(tokens, cu, shapes, pad_id=PAD_ID) if packed else tokens)


class MSADataset(Dataset):
    """ref src/data/datasets/msa_dataset.py:8-58, same constructor.  `seq_tokenizer` is accepted and ignored (the ESM-2 vocabulary is MsaBatchConverter's
    table) and `model_name_or_path` is not opened.  Two attributes set after construction choose where and in which layout the collate works:
    `dataset.device` (None: the GPU when there is one and the batch is large enough, see DEVICE_MIN_BYTES; "cpu": the host path) and `dataset.packed_msa`
    (True: msa_input is a PackedMsa).  collate_fn touches the GPU, so it belongs in the main process: DataLoader(..., num_workers=0)."""

    def __init__(self, data_dir: str, split: str, max_length: int = 1024,
                 msa_depth: int = 100, seq_tokenizer: str = "facebook/esm2_t33_650M_UR50D", model_name_or_path: str = ""):
        filename = f"{data_dir}/{split}_msa.csv"
        self.msa_files = filter_and_create_msa_file_list(filename)
        self.msa_padding_idx = 1
        self.msa_transformer_batch_converter = MsaBatchConverter(max_length=max_length, truncation_seq_length=1022)
        self.seq_tokenizer = seq_tokenizer
        self.max_length = max_length
        self.msa_depth = msa_depth
        self.split = split
        self.device = None
        self.packed_msa = False

    def __len__(self) -> int:
        if self.split == "train":
            return len(self.msa_files)
        else:
            return 1000

    def __getitem__(self, idx: int) -> str:
        return self.msa_files[idx]

    def collate_fn(self, msa_files: List[str]):
        """(sequence_input int64 [B, Ls], msa_input int64 [B, R, Lm] or PackedMsa, "msa", sequences): on the GPU from the device path, on the CPU from the
        host path"""
        msas = [read_msa(f) for f in msa_files]
        sequences = [m[0][1] for m in msas]
        arrays, ks = _check_batch([encode_rows(m) for m in msas], self.msa_depth)
        conv = self.msa_transformer_batch_converter
        dev = _want_device(self.device, arrays)
        if dev is None:
            indices = select_batch(arrays, ks, "max", "cpu")
            sequence_input, msa_input = conv.host(arrays, indices, self.packed_msa)
        else:
            batch = DeviceMsaBatch(arrays, ks, dev)
            sequence_input, msa_input = conv.device(batch, batch.select("max"), self.packed_msa)
        return sequence_input, msa_input, "msa", sequences
