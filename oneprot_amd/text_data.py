"""Text input: HF's fast BERT tokenizer (ref src/data/datasets/text_dataset.py:25,51) without `tokenizers` or `transformers`, and the text dataset.
The batch call runs on the device (csrc/wordpiece.hip, include/oneprot_hip.h "text input"); `BertWordPieceTokenizer.encode_all` is the same rule on the
host: the specification, and the path of a user without a GPU (DESIGN.md section 7 states the rule once and lists the known differences).

The rule is `tokenizers`' BertNormalizer(clean_text, handle_chinese_chars, strip_accents = lowercase, lowercase) + BertPreTokenizer +
WordPiece(max_input_chars_per_word=100) + [CLS] .. [SEP] + truncation.  Per code point, in this order: U+0000, U+FFFD and the categories Cc, Cf and Co
other than tab, line feed and carriage return are dropped (an unassigned code point, Cn, is kept: `tokenizers` keeps it); those three and every
White_Space character become a space; a code point of BERT's eight CJK ranges gets a space on both sides; when lowercasing, NFD and the Mn marks are
dropped, then every character is lowercased on its own.  Words are split at spaces, every punctuation character (ASCII punctuation or P*) is a word of
its own, a word of more than 100 characters is [UNK], every other word is matched greedily, longest piece first, continuation pieces under "##"; one
position without a match makes the whole word one [UNK]."""
import functools
import json
import os
import unicodedata

import numpy as np
import torch
from torch.utils.data import Dataset

from .packing import PAD_MULTIPLE, PackedTokens

KIND_OTHER, KIND_SOLO, KIND_SPACE = 0, 1, 2          # a normalised character: part of a word / a word of its own (punctuation, CJK) / a separator
MAX_WORD_CHARS = 100
MAX_EXPANSION = 3                                    # normalised characters per input character (kMaxExpand of csrc/wordpiece.hip); asserted by norm_table
HASH_P = 0x01000193
WHITE_SPACE = frozenset([9, 10, 11, 12, 13, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x2000, 0x200B)))
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF), (0xF900, 0xFAFF),
              (0x2F800, 0x2FA1F))
_ASCII_PUNCT = frozenset(map(ord, "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"))
# device=None picks the GPU for a batch with at least this many UTF-8 bytes and the host rule below it.  Measured on one text (the worst case for the
# device: one work-group walks it alone) against the host rule with a cold word cache: a tie at 869 bytes, the device ahead from 1.8 KB on; a batch
# of many texts only moves the crossover down (tools/text_tokenize_ab.py, profiles/text_tokenize.json)
DEVICE_MIN_BYTES = 1 << 10


def _kind_of(ch):
    cp = ord(ch)
    if cp in WHITE_SPACE:
        return KIND_SPACE
    if cp in _ASCII_PUNCT or unicodedata.category(ch).startswith("P"):
        return KIND_SOLO
    return KIND_OTHER


def is_cjk(cp):
    return any(lo <= cp <= hi for lo, hi in CJK_RANGES)


def normalize_char(ch, lowercase=True):
    """the five steps for one character: a tuple of (character, kind), empty when it is dropped"""
    cp = ord(ch)
    if cp == 0 or cp == 0xFFFD:
        return ()
    if ch in "\t\n\r":
        return ((" ", KIND_SPACE),)
    if unicodedata.category(ch) in ("Cc", "Cf", "Co", "Cs"):
        return ()
    if cp in WHITE_SPACE:
        return ((" ", KIND_SPACE),)
    out = ch
    if lowercase:
        out = "".join(c for c in unicodedata.normalize("NFD", ch) if unicodedata.category(c) != "Mn")
        out = "".join(c.lower() for c in out)
    if is_cjk(cp):                                   # " c ": a word of its own, like a punctuation character
        if len(out) != 1:
            raise AssertionError(f"U+{cp:04X}: a CJK character that does not normalise to one character")
        return ((out, KIND_SOLO),)
    return tuple((c, _kind_of(c)) for c in out)


@functools.lru_cache(maxsize=2)
def norm_table(lowercase=True):
    """(index int32 [0x1100], entries int32 [n_blocks, 256], pool int32 [n_pool]) of include/oneprot_hip.h "text input", for every code point"""
    entries = np.zeros(0x110000, dtype=np.int64)
    pool, widest = [], 0
    category = unicodedata.category
    for cp in range(0x110000):
        ch = chr(cp)
        if category(ch) in ("Cc", "Cf", "Co", "Cs") and ch not in "\t\n\r":
            continue
        out = normalize_char(ch, lowercase)
        widest = max(widest, len(out))
        if len(out) == 1:
            entries[cp] = (1 << 23) | (out[0][1] << 21) | ord(out[0][0])
        elif len(out) > 1:
            entries[cp] = (len(out) << 23) | len(pool)
            pool += [ord(c) | (k << 21) for c, k in out]
    if widest > MAX_EXPANSION:
        raise AssertionError(f"a code point normalises to {widest} characters; the kernel's buffer is sized for {MAX_EXPANSION}")
    if len(pool) >= 1 << 21:
        raise AssertionError("the expansion pool outgrew its 21-bit index")
    blocks, index = np.unique(entries.reshape(0x1100, 256), axis=0, return_inverse=True)
    return index.reshape(-1).astype(np.int32), blocks.astype(np.int32), np.asarray(pool or [0], dtype=np.int32)


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def piece_key(chars, cont):
    """the 32-bit key of a piece (a string without its "##") in keyspace `cont`, as csrc/wordpiece.hip computes it"""
    h = 0
    for c in chars:
        h = (h * HASH_P + ord(c) + 1) & 0xFFFFFFFF
    return _fmix32(h ^ ((len(chars) * 0x9E3779B1) & 0xFFFFFFFF) ^ (0x85EBCA6B if cont else 0))


def _read_vocab_file(path):
    with open(path, encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f]


class BertWordPieceTokenizer:
    """vocab: a vocab.txt path, a local directory that holds one (`do_lower_case` is then read from its tokenizer_config.json when there is one), or a
    list of tokens.  table_slots: the size of the device hash table (a power of two above the number of pieces; default: at least twice it)."""

    def __init__(self, vocab, lowercase=True, table_slots=None):
        if isinstance(vocab, (str, os.PathLike)):
            path = os.fspath(vocab)
            if os.path.isdir(path):
                cfg = os.path.join(path, "tokenizer_config.json")
                if os.path.exists(cfg):
                    with open(cfg) as f:
                        lowercase = bool(json.load(f).get("do_lower_case", lowercase))
                path = os.path.join(path, "vocab.txt")
            if not os.path.isfile(path):
                raise ValueError(f"BertWordPieceTokenizer: {os.fspath(vocab)!r} is neither a vocab.txt nor a directory that holds one.  Pass a local path: "
                                 "no network is used, so a hub name such as 'allenai/scibert_scivocab_uncased' is not downloaded")
            tokens = _read_vocab_file(path)
        else:
            tokens = [str(t) for t in vocab]
        self.lowercase = bool(lowercase)
        self.tokens = tokens
        self.vocab = {t: i for i, t in enumerate(tokens)}                       # a token listed twice keeps its last id, as a dict built from the file does
        for name in ("[CLS]", "[SEP]", "[UNK]"):
            if name not in self.vocab:
                raise ValueError(f"BertWordPieceTokenizer: the vocabulary has no {name} entry")
        self.cls_id, self.sep_id, self.unk_id = (self.vocab[t] for t in ("[CLS]", "[SEP]", "[UNK]"))
        self.pad_id = self.vocab.get("[PAD]", 0)
        # the two keyspaces: whole-word pieces, and the continuation pieces without their "##"
        self.pieces = ({t: i for t, i in self.vocab.items() if t and not t.startswith("##")}, {t[2:]: i for t, i in self.vocab.items() if len(t) > 2 and t.startswith("##")})
        self.max_piece_chars = min(max([len(t) for d in self.pieces for t in d] or [1]), MAX_WORD_CHARS)
        self.table_slots = table_slots
        self._norm, self._words, self._dev = {}, {}, {}

    # ------------------------------------------------------------------------------------------------------------ host
    def normalize(self, text):
        """[(character, kind)] of a text after the five steps"""
        norm, out = self._norm, []
        for ch in text:
            m = norm.get(ch)
            if m is None:
                m = norm[ch] = normalize_char(ch, self.lowercase)
            out += m
        return out

    def word_pieces(self, word):
        """the ids of one pre-tokenised word"""
        got = self._words.get(word)
        if got is not None:
            return got
        if len(word) > MAX_WORD_CHARS:
            ids = [self.unk_id]
        else:
            ids, start, n = [], 0, len(word)
            while start < n:
                table = self.pieces[1 if start else 0]
                end = min(n, start + self.max_piece_chars)
                while end > start and word[start:end] not in table:
                    end -= 1
                if end == start:
                    ids = [self.unk_id]
                    break
                ids.append(table[word[start:end]])
                start = end
        if len(self._words) >= 1 << 16:
            self._words.clear()
        self._words[word] = ids
        return ids

    def words(self, text):
        """the pre-tokenised words of a text"""
        out, cur = [], []
        for ch, kind in self.normalize(text):
            if kind == KIND_OTHER:
                cur.append(ch)
                continue
            if cur:
                out.append("".join(cur))
                cur = []
            if kind == KIND_SOLO:
                out.append(ch)
        if cur:
            out.append("".join(cur))
        return out

    def encode_all(self, texts, max_length=512):
        """(flat int64 [sum of lengths], offsets int64 [B + 1]): text b is flat[offsets[b]:offsets[b + 1]] = [CLS], at most max_length - 2 pieces, [SEP]"""
        if max_length < 2:
            raise ValueError("max_length must hold [CLS] and [SEP]")
        texts = _check_texts(texts)
        flat, off = [], [0]
        for text in texts:
            ids = [self.cls_id]
            for word in self.words(text):
                ids += self.word_pieces(word)
                if len(ids) > max_length - 2:
                    break
            del ids[max_length - 1:]
            ids.append(self.sep_id)
            flat += ids
            off.append(len(flat))
        return np.asarray(flat, dtype=np.int64), np.asarray(off, dtype=np.int64)

    # ------------------------------------------------------------------------------------------------------------ device
    def hash_table(self):
        """(slots int32 [n_slots, 4], chars int32 [n_chars]) of include/oneprot_hip.h "text input" """
        n = len(self.pieces[0]) + len(self.pieces[1])
        cap = 2
        while cap < 2 * n:
            cap *= 2
        if self.table_slots is not None:
            cap = int(self.table_slots)
            if cap < 2 or cap & (cap - 1) or cap <= n:
                raise ValueError(f"table_slots = {cap}: a power of two above the {n} pieces is needed (one slot stays empty)")
        slots = np.zeros((cap, 4), dtype=np.int64)
        slots[:, 3] = -1
        chars = []
        for cont, table in enumerate(self.pieces):
            for piece, idx in table.items():
                if len(piece) > MAX_WORD_CHARS:
                    continue                                    # can never match: a longer word is [UNK] before the search
                key = piece_key(piece, cont)
                s = key & (cap - 1)
                while slots[s, 3] >= 0:
                    s = (s + 1) & (cap - 1)
                slots[s] = (key - (1 << 32) if key >= 1 << 31 else key, len(chars), len(piece) | (cont << 16), idx)
                chars += map(ord, piece)
        return slots.astype(np.int32), np.asarray(chars or [0], dtype=np.int32)

    def _device_tables(self, device):
        t = self._dev.get(str(device))
        if t is None:
            index, entries, pool = norm_table(self.lowercase)
            slots, chars = self.hash_table()
            t = self._dev[str(device)] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (index, entries, pool, slots, chars))
        return t

    def encode_device(self, texts, max_length=512, device="cuda"):
        """(ids int32 [B, max_length] padded with the pad id, lengths int32 [B]) on `device`; nothing is read back"""
        from . import hip
        if not 2 <= max_length <= hip._consts["WORDPIECE_MAX_LENGTH"]:
            raise ValueError(f"max_length must lie in 2 .. {hip._consts['WORDPIECE_MAX_LENGTH']}")
        texts = _check_texts(texts)
        if not 1 <= len(texts) <= hip._consts["WORDPIECE_MAX_TEXTS"]:
            raise ValueError(f"a batch holds 1 .. {hip._consts['WORDPIECE_MAX_TEXTS']} texts")
        device = torch.device(device)
        raw = [t.encode("utf-8") for t in texts]
        offsets = torch.zeros(len(raw) + 1, dtype=torch.int64)
        offsets[1:] = torch.tensor([len(r) for r in raw], dtype=torch.int64).cumsum(0)
        n_bytes = int(offsets[-1])
        host = torch.zeros(max(n_bytes, 1), dtype=torch.uint8, pin_memory=device.type == "cuda")
        host.numpy()[:n_bytes] = np.frombuffer(b"".join(raw), dtype=np.uint8)
        with torch.cuda.device(device):
            index, entries, pool, slots, chars = self._device_tables(device)
            data, off_dev = host.to(device, non_blocking=True), offsets.to(device, non_blocking=True)
            ids = torch.empty(len(raw), max_length, dtype=torch.int32, device=device)
            lengths = torch.empty(len(raw), dtype=torch.int32, device=device)
            hip.call("oneprot_wordpiece_encode", data, off_dev, index, entries, pool, slots, chars, ids, lengths, offsets.data_ptr(), n_bytes, len(raw),
                     entries.shape[0], pool.numel(), slots.shape[0], chars.numel(), self.max_piece_chars, max_length, self.cls_id, self.sep_id, self.unk_id,
                     self.pad_id)
        self._last_host = host                 # the pinned source of an asynchronous copy stays alive until the next call
        return ids, lengths

    def _want_device(self, device, texts):
        if device is None:
            from . import hip
            if not (os.path.exists(hip.LIB_PATH) and torch.cuda.is_available()):
                return None
            if sum(map(len, texts)) < DEVICE_MIN_BYTES:                      # characters: a lower bound of the bytes, and free
                return None
            return torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        return None if device.type == "cpu" else device

    def __call__(self, texts, max_length=512, device=None, packed=False):
        """int64 [B, longest] padded with the pad id (0), what HF's call with padding=True, truncation=True gives; packed=True: a PackedTokens with that pad
        id.  On the GPU from the device path (device=None: for a batch of at least DEVICE_MIN_BYTES), on the CPU from the host rule."""
        texts = _check_texts(texts)
        dev = self._want_device(device, texts)
        if dev is None:
            flat, off = self.encode_all(texts, max_length)
            lens = np.diff(off)
            if packed:
                return PackedTokens.from_list([torch.from_numpy(flat[a:b]) for a, b in zip(off[:-1], off[1:])], pad_id=self.pad_id)
            out = np.full((lens.size, int(lens.max()) if lens.size else 0), self.pad_id, dtype=np.int64)
            out[np.arange(out.shape[1])[None, :] < lens[:, None]] = flat
            return torch.from_numpy(out)
        ids, lengths = self.encode_device(texts, max_length, dev)
        if not packed:
            return ids[:, :int(lengths.max())].to(torch.int64)               # the one readback: the width of the batch
        lens = lengths.tolist()                                              # a PackedTokens carries its lengths on the host
        total = sum(lens)
        keep = torch.arange(max_length, device=dev)[None, :] < lengths[:, None]
        stream = torch.full((-(-total // PAD_MULTIPLE) * PAD_MULTIPLE,), self.pad_id, dtype=torch.int64, device=dev)
        stream[:total] = ids[keep]
        cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
        cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
        return PackedTokens(stream, cu.to(dev), max(lens), lens, pad_id=self.pad_id)


def _check_texts(texts):
    texts = list(texts)
    for i, t in enumerate(texts):
        if not isinstance(t, str):
            raise ValueError(f"text {i} is a {type(t).__name__}; texts are strings")
        try:
            t.encode("utf-8")
        except UnicodeEncodeError:
            raise ValueError(f"text {i} holds a lone surrogate, which is no character and has no UTF-8 form") from None
    return texts


# ---- datasets' common parts (TextDataset here, StructTokenDataset and SequenceSimDataset in token_data.py) ---------------------------------------------------
def sequence_tokenizer(spec, extra_tokens=()):
    """the ESM tokenizer a dataset's `seq_tokenizer` names: a local vocab.txt, a local directory that holds one, or any other string (a hub name such as
    facebook/esm2_t33_650M_UR50D) for the built-in ESM-2 table; extra_tokens are appended, as `add_tokens` does"""
    from .collect import EsmSequenceTokenizer
    from .msa_data import MsaBatchConverter
    tokens = None
    if isinstance(spec, (str, os.PathLike)):
        path = os.fspath(spec)
        if os.path.isdir(path):
            path = os.path.join(path, "vocab.txt")
        if os.path.isfile(path):
            tokens = [t.strip() for t in _read_vocab_file(path)]
    if tokens is None:
        tokens = list(MsaBatchConverter.all_toks)
    return EsmSequenceTokenizer(tokens + [t for t in extra_tokens if t not in tokens])


def esm_side(tokenizer, sequences, max_length, packed=False):
    """the ESM side of a batch on the host: int64 [B, longest] padded with 1, or a PackedTokens"""
    if not packed:
        return tokenizer(sequences, max_length).long()
    flat, off = tokenizer.encode_all(sequences, max_length)
    return PackedTokens.from_list([torch.from_numpy(flat[a:b]) for a, b in zip(off[:-1], off[1:])], pad_id=tokenizer.pad_id)


def read_csv_rows(path):
    """the non-empty rows of a CSV file as lists of strings (Python's csv module: quoted fields may hold commas, quotes and line breaks)"""
    import csv
    with open(path, newline="", encoding="utf-8") as f:
        return [row for row in csv.reader(f) if row]


def as_str(value):
    return value.decode("utf-8") if isinstance(value, (bytes, np.bytes_)) else str(value)


def eval_len(split, rows):
    """the reference returns 1000 for val / test and then indexes past a shorter file; here the length is min(1000, rows)"""
    return rows if split == "train" else min(1000, rows)


class TextDataset(Dataset):
    """ref src/data/datasets/text_dataset.py:8-54, same constructor and return tuple.  `text_tokenizer` is a local vocab.txt or a local directory (there is
    no network); `seq_tokenizer` as sequence_tokenizer takes it.  `{split}_text.csv`: column 0 the id, column 1 the text, no header.  `h5_file` may be
    replaced after construction by an opened file or a nested mapping.  Attributes set after construction: `device` (None: the GPU for a batch of at
    least DEVICE_MIN_BYTES, "cpu": the host rule), `packed` (the ESM side as PackedTokens), `packed_text` (the text side as PackedTokens, pad id 0)."""

    def __init__(self, data_dir: str, split: str, max_length: int = 1024, text_max_length: int = 512, text_tokenizer: str = "allenai/scibert_scivocab_uncased",
                 seq_tokenizer: str = "facebook/esm2_t33_650M_UR50D"):
        self.text_max_length, self.max_length, self.split = text_max_length, max_length, split
        self.h5_file = f"{data_dir}/seqstruc.h5"
        csv_file = f"{data_dir}/{split}_text.csv"
        try:
            self.rows = read_csv_rows(csv_file)
        except FileNotFoundError:
            print(f"File not found: {csv_file}")
            self.rows = []
        self.first_row = {}
        for i, row in enumerate(self.rows):
            self.first_row.setdefault(row[0], i)
        self.text_tokenizer = BertWordPieceTokenizer(text_tokenizer)
        self.seq_tokenizer = sequence_tokenizer(seq_tokenizer)
        self.device, self.packed, self.packed_text = None, False, False

    def __len__(self) -> int:
        return eval_len(self.split, len(self.rows))

    def __getitem__(self, idx: int) -> str:
        return self.rows[idx][0]

    def collate_fn(self, data):
        """(sequence ids, text ids, "text", sequences): an id the structure file does not hold drops both sides of its pair"""
        from .graph_data import _open, _value
        sequences, texts = [], []
        file, opened = _open(self.h5_file)
        try:
            for seq_id in data:
                if seq_id not in self.first_row:
                    raise IndexError(f"{seq_id} is not in the text file")
                try:
                    sequence = as_str(_value(file[seq_id]["structure"]["0"]["A"]["residues"]["seq1"]))
                except KeyError:
                    print(f"KeyError: {seq_id} not found in {self.h5_file if isinstance(self.h5_file, str) else 'the structure file'}")
                    continue
                sequences.append(sequence)
                texts.append(self.rows[self.first_row[seq_id]][1])
        finally:
            if opened:
                file.close()
        text_input = self.text_tokenizer(texts, max_length=self.text_max_length, device=self.device, packed=self.packed_text)
        sequence_input = esm_side(self.seq_tokenizer, sequences, self.max_length, self.packed).to(text_input.device)
        return sequence_input, text_input, "text", sequences
