"""Embedding collection on the device: task CSVs -> the files the downstream probes start from (ref src/collect_embeddings.py, configs/collect_embeddings.yaml).

    <output_dir>/<task>/<split>/<task>_<split>_embeddings_labels.pt   {"embeddings": fp32 [N, D] ([N, 2D] for ppi), "labels_fitness": ...}, rows in CSV order

which is what downstream.load_data reads (with output_dir = <emb_dir>/<model_type>).  Five parts, each usable on its own:

  EsmSequenceTokenizer   the rule of HF's EsmTokenizer on the host, vectorised over a whole split: leftmost-longest match of vocabulary entries (specials
                         included), everything else between matches split at white space into one <unk> per chunk, <cls> ... <eos>, truncation to max_length
                         tokens with <eos> kept.  graph_data.tokenize_sequences (one byte, one id) is NOT this rule and stays as it is.
  read_task_csv          the reference's four label types from a CSV, by header, on Python's csv module.
  plan_batches           the UNIQUE sequences of a split in canonical order (token count, then bytes), filled greedily into token budgets.
  embed_sequences        (run_plan) every batch of the plan as one PackedTokens stream through the towers' existing kernels; the next batch's ids are staged from pinned
                         memory on a copy stream while the current one runs; nothing is read back per batch.  This module indexes, gathers and concatenates rows
                         and computes nothing on them.
  collect_task / main    the reference's two steps (shards, then the combined file) and its config keys; `--run` does both in one go.

There is no CPU path: a CPU encoder raises hip.HipKernelError, a missing library hip.HipLibraryMissing."""
import ast
import csv
import logging
import os
import re

import numpy as np
import torch

from . import hip
from . import layout
from .msa_data import MsaBatchConverter
from .packing import PackedTokens

logger = logging.getLogger(__name__)

MAX_LENGTH = 1024                   # ref collect_embeddings.py:86: truncation=True, max_length=1024
DEFAULT_MAX_TOKENS = 131072         # the smallest measured budget within 3 % of the best on every shape and split (tools/collect_ab.py)
DEFAULT_MAX_SEQS = 1024
LABEL_TYPES = ("classification", "ppi", "regression", "multi-label")
LABEL_COLUMN = "label/fitness"
CONFIG_KEYS = ("models", "tasks", "esm_model", "tokenizer_name", "saprot_model", "output_dir", "batch_size", "single_batch_mode", "huggingface",
               "num_workers", "num_gpus", "num_nodes")          # the last three: accepted and ignored on one device
SAPROT_REASON = ("saprot: the SaProt tower reads a 446-token structure-aware vocabulary that is not available here, so its tokenizer cannot be pinned "
                 "against the reference's; embeddings of it are not built")
_SPACE_BYTES = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"              # what str.split() splits at, within ASCII
_SHARD = re.compile(r"embeddings_rank(\d+)_batch(\d+)\.pt$")


# ---- 1. tokenizer ---------------------------------------------------------------------------------------------------------------------------------------
class EsmSequenceTokenizer:
    """HF EsmTokenizer's rule.  vocab: None (the ESM-2 table of msa_data.MsaBatchConverter), a path to a vocab.txt (one token per line) or a list of tokens.

    The common path -- every byte a one-letter token, an out-of-vocabulary byte or white space -- is array code over the concatenated split.  A sequence that
    holds the first character of a longer vocabulary entry (`<` for ESM-2) or a non-ASCII character is matched on its own by `_encode_one`."""

    def __init__(self, vocab=None):
        if vocab is None:
            tokens = list(MsaBatchConverter.all_toks)
        elif isinstance(vocab, (str, os.PathLike)):
            with open(vocab) as f:
                tokens = [line.strip() for line in f.read().splitlines()]
        else:
            tokens = [str(t) for t in vocab]
        self.tokens = tokens
        self.token_to_id = {t: i for i, t in enumerate(tokens)}
        for name in ("<cls>", "<pad>", "<eos>", "<unk>"):
            if name not in self.token_to_id:
                raise ValueError(f"EsmSequenceTokenizer: the vocabulary has no {name} entry")
        self.cls_id, self.pad_id, self.eos_id, self.unk_id = (self.token_to_id[t] for t in ("<cls>", "<pad>", "<eos>", "<unk>"))
        self._table = np.full(256, -1, dtype=np.int64)          # one-letter ASCII entries
        self._slow = np.zeros(256, dtype=bool)                  # bytes that send a sequence to _encode_one
        self._slow[128:] = True
        for t, i in self.token_to_id.items():
            if len(t) == 1 and ord(t) < 128:
                self._table[ord(t)] = i
            elif t:
                self._slow[t.encode("utf-8")[0]] = True
        self._slow_in_table = bool((self._slow & (self._table >= 0)).any())         # a one-letter entry that also starts a longer one (never in ESM-2's table)
        self._space = np.zeros(256, dtype=bool)
        self._space[list(_SPACE_BYTES)] = True
        self._space &= self._table < 0
        entries = sorted((t for t in self.token_to_id if t), key=len, reverse=True)         # alternation order: the longest entry at a position wins
        self._match = re.compile("|".join(re.escape(t) for t in entries))

    def _encode_one(self, s):
        """the body ids (no <cls> / <eos>, not truncated) of one string, by the rule itself"""
        out, pos, unk = [], 0, self.unk_id
        for m in self._match.finditer(s):
            out += [unk] * len(s[pos:m.start()].split())
            out.append(self.token_to_id[m.group()])
            pos = m.end()
        out += [unk] * len(s[pos:].split())
        return out

    def encode_all(self, sequences, max_length=MAX_LENGTH):
        """(flat int64 [sum of lengths], offsets int64 [B + 1]): sequence b is flat[offsets[b]:offsets[b + 1]] = <cls> body <eos>, at most max_length ids"""
        if max_length < 2:
            raise ValueError("max_length must hold <cls> and <eos>")
        sequences = list(sequences)
        n = len(sequences)
        if any(not isinstance(s, str) for s in sequences):
            raise ValueError("EsmSequenceTokenizer: sequences are strings")
        joined = "".join(sequences)
        own = {}                                                 # index -> body ids of the sequences matched on their own
        if not joined.isascii():
            for i, s in enumerate(sequences):
                if not s.isascii():
                    own[i] = self._encode_one(s)
                    sequences[i] = ""
            joined = "".join(sequences)
        raw = np.frombuffer(joined.encode("ascii"), dtype=np.uint8)
        lens = np.fromiter(map(len, sequences), dtype=np.int64, count=n)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        ids = self._table[raw]
        valid = ids >= 0
        if valid.all() and not (self._slow_in_table and self._slow[raw].any()):         # the common path: every byte is a one-letter entry
            tok, counts = ids, lens
        else:
            oov = ~valid & ~self._space[raw]
            slow = self._slow[raw]
            seq_of = None
            if slow.any():
                seq_of = np.repeat(np.arange(n), lens)
                for i in np.unique(seq_of[slow]).tolist():
                    own[i] = self._encode_one(sequences[i])
            prev = np.zeros_like(oov)
            prev[1:] = oov[:-1]
            prev[off[:-1][lens > 0]] = False                     # a run of out-of-vocabulary bytes ends with its sequence
            keep = valid | (oov & ~prev)                         # one <unk> per run; white space is dropped
            if seq_of is not None:
                gone = np.zeros(n, dtype=bool)
                gone[list(own)] = True
                keep &= ~gone[seq_of]
            c = np.zeros(raw.size + 1, dtype=np.int64)
            np.cumsum(keep, out=c[1:])
            counts = c[off[1:]] - c[off[:-1]]
            tok = np.where(valid, ids, self.unk_id)[keep]
        body = np.minimum(counts, max_length - 2)
        out_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(body + 2, out=out_off[1:])
        flat = np.empty(int(out_off[-1]), dtype=np.int64)
        flat[out_off[:-1]] = self.cls_id
        flat[out_off[1:] - 1] = self.eos_id
        tok_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=tok_off[1:])
        t = np.arange(tok.size, dtype=np.int64)
        sel = t - np.repeat(tok_off[:-1], counts) < np.repeat(body, counts)
        flat[(t + np.repeat(out_off[:-1] + 1 - tok_off[:-1], counts))[sel]] = tok[sel]
        if own:
            pieces, sizes, last = [], body + 2, 0
            for i in sorted(own):
                b = np.asarray(own[i][:max_length - 2], dtype=np.int64)
                pieces += [flat[out_off[last]:out_off[i]], [self.cls_id], b, [self.eos_id]]
                sizes[i] = b.size + 2
                last = i + 1
            pieces.append(flat[out_off[last]:])
            flat = np.concatenate([np.asarray(p, dtype=np.int64) for p in pieces])
            out_off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(sizes, out=out_off[1:])
        return flat, out_off

    def __call__(self, sequences, max_length=MAX_LENGTH):
        """host int64 [B, L], right-padded with the pad id (1), L the longest row: the tokenizer call of ref collect_embeddings.py:81-87"""
        flat, off = self.encode_all(sequences, max_length)
        lens = np.diff(off)
        if lens.size == 0:
            return torch.empty(0, 0, dtype=torch.int64)
        out = np.full((lens.size, int(lens.max())), self.pad_id, dtype=np.int64)
        out[np.arange(out.shape[1])[None, :] < lens[:, None]] = flat
        return torch.from_numpy(out)


# ---- 2. CSV reader --------------------------------------------------------------------------------------------------------------------------------------
def split_of(path):
    """ref collect_embeddings.py:207-215: train / valid / test by substring of the lower-cased file name, tested in that order"""
    name = os.path.basename(str(path)).lower()
    for split in ("train", "valid", "test"):
        if split in name:
            return split
    raise ValueError(f"Unable to determine split from filename: {path}")


def read_task_csv(path, label_type):
    """(columns, labels) of a task CSV (ref SequenceDataset, collect_embeddings.py:29-67, without pandas).  columns: one list of strings per sequence column
    (`sequence`; `sequence_1`, `sequence_2` for ppi), in file order; labels from `label/fitness`: int64 [N] (classification, ppi), float32 [N] (regression),
    int32 [N, C] (multi-label: each cell a Python list literal)."""
    if label_type not in LABEL_TYPES:
        raise ValueError(f"Unsupported label_type: {label_type!r}; one of {', '.join(LABEL_TYPES)}")
    with open(path, newline="", encoding="utf-8-sig") as f:
        reader = csv.reader(f)
        header = next(reader, None)
        if header is None:
            raise ValueError(f"{path}: empty file")
        names = ("sequence_1", "sequence_2") if label_type == "ppi" else ("sequence",)
        where = []
        for name in names + (LABEL_COLUMN,):
            if name not in header:
                raise ValueError(f"{path}: no column {name!r} (label_type {label_type!r}); the header is {header}")
            where.append(header.index(name))
        rows = []
        for row in reader:
            if not row:                     # a blank line, as pandas skips it
                continue
            if len(row) <= max(where):
                raise ValueError(f"{path}, line {reader.line_num}: {len(row)} fields, the header has {len(header)}")
            rows.append(row)
    columns = tuple([row[i] for row in rows] for i in where[:-1])
    cells = [row[where[-1]] for row in rows]
    try:
        if label_type == "regression":
            labels = torch.from_numpy(np.asarray(cells, dtype=np.float64).astype(np.float32).reshape(len(cells)))
        elif label_type == "multi-label":
            lists = [ast.literal_eval(c) for c in cells]
            widths = {len(v) if isinstance(v, (list, tuple)) else -1 for v in lists}
            if len(widths) > 1 or -1 in widths:
                raise ValueError(f"{path}: ragged multi-label rows (list lengths {sorted(widths)}; -1: not a list)")
            labels = torch.from_numpy(np.asarray(lists, dtype=np.int32).reshape(len(lists), -1))
        else:
            try:
                arr = np.asarray(cells, dtype=np.int64)
            except ValueError:              # "1.0": a float column, truncated as torch.tensor(..., dtype=torch.long) truncates it
                arr = np.asarray(cells, dtype=np.float64).astype(np.int64)
            labels = torch.from_numpy(arr.reshape(len(cells)))
    except (SyntaxError, TypeError) as e:
        raise ValueError(f"{path}: column {LABEL_COLUMN!r} does not parse as {label_type} labels ({e})") from None
    return columns, labels


# ---- 3. plan --------------------------------------------------------------------------------------------------------------------------------------------
def unique_sequences(*columns):
    """(the distinct strings of all columns together, sorted by bytes; per column an int64 array: the row's index into them)"""
    uniq = sorted(set().union(*columns), key=lambda s: s.encode("utf-8"))
    index = {s: i for i, s in enumerate(uniq)}
    return uniq, tuple(np.fromiter((index[s] for s in col), dtype=np.int64, count=len(col)) for col in columns)


def plan_batches(lengths, max_tokens, max_seqs, keys=None, max_length=MAX_LENGTH):
    """Batches of the unique sequences of a split: a list of lists of indices into `lengths` (token counts, <cls> and <eos> included).  Canonical order -- by
    token count, then by `keys` (the sequences' bytes; None: the input is already sorted by them) -- filled greedily: a batch is closed when the next sequence
    would take its token sum past max_tokens or its size past max_seqs.  The batches are a function of the set of sequences, not of the file's order."""
    if max_tokens < max_length:
        raise ValueError(f"plan_batches: max_tokens {max_tokens} is below max_length {max_length}: the longest sequence would fit no batch")
    if max_seqs < 1:
        raise ValueError("plan_batches: max_seqs must be at least 1")
    lengths = [int(n) for n in lengths]
    if any(n > max_tokens or n < 1 for n in lengths):
        raise ValueError(f"plan_batches: every sequence holds between 1 and max_tokens = {max_tokens} tokens")
    if keys is None:
        order = sorted(range(len(lengths)), key=lengths.__getitem__)
    else:
        keys = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
        order = sorted(range(len(lengths)), key=lambda i: (lengths[i], keys[i]))
    batches, cur, tokens = [], [], 0
    for i in order:
        if cur and (tokens + lengths[i] > max_tokens or len(cur) == max_seqs):
            batches.append(cur)
            cur, tokens = [], 0
        cur.append(i)
        tokens += lengths[i]
    if cur:
        batches.append(cur)
    return batches


def plan_sequences(sequences, max_length=MAX_LENGTH, max_tokens=None, max_seqs=None, tokenizer=None):
    """What embed_sequences runs for `sequences`: dict(uniq: the distinct strings sorted by bytes, inverse: int64 [N] row -> index into uniq, flat / off: their
    ragged ids, batches: plan_batches over them (lists of indices into uniq), pad_id)"""
    tok = tokenizer if tokenizer is not None else EsmSequenceTokenizer()
    max_tokens = DEFAULT_MAX_TOKENS if max_tokens is None else int(max_tokens)
    max_seqs = DEFAULT_MAX_SEQS if max_seqs is None else int(max_seqs)
    if max_tokens < max_length:
        raise ValueError(f"max_tokens {max_tokens} is below max_length {max_length}: the longest sequence would fit no batch")
    uniq, (inverse,) = unique_sequences(list(sequences))
    flat, off = tok.encode_all(uniq, max_length)
    return dict(uniq=uniq, inverse=inverse, flat=flat, off=off, batches=plan_batches(np.diff(off), max_tokens, max_seqs, max_length=max_length),
                pad_id=tok.pad_id)


# ---- 4. embedding ---------------------------------------------------------------------------------------------------------------------------------------
class _MeanMode:
    mode = 0          # layout.pool_fwd's masked mean over the non-pad tokens of a segment, <cls> and <eos> included


def _stage(flat, off, lo, hi, dev, copy_stream, pad_id):
    """the PackedTokens of canonical sequences lo .. hi-1, built in pinned memory and copied on the copy stream; T_pad and the attention work table are what
    PackedTokens.from_list gives for these sequences"""
    lens = np.diff(off[lo:hi + 1])
    total = int(off[hi] - off[lo])
    T = -(-total // 256) * 256
    ids = torch.empty(T, dtype=torch.int64, pin_memory=True)
    ids[:total] = torch.from_numpy(flat[off[lo]:off[hi]])
    ids[total:] = pad_id
    cu = torch.empty(lens.size + 1, dtype=torch.int32, pin_memory=True)
    cu[0] = 0
    cu[1:] = torch.from_numpy(np.cumsum(lens).astype(np.int32))
    with torch.cuda.stream(copy_stream):
        p = PackedTokens(ids.to(dev, non_blocking=True), cu.to(dev, non_blocking=True), int(lens.max()), lens.tolist(), pad_id)
        work = p.attn_work()
        done = copy_stream.record_event()
    return p, work, done


def embed_sequences(encoder, sequences, kind, max_length=MAX_LENGTH, max_tokens=None, max_seqs=None, tokenizer=None, timings=None):
    """fp32 [N, D] on the encoder's device, row i the embedding of sequences[i].

    kind "oneprot": the encoder's own output (pooling, head and norm: what `model.network["sequence"]` returns); "esm2": the reference's baseline, the masked
    mean of the tower's last_hidden_state over the non-pad tokens, width hidden_size (the tower's fused final-LayerNorm + pooling entry; `encoder` is an
    EsmTransformer or an encoder that holds one as `.transformer`); "saprot": NotImplementedError.  Every distinct sequence is embedded once and gathered.  The
    encoder runs in eval mode under no_grad; its modules' training flags are put back afterwards.  timings: a list that receives one (start, end) pair of
    timing events per batch (tools/collect_ab.py reads the device's idle time between batches from them); None records nothing."""
    if kind == "saprot":
        raise NotImplementedError(SAPROT_REASON)
    if kind not in ("oneprot", "esm2"):
        raise ValueError(f"embed_sequences: kind {kind!r}; one of 'oneprot', 'esm2', 'saprot'")
    sequences = list(sequences)
    if not sequences:
        raise ValueError("embed_sequences: no sequences")
    dev = next(encoder.parameters()).device
    if dev.type != "cuda":
        raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback (move the encoder to the device)")
    hip.lib()                                                   # HipLibraryMissing before any device work
    plan = plan_sequences(sequences, max_length, max_tokens, max_seqs, tokenizer)
    tr = getattr(encoder, "transformer", encoder)
    if kind == "oneprot":
        forward = encoder
    else:
        def forward(p):
            x, _ = tr.run_layers(p, save=False)
            return layout.of(tr, p).pool_fwd(tr, x, _MeanMode, False)[0]
    return run_plan(encoder, forward, plan, dev, timings)


def run_plan(encoder, forward, plan, dev, timings=None):
    """fp32 [N, D] on `dev`: every batch of `plan` (plan_sequences' dict: uniq, inverse, flat / off, batches, pad_id) as one PackedTokens stream through
    forward(p) -> [len(batch), D], written into a resident [U, D] buffer and gathered to the rows of plan["inverse"].  The next batch's ids are staged from
    pinned memory on a copy stream while the current one runs; nothing is read back.  `encoder` is put in eval mode, under no_grad, and its modules'
    training flags are put back afterwards.  embed_sequences and evaluate.embed_modalities (any tokenizer, any pad id) both end here."""
    uniq, inverse, flat, off, batches, pad_id = (plan[k] for k in ("uniq", "inverse", "flat", "off", "batches", "pad_id"))
    lengths = np.diff(off)
    order = np.fromiter((i for b in batches for i in b), dtype=np.int64, count=len(uniq))
    # the ragged ids in canonical order: every batch is one slice
    c_off = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum(lengths[order], out=c_off[1:])
    t = np.arange(flat.size, dtype=np.int64)
    c_flat = flat[t + np.repeat(off[:-1][order] - c_off[:-1], lengths[order])]
    bounds = np.zeros(len(batches) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in batches], out=bounds[1:])
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    flags = [(m, m.training) for m in encoder.modules()]
    main, copy_stream = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    out = None
    encoder.eval()
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            rows = torch.empty(len(inverse), dtype=torch.int64, pin_memory=True)
            rows.copy_(torch.from_numpy(rank[inverse]))
            rows = rows.to(dev, non_blocking=True)
            staged = _stage(c_flat, c_off, int(bounds[0]), int(bounds[1]), dev, copy_stream, pad_id)
            for b in range(len(batches)):
                p, work, done = staged
                main.wait_event(done)
                for tns in (p.ids, p.cu_seqlens, work):
                    tns.record_stream(main)
                if timings is not None:
                    timings.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    timings[-1][0].record(main)
                feats = forward(p)
                if out is None:
                    out = torch.empty(len(uniq), feats.shape[1], dtype=torch.float32, device=dev)
                out[int(bounds[b]):int(bounds[b + 1])] = feats
                if timings is not None:
                    timings[-1][1].record(main)
                if b + 1 < len(batches):                        # staged while batch b runs
                    staged = _stage(c_flat, c_off, int(bounds[b + 1]), int(bounds[b + 2]), dev, copy_stream, pad_id)
            return out.index_select(0, rows)
    finally:
        for m, flag in flags:
            m.training = flag


# ---- 5. files -------------------------------------------------------------------------------------------------------------------------------------------
def _tokenizer_of(cfg):
    """cfg.tokenizer_name: a vocab.txt, or a directory that holds one (a local HF tokenizer directory), is read; a hub name stands for the ESM-2 table"""
    name = cfg.get("tokenizer_name")
    if name:
        for cand in (str(name), os.path.join(str(name), "vocab.txt")):
            if os.path.isfile(cand):
                return EsmSequenceTokenizer(cand)
    return EsmSequenceTokenizer()


def load_model(cfg, model_cfg, device="cuda"):
    """(encoder on the device, kind) of one entry of cfg.models (ref collect_embeddings.py:137-170, 231-245)"""
    name = model_cfg["name"]
    if name == "saprot":
        raise NotImplementedError(SAPROT_REASON)
    if name == "esm2":
        from .esm import EsmTransformer
        return EsmTransformer.from_pretrained(cfg["esm_model"], add_pooling_layer=False).to(device).eval(), "esm2"
    return load_module(model_cfg.get("config_path"), model_cfg.get("ckpt_path"), plain_state_dict=bool(cfg.get("huggingface"))).network["sequence"].to(device).eval(), "oneprot"


def load_module(config_path, ckpt_path=None, plain_state_dict=False):
    """the whole module of a run: `config_path` composed, its `model` instantiated, `ckpt_path` (None: no weights are loaded) loaded strictly -- the
    ["state_dict"] of a Lightning checkpoint, or the file itself when plain_state_dict.  On the host; load_model here and evaluate.load_custom_model move it."""
    from . import config as config_mod
    if not config_path or not os.path.exists(config_path):
        raise FileNotFoundError(f"Model config file not found: {config_path}")
    composed = config_mod.compose(os.path.dirname(os.path.abspath(config_path)), os.path.basename(config_path))
    model = config_mod.instantiate(composed["model"])
    if ckpt_path is not None:
        sd = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        model.load_state_dict(sd if plain_state_dict else sd["state_dict"], strict=True)
    return model


def _dirs(cfg, model_cfg, task, csv_file):
    split = split_of(csv_file)
    base = os.path.join(str(cfg["output_dir"]).format(model_name=model_cfg["name"]), task, split)
    return split, base, os.path.join(base, "single_embs"), os.path.join(base, f"{task}_{split}_embeddings_labels.pt")


def write_shards(shard_dir, embeddings, labels, batch_size):
    """the reference's shards (collect_embeddings.py:127-135): embeddings_rank0_batch{i}.pt, each batch_size consecutive rows; shards of an earlier run go"""
    os.makedirs(shard_dir, exist_ok=True)
    for name in os.listdir(shard_dir):
        if _SHARD.match(name):
            os.remove(os.path.join(shard_dir, name))
    emb, labels = embeddings.detach().cpu(), labels.detach().cpu()
    n = emb.shape[0]
    for i, lo in enumerate(range(0, n, batch_size)):
        torch.save({"embeddings": emb[lo:lo + batch_size].clone(), "labels_fitness": labels[lo:lo + batch_size].clone()},
                   os.path.join(shard_dir, f"embeddings_rank0_batch{i}.pt"))
    return -(-n // batch_size)


def combine_shards(shard_dir, output_file):
    """ref combine_embeddings_for_split (collect_embeddings.py:172-198), the shards in numeric (rank, batch) order; False when there is nothing to combine"""
    found = sorted((int(m.group(1)), int(m.group(2)), name) for name in (os.listdir(shard_dir) if os.path.isdir(shard_dir) else ())
                   for m in [_SHARD.match(name)] if m)
    if not found:
        logger.info(f"No single embeddings found in {shard_dir}. Skipping collection.")
        return False
    parts = [torch.load(os.path.join(shard_dir, name), map_location="cpu", weights_only=True) for _, _, name in found]
    both = {"embeddings": torch.cat([p["embeddings"] for p in parts], dim=0).float().contiguous(),
            "labels_fitness": torch.cat([p["labels_fitness"] for p in parts], dim=0).contiguous()}
    torch.save(both, output_file)
    logger.info(f"Combined embeddings saved to {output_file}: embeddings {tuple(both['embeddings'].shape)}, labels {tuple(both['labels_fitness'].shape)}")
    return True


def collect_task(cfg, model_cfg, task, csv_file, both=False, model=None):
    """One CSV of one task for one model.  cfg.single_batch_mode true: embed and write the shards; false: combine a shard directory (ours, or one the
    reference wrote) into the combined file; both=True: the two steps in one go.  model: (encoder, kind) from load_model, loaded here when None.  Returns the
    combined file's path, or None when none was written."""
    label_type = cfg["tasks"][task]["label_type"]
    split, _, shard_dir, output_file = _dirs(cfg, model_cfg, task, csv_file)
    if both or cfg.get("single_batch_mode"):
        encoder, kind = model if model is not None else load_model(cfg, model_cfg)
        columns, labels = read_task_csv(csv_file, label_type)
        logger.info(f"Embedding task {task}, split {split}: {len(labels)} rows of {csv_file}")
        stacked = embed_sequences(encoder, [s for col in columns for s in col], kind, max_tokens=cfg.get("max_tokens"), max_seqs=cfg.get("max_seqs"),
                                  tokenizer=_tokenizer_of(cfg))          # both ppi columns in one plan: a protein is embedded once per split
        n = len(labels)
        emb = torch.cat([stacked[i * n:(i + 1) * n] for i in range(len(columns))], dim=1) if len(columns) > 1 else stacked
        write_shards(shard_dir, emb, labels, int(cfg.get("batch_size", 32)))
        if not both:
            return None
    return output_file if combine_shards(shard_dir, output_file) else None


def main(argv=None, default_config=None):
    """python src/collect_embeddings.py [--config configs/collect_embeddings.yaml] [--run] [key=value ...]"""
    import argparse
    import yaml
    from . import config as config_mod
    if default_config is None:
        default_config = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "collect_embeddings.yaml")
    ap = argparse.ArgumentParser(description="task CSVs -> <output_dir>/<task>/<split>/<task>_<split>_embeddings_labels.pt on the HIP towers")
    ap.add_argument("--config", default=default_config)
    ap.add_argument("--run", action="store_true", help="embed and combine in one go, whatever single_batch_mode says")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    cfg = config_mod.compose(os.path.dirname(os.path.abspath(args.config)), os.path.basename(args.config), resolve=False)
    for ov in args.overrides:
        key, _, value = ov.partition("=")
        node, parts = cfg, key.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = yaml.safe_load(value)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    written = []
    for model_cfg in cfg["models"]:
        logger.info(f"Processing model: {model_cfg['name']}")
        model = load_model(cfg, model_cfg) if (args.run or cfg.get("single_batch_mode")) else None
        for task, task_cfg in cfg["tasks"].items():
            for csv_file in task_cfg["csv_files"]:
                path = collect_task(cfg, model_cfg, task, csv_file, both=args.run, model=model)
                if path is not None:
                    written.append(path)
    return written
