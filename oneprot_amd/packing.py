"""Packed (variable-length) batches of token ids (ESM towers and the BERT text tower): the flash-attention "varlen" layout.

A packed batch is a token stream: the N sequences of a batch concatenated, each with its own <cls> ... <eos> ([CLS] ... [SEP] for a caption), the
tail filled with the pad id up to T_pad (a multiple of 256, which keeps the 8-phase GEMMs eligible).  `cu_seqlens` int32 [N + 1] marks where each
sequence starts.  Every row-wise stage of a tower (LayerNorm, the QKV / out-proj / FFN GEMMs and their epilogues, the LoRA branch, BERT's hidden
dropouts) runs on the T_pad rows as if they were one sequence; embedding, positions (rotary tables for ESM, absolute positions for BERT), attention
and pooling follow the segments (DESIGN.md sections 3 and 6).  Against a padded [B, L] batch this saves the rows of padding, which in shuffled real
data (ref struct_token_dataset.py:87-88, lengths up to 1 024; ref text_dataset.py:51, captions padded to the longest of the batch, up to 512) is a
large share of every batch.

`SequenceEncoder` / `StructTokenEncoder` / `TextEncoder` / `OneProtLitModule` take a PackedTokens wherever they take padded ids and return [N, D]
features in sequence order.  The stream's pad id must be the tower's: 1 for ESM (the default here), 0 for BERT
(`PackedTokens.from_padded(ids, pad_id=0)`); the text tower refuses a stream packed with another pad id.
"""
import torch

MAX_SEGMENT = 1026          # ESM-2's max_position_embeddings: the longest sequence (<cls> and <eos> included) the rotary tables are built for
                            # (the BERT tower enforces its own, smaller max_position_embeddings -- 512 -- when it is handed a stream)
PAD_MULTIPLE = 256


def _round_up(n, m):
    return -(-n // m) * m


class PackedTokens:
    """ids int64 [T_pad], cu_seqlens int32 [N + 1], max_len; `lengths` (host ints) travel with it so that nothing has to be read back from the
    device to schedule the kernels."""

    def __init__(self, ids, cu_seqlens, max_len, lengths=None, pad_id=1):
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype != torch.int64:
            raise ValueError(f"PackedTokens.ids must be a 1-D int64 tensor, got {getattr(ids, 'dtype', type(ids))} of shape {tuple(getattr(ids, 'shape', ()))}")
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dim() != 1 or cu_seqlens.dtype != torch.int32 or cu_seqlens.numel() < 2:
            raise ValueError("PackedTokens.cu_seqlens must be a 1-D int32 tensor with at least two entries")
        if lengths is None:
            c = cu_seqlens.detach().cpu().tolist()
            lengths = [b - a for a, b in zip(c[:-1], c[1:])]
        lengths = [int(n) for n in lengths]
        if len(lengths) != cu_seqlens.numel() - 1:
            raise ValueError("PackedTokens: lengths and cu_seqlens disagree")
        _check_lengths(lengths)
        if ids.numel() % PAD_MULTIPLE or ids.numel() < sum(lengths):
            raise ValueError(f"PackedTokens: T_pad = {ids.numel()} must be a multiple of {PAD_MULTIPLE} and hold all {sum(lengths)} tokens")
        self.ids, self.cu_seqlens, self.lengths, self.pad_id = ids, cu_seqlens, lengths, int(pad_id)
        self.max_len = int(max_len)
        if self.max_len != max(lengths):
            raise ValueError(f"PackedTokens: max_len {max_len} is not the longest segment ({max(lengths)})")
        self._work = {}

    # ---------------------------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_list(cls, seqs, pad_id=1, t_pad=None, device=None):
        """from a list of 1-D int id tensors (each a whole sequence: <cls> ... <eos>); t_pad: a larger stream length (multiple of 256)"""
        seqs = list(seqs)
        if not seqs:
            raise ValueError("PackedTokens.from_list: no sequences")
        for i, s in enumerate(seqs):
            if not isinstance(s, torch.Tensor) or s.dim() != 1:
                raise ValueError(f"PackedTokens.from_list: sequence {i} is not a 1-D tensor")
            if s.dtype.is_floating_point or s.dtype.is_complex or s.dtype == torch.bool:
                raise ValueError(f"PackedTokens.from_list: sequence {i} has dtype {s.dtype}; token ids are integers")
        lengths = [int(s.numel()) for s in seqs]
        _check_lengths(lengths)
        total = sum(lengths)
        T = _round_up(total, PAD_MULTIPLE)
        if t_pad is not None:
            if t_pad < total or t_pad % PAD_MULTIPLE:
                raise ValueError(f"PackedTokens: t_pad {t_pad} must be a multiple of {PAD_MULTIPLE} and >= {total}")
            T = int(t_pad)
        dev = seqs[0].device if device is None else torch.device(device)
        ids = torch.full((T,), int(pad_id), dtype=torch.int64, device=dev)
        ids[:total] = torch.cat([s.to(device=dev, dtype=torch.int64) for s in seqs])
        cu = torch.zeros(len(lengths) + 1, dtype=torch.int32)
        cu[1:] = torch.tensor(lengths, dtype=torch.int32).cumsum(0)
        return cls(ids, cu.to(dev), max(lengths), lengths, pad_id)

    @classmethod
    def from_padded(cls, ids, pad_id=1, t_pad=None):
        """from a right-padded [B, L] id tensor: row b contributes its tokens before the first pad (a row must not be all padding)"""
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
            raise ValueError("PackedTokens.from_padded needs a 2-D [B, L] id tensor")
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise ValueError(f"PackedTokens.from_padded: ids have dtype {ids.dtype}; token ids are integers")
        valid = (ids != pad_id).cpu()
        lengths = valid.sum(1).tolist()
        rows = [ids[b, :int(n)] for b, n in enumerate(lengths)]
        return cls.from_list(rows, pad_id=pad_id, t_pad=t_pad)

    # ---------------------------------------------------------------------------------------------------------- container protocol
    def __len__(self):
        return len(self.lengths)

    @property
    def T_pad(self):
        return self.ids.numel()

    @property
    def n_tokens(self):
        return sum(self.lengths)

    @property
    def device(self):
        return self.ids.device

    @property
    def is_cuda(self):
        return self.ids.is_cuda

    def to(self, device, non_blocking=False):
        out = PackedTokens.__new__(PackedTokens)
        out.__dict__.update(self.__dict__)
        out.ids = self.ids.to(device, non_blocking=non_blocking)
        out.cu_seqlens = self.cu_seqlens.to(device, non_blocking=non_blocking)
        out._work = {}
        return out

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def unpack(self):
        """the sequences as a list of 1-D id tensors"""
        c = [0]
        for n in self.lengths:
            c.append(c[-1] + n)
        return [self.ids[a:b] for a, b in zip(c[:-1], c[1:])]

    def to_padded(self, L=None):
        """[N, L] right-padded form (L defaults to max_len)"""
        L = self.max_len if L is None else int(L)
        out = torch.full((len(self), L), self.pad_id, dtype=torch.int64, device=self.ids.device)
        for b, s in enumerate(self.unpack()):
            out[b, :s.numel()] = s
        return out

    def attn_work(self, block=128):
        """int32 [n_work, 2] (segment, block) items of the varlen attention kernels, longest segment first (one long segment must not finish alone
        at the end of a launch); built once per batch and device"""
        key = (block, str(self.ids.device))
        w = self._work.get(key)
        if w is None:
            order = sorted(range(len(self.lengths)), key=lambda b: -self.lengths[b])
            items = [(b, j) for b in order for j in range(-(-self.lengths[b] // block))]
            w = self._work[key] = torch.tensor(items, dtype=torch.int32).to(self.ids.device)
        return w

    def __repr__(self):
        return f"PackedTokens(N={len(self)}, T_pad={self.T_pad}, tokens={self.n_tokens}, max_len={self.max_len}, device={self.ids.device})"


def _check_lengths(lengths):
    for i, n in enumerate(lengths):
        if n <= 0:
            raise ValueError(f"PackedTokens: sequence {i} is empty")
        if n > MAX_SEGMENT:
            raise ValueError(f"PackedTokens: sequence {i} has {n} tokens; ESM-2's rotary / position limit is {MAX_SEGMENT}")


def is_packed(x):
    return isinstance(x, PackedTokens)


def batch_size(x):
    """N of a packed batch, B of a padded one"""
    return len(x) if isinstance(x, PackedTokens) else int(x.shape[0])
