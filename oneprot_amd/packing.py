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


class PackedMsa:
    """A ragged batch of MSAs, each at its own depth and length (the MSA tower's packed input).

    ids int64 [T_pad] (T_pad a multiple of 256, the tail filled with the pad id): MSA b is a dense R_b x L_b block at t = cu_tokens[b] + r * L_b + l.
    Only geometry is cut -- an MSA's trailing all-pad rows and columns; a block may still hold pad ids (interior holes, a shorter row 0).
    cu_tokens int32 [N + 1] on the ids' device; `shapes` [(R_b, L_b)] host ints, so that no launch needs a read-back; `padded_shape` (R, L): the padded
    batch the stream stands for (default: the largest R_b and L_b) -- R is the row count of the published row-attention scale hd^-1/2 / sqrt(R), L the
    column stride of the column-attention dropout stream.  The cut is exact: the tower computes, at every position of a block, what it computes there on
    the padded batch (include/oneprot_hip.h, the ragged MSA entry points)."""

    def __init__(self, ids, cu_tokens, shapes, padded_shape=None, pad_id=1):
        from . import hip
        if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype != torch.int64:
            raise ValueError(f"PackedMsa.ids must be a 1-D int64 tensor, got {getattr(ids, 'dtype', type(ids))} of shape {tuple(getattr(ids, 'shape', ()))}")
        shapes = [(int(r), int(l)) for r, l in shapes]
        if not shapes:
            raise ValueError("PackedMsa: no MSAs")
        if not isinstance(cu_tokens, torch.Tensor) or cu_tokens.dim() != 1 or cu_tokens.dtype != torch.int32 or cu_tokens.numel() != len(shapes) + 1:
            raise ValueError("PackedMsa.cu_tokens must be a 1-D int32 tensor with one entry more than there are MSAs")
        for b, (r, l) in enumerate(shapes):
            if r <= 0 or l <= 0:
                raise ValueError(f"PackedMsa: MSA {b} holds no token")
            if r > hip.MSA_MAX_ROWS:
                raise ValueError(f"PackedMsa: MSA {b} has {r} rows; the column-attention kernel takes up to {hip.MSA_MAX_ROWS}")
            if l > hip.MSA_MAX_LEN:
                raise ValueError(f"PackedMsa: MSA {b} has rows of {l} tokens; the row-attention kernels take up to {hip.MSA_MAX_LEN}")
        total = sum(r * l for r, l in shapes)
        if ids.numel() % PAD_MULTIPLE or ids.numel() < total or ids.numel() > 0x7FFFFFFF:
            raise ValueError(f"PackedMsa: T_pad = {ids.numel()} must be a multiple of {PAD_MULTIPLE}, hold all {total} tokens and stay below 2^31")
        Rm, Lm = max(r for r, _ in shapes), max(l for _, l in shapes)
        padded_shape = (Rm, Lm) if padded_shape is None else (int(padded_shape[0]), int(padded_shape[1]))
        if padded_shape[0] < Rm or padded_shape[1] < Lm:
            raise ValueError(f"PackedMsa: padded_shape {padded_shape} is smaller than the largest block ({Rm}, {Lm})")
        self.ids, self.cu_tokens, self.shapes, self.padded_shape, self.pad_id = ids, cu_tokens, shapes, padded_shape, int(pad_id)
        self._tables = {}

    # ---------------------------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_list(cls, msas, padded_shape=None, pad_id=1, device=None):
        """from a list of [R_b, L_b] integer tensors, each a whole block (taken as it is: nothing is cut)"""
        msas = list(msas)
        if not msas:
            raise ValueError("PackedMsa.from_list: no MSAs")
        for i, m in enumerate(msas):
            if not isinstance(m, torch.Tensor) or m.dim() != 2:
                raise ValueError(f"PackedMsa.from_list: MSA {i} is not a 2-D [R, L] tensor")
            if m.dtype.is_floating_point or m.dtype.is_complex or m.dtype == torch.bool:
                raise ValueError(f"PackedMsa.from_list: MSA {i} has dtype {m.dtype}; token ids are integers")
            if m.numel() == 0:
                raise ValueError(f"PackedMsa.from_list: MSA {i} holds no token")
        shapes = [(int(m.shape[0]), int(m.shape[1])) for m in msas]
        total = sum(r * l for r, l in shapes)
        dev = msas[0].device if device is None else torch.device(device)
        ids = torch.full((_round_up(total, PAD_MULTIPLE),), int(pad_id), dtype=torch.int64, device=dev)
        ids[:total] = torch.cat([m.reshape(-1).to(device=dev, dtype=torch.int64) for m in msas])
        cu = torch.zeros(len(shapes) + 1, dtype=torch.int32)
        cu[1:] = torch.tensor([r * l for r, l in shapes], dtype=torch.int64).cumsum(0).to(torch.int32)
        return cls(ids, cu.to(dev), shapes, padded_shape, pad_id)

    @classmethod
    def from_padded(cls, tokens, pad_id=1):
        """from a padded [B, R, L] batch: R_b / L_b = 1 + the last row / column of MSA b that holds any non-pad token; padded_shape = (R, L)"""
        if not isinstance(tokens, torch.Tensor) or tokens.dim() != 3:
            raise ValueError("PackedMsa.from_padded needs a 3-D [B, R, L] id tensor")
        if tokens.dtype.is_floating_point or tokens.dtype.is_complex or tokens.dtype == torch.bool:
            raise ValueError(f"PackedMsa.from_padded: tokens have dtype {tokens.dtype}; token ids are integers")
        B, R, L = tokens.shape
        valid = (tokens != pad_id).cpu()
        rows, cols = valid.any(2), valid.any(1)
        msas = []
        for b in range(B):
            if not bool(rows[b].any()):
                raise ValueError(f"PackedMsa.from_padded: MSA {b} holds no token")
            rb, lb = int(rows[b].nonzero().max()) + 1, int(cols[b].nonzero().max()) + 1
            msas.append(tokens[b, :rb, :lb])
        return cls.from_list(msas, padded_shape=(R, L), pad_id=pad_id)

    # ---------------------------------------------------------------------------------------------------------- container protocol
    def __len__(self):
        return len(self.shapes)

    @property
    def T_pad(self):
        return self.ids.numel()

    @property
    def n_tokens(self):
        return sum(r * l for r, l in self.shapes)

    @property
    def device(self):
        return self.ids.device

    @property
    def is_cuda(self):
        return self.ids.is_cuda

    def to(self, device, non_blocking=False):
        out = PackedMsa.__new__(PackedMsa)
        out.__dict__.update(self.__dict__)
        out.ids = self.ids.to(device, non_blocking=non_blocking)
        out.cu_tokens = self.cu_tokens.to(device, non_blocking=non_blocking)
        out._tables = {}
        return out

    def cuda(self, device=None):
        return self.to(torch.device("cuda") if device is None else device)

    def offsets(self):
        """host ints: where each block starts in the stream, and the end of the last"""
        c = [0]
        for r, l in self.shapes:
            c.append(c[-1] + r * l)
        return c

    def unpack(self, x=None):
        """per-MSA [R_b, L_b, ...] views of a stream x [T_pad, ...] (default: the ids)"""
        x = self.ids if x is None else x
        if x.shape[0] != self.T_pad:
            raise ValueError(f"PackedMsa.unpack: the stream has {x.shape[0]} rows, this batch {self.T_pad}")
        c = self.offsets()
        return [x[c[b]:c[b + 1]].view(r, l, *x.shape[1:]) for b, (r, l) in enumerate(self.shapes)]

    def to_padded(self):
        """the [N, R, L] batch of `padded_shape`, pad id everywhere outside the blocks"""
        R, L = self.padded_shape
        out = torch.full((len(self), R, L), self.pad_id, dtype=torch.int64, device=self.ids.device)
        for b, m in enumerate(self.unpack()):
            out[b, :m.shape[0], :m.shape[1]] = m
        return out

    def row_lens(self):
        """int32 [N] = L_b on the ids' device (the embedding kernel's second table); built once per batch and device"""
        key = ("row_lens", str(self.ids.device))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = torch.tensor([l for _, l in self.shapes], dtype=torch.int32).to(self.ids.device)
        return t

    def row0(self):
        """(index int64 [T0_pad] on the device, cu int32 [N + 1], L_b list): the stream rows of every MSA's row 0, concatenated in MSA order and filled up
        to a multiple of 256 with the stream's last row -- a tail row, or, where the stream has no tail, a row the segment table leaves out anyway"""
        key = ("row0", str(self.ids.device))
        t = self._tables.get(key)
        if t is None:
            c = self.offsets()
            idx = torch.cat([torch.arange(c[b], c[b] + l, dtype=torch.int64) for b, (_, l) in enumerate(self.shapes)])
            full = torch.full((_round_up(idx.numel(), PAD_MULTIPLE),), self.T_pad - 1, dtype=torch.int64)
            full[:idx.numel()] = idx
            cu = torch.zeros(len(self) + 1, dtype=torch.int32)
            cu[1:] = torch.tensor([l for _, l in self.shapes], dtype=torch.int32).cumsum(0)
            t = self._tables[key] = (full.to(self.ids.device), cu.to(self.ids.device), idx.numel())
        return t

    def tables(self, H, groups=None):
        """The device-side geometry of the ragged attention calls (include/oneprot_hip.h), built once per (H, grouping, device) and kept on the object, as
        PackedTokens.attn_work is.  groups: [(b0, b1), ...] consecutive groups of whole MSAs (default: one group, the whole batch).  One dict per group:
        geo int64 [n, 8] on the device, the group's MSAs longest first, rows {tok0, R_b, L_b, s0, p0, vt0, b - b0, 0}; n, b_first = b0, max_R, max_L,
        sum_l_lp, sum_r_lp (the workspace query's arguments) and s_elems (fp32 elements of the group's score maps)."""
        groups = [(0, len(self))] if groups is None else [(int(a), int(b)) for a, b in groups]
        key = ("geo", int(H), tuple(groups), str(self.ids.device))
        out = self._tables.get(key)
        if out is None:
            c, out = self.offsets(), []
            for b0, b1 in groups:
                order = sorted(range(b0, b1), key=lambda b: -(self.shapes[b][0] * self.shapes[b][1] * self.shapes[b][1]))
                rows, s0, sum_l_lp, sum_r_lp = [], 0, 0, 0
                for b in order:
                    r, l = self.shapes[b]
                    rows.append([c[b], r, l, s0, 0, 0, b - b0, 0])
                    s0 += H * l * l
                    sum_l_lp += l * _round_up(l, 32)
                    sum_r_lp += r * _round_up(l, 32)
                p0, vt0 = 0, H * sum_l_lp                  # the probabilities of all the group's MSAs, then their transposed V
                for row in rows:
                    lp = _round_up(row[2], 32)
                    row[4], row[5] = p0, vt0
                    p0 += H * row[2] * lp
                    vt0 += H * row[1] * 64 * lp
                out.append(dict(geo=torch.tensor(rows, dtype=torch.int64).to(self.ids.device), n=b1 - b0, b_first=b0,
                                max_R=max(self.shapes[b][0] for b in order), max_L=max(self.shapes[b][1] for b in order),
                                sum_l_lp=sum_l_lp, sum_r_lp=sum_r_lp, s_elems=s0))
            self._tables[key] = out
        return out

    def __repr__(self):
        return (f"PackedMsa(N={len(self)}, T_pad={self.T_pad}, tokens={self.n_tokens}, padded_shape={self.padded_shape}, device={self.ids.device})")


def is_packed(x):
    return isinstance(x, (PackedTokens, PackedMsa))


def batch_size(x):
    """N of a packed batch, B of a padded one"""
    return len(x) if isinstance(x, (PackedTokens, PackedMsa)) else int(x.shape[0])
