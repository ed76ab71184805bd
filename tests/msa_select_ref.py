"""An independent numpy restatement of the MSA input path, written from the rule's text and not imported from the library (oneprot_amd/msa_data.py,
csrc/msa_select.hip are what it checks).

Selection: S_j = sum over the chosen rows i of #{positions where rows i and j differ}, an integer; each step picks the unselected j with the largest
("max") / smallest ("min") S_j, the lowest j among equal S_j; the first pick is row 0; min(num_seqs, N) picks.
Tokens: <cls> 0, <pad> 1, <eos> 2, <unk> 3, "LAGVSERTIDPKQNFYMHWCXBUZO.-" 4..30, <null_1> 31, <mask> 32, any other byte 3."""
import numpy as np

ALPHABET = "LAGVSERTIDPKQNFYMHWCXBUZO.-"


def to_bytes(seqs):
    return np.array([[ord(c) for c in s] for s in seqs], dtype=np.uint8)


def distance_matrix_row(rows, i):
    return (rows != rows[i][None, :]).sum(axis=1, dtype=np.int64)


def greedy(rows, num_seqs, mode):
    """(sorted picks, picks in the order made, tie_free): tie_free is False when at some step two unselected rows shared the best score"""
    N = len(rows)
    picks = [0]
    S = np.zeros(N, dtype=np.int64)
    tie_free = True
    while len(picks) < min(num_seqs, N):
        S = S + distance_matrix_row(rows, picks[-1])
        free = np.ones(N, dtype=bool)
        free[picks] = False
        cand = np.flatnonzero(free)
        best = S[cand].max() if mode == "max" else S[cand].min()
        hits = cand[S[cand] == best]
        best_j, n_best = int(hits.min()), len(hits)
        tie_free = tie_free and n_best == 1
        picks.append(int(best_j))
    return sorted(picks), picks, tie_free


def token_of(byte):
    ch = chr(byte)
    return 4 + ALPHABET.index(ch) if ch in ALPHABET else 3


def msa_tokens(rows, picks_sorted, max_length):
    """int64 [R, Lt]: <cls> + letters, at most 1022 letters, then at most max_length tokens"""
    out = []
    for i in picks_sorted:
        toks = [0] + [token_of(b) for b in rows[i][:1022]]
        out.append(toks[:max_length])
    return np.array(out, dtype=np.int64)


def seq_tokens(row0, max_length):
    """<cls> letters <eos>; when that is longer than max_length, the letters are cut so that <eos> stays"""
    letters = [token_of(b) for b in row0]
    if len(letters) + 2 > max_length:
        letters = letters[:max_length - 2]
    return np.array([0] + letters + [2], dtype=np.int64)


def padded_batch(blocks, pad=1):
    R, L = max(b.shape[0] for b in blocks), max(b.shape[1] for b in blocks)
    out = np.full((len(blocks), R, L), pad, dtype=np.int64)
    for b, blk in enumerate(blocks):
        out[b, :blk.shape[0], :blk.shape[1]] = blk
    return out


def padded_seqs(seqs, pad=1):
    L = max(len(s) for s in seqs)
    out = np.full((len(seqs), L), pad, dtype=np.int64)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s
    return out


def draw(seed, N, L, kind="iid", letters="ACDEFGHIKLMNPQRSTVWY-", rate=0.15):
    """a drawn alignment as a list of strings: iid rows, or mutated copies of a query"""
    rng = np.random.default_rng(seed)
    abc = np.array(list(letters))
    if kind == "iid":
        arr = rng.integers(0, len(abc), (N, L))
    else:
        q = rng.integers(0, len(abc), L)
        arr = np.tile(q, (N, 1))
        hit = rng.random((N, L)) < rate * rng.random((N, 1)) * 2
        hit[0] = False
        arr = np.where(hit, rng.integers(0, len(abc), (N, L)), arr)
    return ["".join(abc[r]) for r in arr]
