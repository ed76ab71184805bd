"""Input path of the pocket / struct_graph modalities (ref src/data/utils/struct_graph_utils.py:31-226, src/data/datasets/struct_graph_dataset.py):
the batch type the ProNet tower reads, the per-residue featurisation, and the dataset with its three train-only augmentations.  Host code, and the host
side of the batch featurisation on the device (csrc/graph_feats.hip).

* `GraphBatch` carries the attribute names of the PyG `Batch` the reference builds (x, coords_ca / _n / _c, bb_embs, side_chain_embs, batch, ptr,
  num_nodes, num_graphs, .to(device)); `GraphBatch.from_data_list(list)` concatenates per-protein `GraphData`.  torch_geometric is not needed; where it
  is installed a real `Batch` works too, because the tower reads attributes only.
* `get_atom_pos`, `calc_side_chain_embs`, `calc_bb_embs`, `compute_diherals`, `protein_to_graph`: the reference's signatures and arithmetic (pinned by
  tests/golden/struct_graph_feats.pt).  The cross products are written with dim=-1, which is what the reference's dimension-less torch.cross means
  for every protein that does not have exactly 3 residues.
* `protein_to_graph(..., h5_file=...)` takes a path (opened with h5py where that is importable) or any nested mapping with the reference's layout.
* `read_records` is the reading half of `protein_to_graph`; `featurize_batch(records, device=None)` turns a list of such records into the GraphBatch in
  one call: on the host (protein_to_graph's arithmetic per record + from_data_list, exactly), or on the GPU (`prepare_batch`: name codes and residue
  runs, vectorised over the concatenated batch; one pinned staging buffer, one copy, oneprot_graph_featurize; nothing read back).  The four host
  functions are the kernel's specification (DESIGN.md section 7 states the rule once).  `synthetic_atom_records` makes all-atom records for tools and tests.
* `StructDataset`: the reference's constructor; `dataset.device` (set after construction, default None = the host path) featurises the batch there;
  sequence ids come from the ESM vocabulary of oneprot_amd.msa_data, not from a downloaded tokenizer.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import Dataset

from .msa_data import CLS_ID, EOS_ID, PAD_ID, _byte_map

res1int = {aa: k for k, aa in enumerate("ARNDCQEGHILKMFPSTWYV")}
res1int["X"] = 20
_NODE_KEYS = ("x", "coords_ca", "coords_n", "coords_c", "bb_embs", "side_chain_embs")


class GraphData:
    """one protein: attribute bag, as torch_geometric.data.Data is used by the reference"""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def num_nodes(self):
        return int(self.x.shape[0])


class GraphBatch:
    def __init__(self, x, coords_ca, coords_n, coords_c, bb_embs, side_chain_embs, batch, ptr, num_graphs):
        self.x, self.coords_ca, self.coords_n, self.coords_c = x, coords_ca, coords_n, coords_c
        self.bb_embs, self.side_chain_embs, self.batch, self.ptr, self.num_graphs = bb_embs, side_chain_embs, batch, ptr, int(num_graphs)

    @property
    def num_nodes(self):
        return int(self.x.shape[0])

    @classmethod
    def from_data_list(cls, data_list):
        if not data_list:
            raise ValueError("GraphBatch.from_data_list: an empty list")
        for d in data_list:
            n = d.x.shape[0]
            if n < 1 or any(getattr(d, k).shape[0] != n for k in _NODE_KEYS):
                raise ValueError("GraphBatch.from_data_list: every protein needs at least one residue and per-residue arrays of one length")
            if int(d.x.min()) < 0 or int(d.x.max()) > 25:
                raise ValueError("GraphBatch.from_data_list: residue types must lie in 0..25 (the tower's one-hot width)")
        sizes = torch.tensor([d.x.shape[0] for d in data_list], dtype=torch.int64)
        ptr = torch.zeros(len(data_list) + 1, dtype=torch.int64)
        ptr[1:] = sizes.cumsum(0)
        cat = {k: torch.cat([getattr(d, k) for d in data_list], dim=0) for k in _NODE_KEYS}
        return cls(cat["x"].to(torch.int64).reshape(-1, 1), cat["coords_ca"].float(), cat["coords_n"].float(), cat["coords_c"].float(), cat["bb_embs"].float(),
                   cat["side_chain_embs"].float(), torch.repeat_interleave(torch.arange(len(data_list)), sizes), ptr, len(data_list))

    def to(self, device):
        return GraphBatch(*(getattr(self, k).to(device) for k in _NODE_KEYS), self.batch.to(device), self.ptr.to(device), self.num_graphs)

    def clone(self):
        return GraphBatch(*(getattr(self, k).clone() for k in _NODE_KEYS), self.batch.clone(), self.ptr.clone(), self.num_graphs)


# ---- featurisation (ref struct_graph_utils.py:31-144) ---------------------------------------------------------------------------------------------------
# the atom names that stand at each place of the side-chain torsion chain N, CA, C, CB, *G, *D, *E, *Z, NH1 (ref :33-41)
_ATOM_SETS = ((b"N",), (b"CA",), (b"C",), (b"CB",), (b"CG", b"SG", b"OG", b"CG1", b"OG1"), (b"CD", b"SD", b"CD1", b"OD1", b"ND1"), (b"CE", b"NE", b"OE1"),
              (b"CZ", b"NZ"), (b"NH1",))


def get_atom_pos(amino_types, atom_names, atom_amino_id, atom_pos):
    """(pos_n, pos_ca, pos_c, pos_cb, pos_g, pos_d, pos_e, pos_z, pos_h): fp32 [n_residues, 3], NaN where a residue has no such atom; a missing N or C
    takes the residue's CA.  Residues are numbered by the rank of their atom_amino_id (np.unique), so ids need not be contiguous."""
    names = np.asarray(atom_names).astype("S")
    atom_pos = np.asarray(atom_pos)
    _, rank = np.unique(np.asarray(atom_amino_id), return_inverse=True)
    out = []
    for group in _ATOM_SETS:
        mask = np.isin(names, np.array(group, dtype="S"))
        pos = np.full((len(amino_types), 3), np.nan)
        pos[rank[mask]] = atom_pos[mask]
        out.append(torch.FloatTensor(pos))
    pos_n, pos_ca, pos_c = out[:3]
    for p in (pos_n, pos_c):
        miss = torch.isnan(p)
        p[miss] = pos_ca[miss]
    return tuple(out)


def compute_diherals(v1, v2, v3):
    n1, n2 = torch.cross(v1, v2, dim=-1), torch.cross(v2, v3, dim=-1)
    a = (n1 * n2).sum(dim=-1)
    b = torch.nan_to_num((torch.cross(n1, n2, dim=-1) * v2).sum(dim=-1) / v2.norm(dim=1))
    return torch.nan_to_num(torch.atan2(b, a))


def calc_side_chain_embs(pos_n, pos_ca, pos_c, pos_cb, pos_g, pos_d, pos_e, pos_z, pos_h):
    """[n, 8]: sines then cosines of the first four side-chain torsions"""
    chain = (pos_n, pos_ca, pos_cb, pos_g, pos_d, pos_e, pos_z)
    v = [b - a for a, b in zip(chain[:-1], chain[1:])]
    angles = torch.stack([compute_diherals(v[k], v[k + 1], v[k + 2]) for k in range(4)], dim=1)
    return torch.cat((torch.sin(angles), torch.cos(angles)), 1)


def _normalize(tensor, dim=-1):
    return torch.nan_to_num(torch.div(tensor, torch.norm(tensor, dim=dim, keepdim=True)))


def calc_bb_embs(X):
    """X [n, 3, 3] (N, CA, C of every residue) -> [n, 6]: cosines then sines of (phi, psi, omega), with phi[0], psi[-1], omega[-1] set to angle 0"""
    X = torch.reshape(X, [3 * X.shape[0], 3])
    U = _normalize(X[1:] - X[:-1], dim=-1)
    angle = compute_diherals(U[:-2], U[1:-1], U[2:])
    angle = torch.reshape(F.pad(angle, [1, 2]), [-1, 3])
    return torch.cat([torch.cos(angle), torch.sin(angle)], 1)


def _value(node):
    """a leaf of the h5 layout: an h5py dataset (`[()]`), or already the array / bytes"""
    return node[()] if hasattr(node, "shape") and hasattr(node, "id") else node


_RES_TABLE = np.full(256, 255, dtype=np.uint8)      # letter (one byte) -> residue type; 255: no key of res1int
for _aa, _k in res1int.items():
    _RES_TABLE[ord(_aa)] = _k


def _residue_types(seq):
    """uint8 [len(seq)]: res1int of every letter through the byte table; a letter outside it raises KeyError, as the dictionary does"""
    codes = _RES_TABLE[np.frombuffer(seq.encode("utf-8"), dtype=np.uint8)]
    if len(codes) != len(seq) or (codes == 255).any():
        raise KeyError(next(a for a in seq if a not in res1int))
    return codes


def _chain_arrays(chain_group, drop_x):
    seq = _value(chain_group["residues"]["seq1"])
    seq = seq.decode("utf-8") if isinstance(seq, (bytes, np.bytes_)) else str(seq)
    if drop_x:
        seq = seq.replace("X", "")
    pp = chain_group["polypeptide"]
    return _residue_types(seq), np.asarray(_value(pp["atom_amino_id"])), np.asarray(_value(pp["type"])), np.asarray(_value(pp["xyz"]))


def _open(h5_file):
    if isinstance(h5_file, (str, bytes)) or hasattr(h5_file, "__fspath__"):
        try:
            import h5py
        except ImportError:
            raise ImportError(f"protein_to_graph: {h5_file!r} is a path and h5py is not importable here; install h5py, or pass the opened file / a nested "
                              "mapping with the same layout") from None
        return h5py.File(h5_file, "r"), True
    return h5_file, False


def read_records(identifier, h5_file, dataset="non_pdb", chain="A", pockets=False):
    """ref struct_graph_utils.py:147-200, the reading half of protein_to_graph: (amino_types [n], atom_amino_id [a], atom_names [a], atom_pos [a, 3]) of
    one protein of the structure file, the record that featurize_batch takes"""
    file, opened = _open(h5_file)
    try:
        chains = file[f"{identifier}"]["structure"]["0"]
        if chain == "A" and dataset == "non_pdb":
            amino_types, atom_amino_id, atom_names, atom_pos = _chain_arrays(chains["A"], drop_x=False)
        elif chain == "all" and dataset == "pdb":
            parts = [_chain_arrays(chains[c], drop_x=True) for c in chains.keys()]
            amino_types = np.array([a for p in parts for a in p[0]])
            atom_amino_id, atom_names, atom_pos = (np.concatenate([p[k] for p in parts]) for k in (1, 2, 3))
        else:
            amino_types, atom_amino_id, atom_names, atom_pos = _chain_arrays(chains[f"{chain}"], drop_x=True)
    finally:
        if opened:
            file.close()
    return amino_types, atom_amino_id, atom_names, atom_pos


def _record_to_graph(amino_types, atom_amino_id, atom_names, atom_pos, identifier="record"):
    """the arithmetic half of protein_to_graph (ref struct_graph_utils.py:201-226)"""
    pos = get_atom_pos(amino_types, atom_names, atom_amino_id, atom_pos)
    pos_n, pos_ca, pos_c = pos[:3]
    side_chain_embs = calc_side_chain_embs(*pos)
    side_chain_embs[torch.isnan(side_chain_embs)] = 0
    bb_embs = calc_bb_embs(torch.stack((pos_n, pos_ca, pos_c), dim=1))
    bb_embs[torch.isnan(bb_embs)] = 0
    data = GraphData(side_chain_embs=side_chain_embs, bb_embs=bb_embs, x=torch.tensor(amino_types, dtype=torch.int64).unsqueeze(1), coords_ca=pos_ca,
                     coords_n=pos_n, coords_c=pos_c)
    if not all(len(getattr(data, k)) == len(data.x) for k in _NODE_KEYS):
        raise AssertionError(f"{identifier}: per-residue arrays of different lengths")
    return data


def protein_to_graph(identifier, h5_file, dataset="non_pdb", chain="A", pockets=False):
    """ref struct_graph_utils.py:147-226: one protein of the structure file as a GraphData (x [n, 1], coords_ca / _n / _c, bb_embs [n, 6], side_chain_embs [n, 8])"""
    return _record_to_graph(*read_records(identifier, h5_file, dataset, chain, pockets), identifier=identifier)


# ---- the whole batch at once (csrc/graph_feats.hip, include/oneprot_hip.h "graph input") ----------------------------------------------------------------
def name_codes(atom_names):
    """uint32 [a]: the first four bytes of every name, zero padded, as one little-endian word -- what the kernel compares.  The 20 names of _ATOM_SETS
    have at most 3 bytes, so a longer name, cut, can equal none of them."""
    names = np.asarray(atom_names).reshape(-1)
    return np.ascontiguousarray(names.astype("S4")).view("<u4").astype(np.uint32, copy=False)


def _distinct_ids_error(g, distinct, n):
    return IndexError(f"featurize_batch: protein {g} of the batch has {distinct} distinct atom_amino_id and {n} residues")


def prepare_batch(records):
    """The kernel's input from a list of records (read_records), vectorised over the concatenated batch: dict of atom_pos fp32 [A, 3], atom_name4 uint32 [A],
    res_atom_ptr int64 [N + 1], res_type uint8 [N], graph_ptr int64 [G + 1].  Residue k of a protein owns the atoms of its k-th smallest atom_amino_id
    (np.unique's rank in get_atom_pos), as one run: where ids are not sorted inside a protein, the atoms are put in the stable order of their ids first,
    which keeps "the last atom of a set wins".  More distinct ids than residues: IndexError.  Fewer: the trailing residues own no atom."""
    if not records:
        raise ValueError("featurize_batch: an empty list")
    G = len(records)
    types = [np.asarray(r[0]).reshape(-1) for r in records]
    ids = [np.asarray(r[1]).reshape(-1) for r in records]
    n_res = np.array([len(t) for t in types], dtype=np.int64)
    n_atoms = np.array([len(i) for i in ids], dtype=np.int64)
    if (n_res < 1).any():
        raise ValueError("GraphBatch.from_data_list: every protein needs at least one residue and per-residue arrays of one length")
    types, ids = np.concatenate(types), np.concatenate(ids)
    if int(types.min()) < 0 or int(types.max()) > 25:
        raise ValueError("GraphBatch.from_data_list: residue types must lie in 0..25 (the tower's one-hot width)")
    names = [np.asarray(r[2]).reshape(-1) for r in records]
    codes = name_codes(np.concatenate(names)) if len({a.dtype.kind for a in names}) == 1 else np.concatenate([name_codes(a) for a in names])
    pos = np.concatenate([np.asarray(r[3]).reshape(-1, 3) for r in records]).astype(np.float32)
    A, N = len(ids), int(n_res.sum())
    if len(codes) != A or len(pos) != A:
        raise ValueError("featurize_batch: atom_amino_id, atom_names and atom_pos of a record differ in length")
    graph_ptr = np.zeros(G + 1, dtype=np.int64)
    graph_ptr[1:] = np.cumsum(n_res)
    prot = np.repeat(np.arange(G), n_atoms)
    new_run = np.ones(A, dtype=bool)
    if A > 1:
        same = prot[1:] == prot[:-1]
        if (same & (ids[1:] < ids[:-1])).any():
            order = np.lexsort((ids, prot))                                  # stable: equal ids keep their order
            ids, codes, pos = ids[order], codes[order], pos[order]
        new_run[1:] = ~same | (ids[1:] != ids[:-1])
    run_start = np.flatnonzero(new_run)
    run_prot = prot[run_start]
    runs = np.bincount(run_prot, minlength=G)
    over = np.flatnonzero(runs > n_res)
    if len(over):
        raise _distinct_ids_error(int(over[0]), int(runs[over[0]]), int(n_res[over[0]]))
    first_run = np.cumsum(runs) - runs
    counts = np.zeros(N, dtype=np.int64)
    counts[graph_ptr[run_prot] + np.arange(len(run_start)) - first_run[run_prot]] = np.diff(np.append(run_start, A))
    res_atom_ptr = np.zeros(N + 1, dtype=np.int64)
    res_atom_ptr[1:] = np.cumsum(counts)
    return {"atom_pos": pos, "atom_name4": codes, "res_atom_ptr": res_atom_ptr, "res_type": types.astype(np.uint8), "graph_ptr": graph_ptr}


def _device_path_available():
    from . import hip
    return torch.cuda.is_available() and os.path.exists(hip.LIB_PATH)


_last_host = None          # the pinned source of the last asynchronous copy stays alive until the next call


def _featurize_device(prep, device):
    """one pinned staging buffer, one asynchronous copy and oneprot_graph_featurize on the current stream of `device`; nothing is read back"""
    global _last_host
    from . import hip
    hip.lib()
    N, G, A = len(prep["res_type"]), len(prep["graph_ptr"]) - 1, len(prep["atom_name4"])
    parts = (("res_atom_ptr", np.int64, N + 1), ("graph_ptr", np.int64, G + 1), ("atom_pos", np.float32, 3 * max(A, 1)), ("atom_name4", np.uint32, max(A, 1)),
             ("res_type", np.uint8, N))                                       # by falling alignment: every part starts on a multiple of its item size
    at, total = {}, 0
    for key, dt, n in parts:
        at[key] = (total, total + n * np.dtype(dt).itemsize)
        total = at[key][1]
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    flat = host.numpy()
    for key, dt, n in parts:
        src = prep[key].reshape(-1)
        flat[at[key][0]:at[key][0] + src.nbytes] = src.view(np.uint8)
    with torch.cuda.device(device):
        dev = host.to(device, non_blocking=True)
        view = {key: dev[a:b] for key, (a, b) in at.items()}
        f32 = dict(dtype=torch.float32, device=device)
        i64 = dict(dtype=torch.int64, device=device)
        out = GraphBatch(torch.empty(N, 1, **i64), torch.empty(N, 3, **f32), torch.empty(N, 3, **f32), torch.empty(N, 3, **f32), torch.empty(N, 6, **f32),
                         torch.empty(N, 8, **f32), torch.empty(N, **i64), torch.empty(G + 1, **i64), G)
        hip.call("oneprot_graph_featurize", view["atom_pos"].view(torch.float32), view["atom_name4"].view(torch.int32), view["res_atom_ptr"].view(torch.int64),
                 view["res_type"], view["graph_ptr"].view(torch.int64), out.x, out.coords_ca, out.coords_n, out.coords_c, out.bb_embs, out.side_chain_embs,
                 out.batch, out.ptr, host.data_ptr() + at["res_atom_ptr"][0], host.data_ptr() + at["graph_ptr"][0], A, N, G)
    _last_host = host
    return out


def featurize_batch(records, device=None):
    """GraphBatch of a list of records (read_records; synthetic_atom_records).  device "cpu", or None without a GPU or without the built library: the host
    path, protein_to_graph's arithmetic per record and GraphBatch.from_data_list.  Otherwise the device path: prepare_batch, one pinned staging buffer,
    one asynchronous copy and two launches on the current stream (None: the current GPU).  A device that is asked for and cannot run raises."""
    if not records:
        raise ValueError("featurize_batch: an empty list")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if _device_path_available() else torch.device("cpu")
    device = torch.device(device)
    if device.type == "cpu":
        for g, r in enumerate(records):
            distinct = len(np.unique(np.asarray(r[1])))
            if distinct > len(r[0]):
                raise _distinct_ids_error(g, distinct, len(r[0]))
        return GraphBatch.from_data_list([_record_to_graph(*r, identifier=f"record {g}") for g, r in enumerate(records)])
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _featurize_device(prepare_batch(records), device)


# ---- dataset (ref struct_graph_dataset.py) ----------------------------------------------------------------------------------------------------------------
def tokenize_sequences(sequences, max_length):
    """int64 [B, L]: <cls> letters <eos>, right-padded, truncated to max_length tokens as the HF tokenizer does with truncation=True"""
    table = _byte_map()
    rows = []
    for s in sequences:
        body = table[np.frombuffer(s.encode("ascii", "replace"), dtype=np.uint8)][:max(max_length - 2, 0)]
        rows.append(np.concatenate([[CLS_ID], body, [EOS_ID]]).astype(np.int64))
    L = max(len(r) for r in rows)
    out = torch.full((len(rows), L), PAD_ID, dtype=torch.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.from_numpy(r)
    return out


def augment_struct_batch(batch, use_mask, use_coord_noise, use_deform, rng=None, generator=None):
    """the reference's three train-only augmentations, in place (struct_graph_dataset.py:59-77): a uniform-random fraction of x set to 20; N(0, 0.1)
    noise clipped to +-0.3 on each of CA / N / C; one [1, 3] scale N(1, 0.1) clipped to [0.9, 1.1] per atom type.  rng: numpy Generator of the mask;
    generator: torch Generator of the normals (both default to the global ones, as in the reference).  Every draw is made on the host, whatever
    device holds the batch: only the index assignment, the add and the multiply run where the tensors are, so the same seeds give the same batch."""
    if use_mask:
        u = np.random.uniform(0, 1) if rng is None else rng.uniform(0, 1)
        n = batch.num_nodes
        pick = (np.random.choice if rng is None else rng.choice)(n, int(n * u), replace=False)
        batch.x[torch.as_tensor(pick, dtype=torch.int64).to(batch.x.device), 0] = 20
    if use_coord_noise:
        for k in ("coords_ca", "coords_n", "coords_c"):
            c = getattr(batch, k)
            c += torch.clip(torch.normal(0.0, 0.1, size=c.shape, generator=generator), min=-0.3, max=0.3).to(c.device)
    if use_deform:
        for k in ("coords_ca", "coords_n", "coords_c"):
            c = getattr(batch, k)
            c *= torch.clip(torch.normal(1.0, 0.1, size=(1, 3), generator=generator), min=0.9, max=1.1).to(c.device)
    return batch


class StructDataset(Dataset):
    """ref struct_graph_dataset.py:12-81, same constructor.  `seq_tokenizer` is accepted and not opened.  `h5_file` / `h5_file_seq` may be replaced after
    construction by an opened file or a nested mapping (protein_to_graph).  `device`, set after construction like the other datasets' (the data
    module's `attributes:`): None featurises on the host per protein, as ever; a device makes collate_fn read the records and featurise the whole batch
    there in one call (featurize_batch), and return the GraphBatch and the sequence ids on that device."""

    def __init__(self, data_dir: str, split: str, max_length: int = 1024, seq_tokenizer: str = "facebook/esm2_t33_650M_UR50D", use_struct_mask: bool = False,
                 use_struct_coord_noise: bool = False, use_struct_deform: bool = False, pocket: bool = False):
        self.id_list = []
        self.pocket, self.split, self.max_length = pocket, split, max_length
        self.h5_file = f'{data_dir}/{"pockets_100_residues" if pocket else "seqstruc"}.h5'
        self.h5_file_seq = f"{data_dir}/seqstruc.h5"
        self.use_struct_mask, self.use_struct_coord_noise, self.use_struct_deform = use_struct_mask, use_struct_coord_noise, use_struct_deform
        csv_file = f'{data_dir}/{split}_{"pocket" if pocket else "seqstruc"}.csv'
        try:
            with open(csv_file, "r") as file:
                self.id_list = [line.split(",")[0].strip() for line in file]
        except FileNotFoundError:
            print(f"File not found: {csv_file}")
        self.seq_tokenizer = seq_tokenizer
        self.device = None       # set after construction (the data module's `attributes:`): the batch is featurised there in one call (featurize_batch)

    def __len__(self) -> int:
        return len(self.id_list) if self.split == "train" else 1000

    def __getitem__(self, idx: int) -> str:
        return self.id_list[idx]

    def collate_fn(self, seq_ids, return_raw_sequences: bool = False):
        """(sequence_ids int64 [B, L], GraphBatch, "pocket" | "struct_graph", sequences)"""
        sequences, structures = [], []
        seq_file, opened = _open(self.h5_file_seq)
        try:
            for seq_id in seq_ids:
                try:
                    seq = _value(seq_file[seq_id]["structure"]["0"]["A"]["residues"]["seq1"])
                    structure = (protein_to_graph if self.device is None else read_records)(seq_id, self.h5_file, "non_pdb", "A", pockets=self.pocket)
                except KeyError:
                    print(f"KeyError: {seq_id} not found in {self.h5_file}")
                    continue
                sequences.append(seq.decode("utf-8") if isinstance(seq, (bytes, np.bytes_)) else str(seq))
                structures.append(structure)
        finally:
            if opened:
                seq_file.close()
        if return_raw_sequences:
            return sequences
        batch_struct = GraphBatch.from_data_list(structures) if self.device is None else featurize_batch(structures, self.device)
        if self.split == "train":
            augment_struct_batch(batch_struct, self.use_struct_mask, self.use_struct_coord_noise, self.use_struct_deform)
        seq_tokens = tokenize_sequences(sequences, self.max_length)
        return seq_tokens if self.device is None else seq_tokens.to(self.device), batch_struct, "pocket" if self.pocket else "struct_graph", sequences


# ---- synthetic proteins (oneprot_amd.data.SyntheticPairs, tools/pronet_ab.py, the tests) -------------------------------------------------------------------
def synthetic_protein(n, gen):
    """GraphData of n residues: a random-walk backbone with 3.8 A CA steps, N and C at 1.46 A and 1.52 A from CA in random directions, residue types
    0..19, backbone features through calc_bb_embs, no side chains (all-zero side_chain_embs, as for a CA/N/C-only structure)"""
    def unit(k):
        v = torch.randn(k, 3, generator=gen)
        return v / v.norm(dim=-1, keepdim=True)
    ca = torch.cumsum(3.8 * unit(n), dim=0)
    cn, cc = ca + 1.46 * unit(n), ca + 1.52 * unit(n)
    bb = calc_bb_embs(torch.stack((cn, ca, cc), dim=1))
    bb[torch.isnan(bb)] = 0
    return GraphData(x=torch.randint(0, 20, (n, 1), generator=gen), coords_ca=ca, coords_n=cn, coords_c=cc, bb_embs=bb, side_chain_embs=torch.zeros(n, 8))


# the heavy atoms behind N, CA, C, O of each residue type, in the order structure files list them (one row per key of res1int, "X" as glycine)
_SIDE_CHAIN_ATOMS = ("CB", "CB CG CD NE CZ NH1 NH2", "CB CG OD1 ND2", "CB CG OD1 OD2", "CB SG", "CB CG CD OE1 NE2", "CB CG CD OE1 OE2", "", "CB CG ND1 CD2 CE1 NE2",
                     "CB CG1 CG2 CD1", "CB CG CD1 CD2", "CB CG CD CE NZ", "CB CG SD CE", "CB CG CD1 CD2 CE1 CE2 CZ", "CB CG CD", "CB OG", "CB OG1 CG2",
                     "CB CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2", "CB CG CD1 CD2 CE1 CE2 CZ OH", "CB CG1 CG2", "")
_PLACE_OF_NAME = {name.decode(): k for k, group in enumerate(_ATOM_SETS) for name in group}
MIN_TORSION_CONDITIONING = 0.05


def torsion_conditioning(p0, p1, p2, p3):
    """|n1| |n2| / (|v1| |v2|^2 |v3|) of the torsions over the points p0 .. p3 (float64 [m, 3]): the product of the sines of the two bond angles, the
    factor by which a rounding error of the operands grows in atan2(b, a).  NaN where a vector is zero or an atom is missing."""
    v1, v2, v3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(v1, v2), np.cross(v2, v3)
    norm = lambda v: np.sqrt((v * v).sum(-1))      # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        return norm(n1) * norm(n2) / (norm(v1) * norm(v2) ** 2 * norm(v3))


def record_torsions(place_pos):
    """the quadruples of points behind every angle of a protein, from its nine place positions [9, n, 3] (N and C already CA where missing):
    (p0, p1, p2, p3, last, third); `last` = (places, residues) of each torsion's fourth atom, `third` of an atom that sets its first bond angle (the
    third atom; N for phi, whose third atom is the CA).  Side chains first (N CA CB G D E Z), then phi, psi, omega."""
    n = place_pos.shape[1]
    chain = (0, 1, 3, 4, 5, 6, 7)
    quads, last, third = [], [], []
    r = np.arange(n)
    for k in range(4):
        quads.append(tuple(place_pos[chain[k + j]] for j in range(4)))
        last.append((np.full(n, chain[k + 3]), r))
        third.append((np.full(n, chain[k + 2]), r))
    N, CA, C = place_pos[0], place_pos[1], place_pos[2]
    if n > 1:
        quads += [(C[:-1], N[1:], CA[1:], C[1:]), (N[:-1], CA[:-1], C[:-1], N[1:]), (CA[:-1], C[:-1], N[1:], CA[1:])]
        last += [(np.full(n - 1, 2), r[1:]), (np.full(n - 1, 0), r[1:]), (np.full(n - 1, 1), r[1:])]
        third += [(np.full(n - 1, 0), r[1:]), (np.full(n - 1, 2), r[:-1]), (np.full(n - 1, 0), r[1:])]
    cat = lambda pairs: (np.concatenate([a[0] for a in pairs]), np.concatenate([a[1] for a in pairs]))      # noqa: E731
    return tuple(np.concatenate([q[j] for q in quads]) for j in range(4)) + (cat(last), cat(third))


def synthetic_atom_records(n, gen, ca_only=0.04, bare=0.04):
    """An all-atom record (amino_types uint8 [n], atom_amino_id int64 [a], atom_names S4 [a], atom_pos fp32 [a, 3]) of n residues, what read_records
    returns: a random-walk CA trace with 3.8 A steps, N / C / CB at bond length from CA and G, D, E, Z, NH1 each from its predecessor in random
    directions, every residue type's real atom names, ids with gaps, a fraction `ca_only` of CA-only residues and `bare` of residues of N, CA, C, O alone.
    A torsion whose conditioning |n1| |n2| / (|v1| |v2|^2 |v3|) is below MIN_TORSION_CONDITIONING (about 0.7 % of random ones) has its last atom drawn
    again (and the third one where the first bond angle alone is too flat), so that every angle of the record is a well-posed function of fp32 coordinates."""
    def unit(*shape):
        v = torch.randn(*shape, 3, generator=gen, dtype=torch.float64).numpy()
        return v / np.sqrt((v * v).sum(-1, keepdims=True))
    types = torch.randint(0, 20, (n,), generator=gen).numpy().astype(np.uint8)
    kind = torch.rand(n, generator=gen).numpy()
    ca_only, bare = kind < ca_only, (kind >= ca_only) & (kind < ca_only + bare)
    ids = np.cumsum(1 + (torch.rand(n, generator=gen).numpy() < 0.05).astype(np.int64)) + 2
    atoms = [["CA"] if ca_only[r] else ["N", "CA", "C", "O"] + ([] if bare[r] else _SIDE_CHAIN_ATOMS[types[r]].split()) for r in range(n)]
    has = np.zeros((9, n), dtype=bool)
    for r, names in enumerate(atoms):
        for a in names:
            if a in _PLACE_OF_NAME:
                has[_PLACE_OF_NAME[a], r] = True
    step, dirs = unit(n), unit(9, n)                       # the CA step into residue r; the bond direction of each place's atom
    bond = np.array([1.46, 0.0, 1.52, 1.53, 1.5, 1.5, 1.5, 1.5, 1.33])[:, None, None]
    parent = (1, 1, 1, 1, 3, 4, 5, 6, 7)

    def places():
        pos = np.empty((9, n, 3))
        pos[1] = np.cumsum(3.8 * step, axis=0)
        for k in (0, 2, 3, 4, 5, 6, 7, 8):
            pos[k] = pos[parent[k]] + bond[k] * dirs[k]
        pos = pos.astype(np.float32).astype(np.float64)
        pos[~has] = np.nan
        for k in (0, 2):
            pos[k] = np.where(np.isnan(pos[k]), pos[1], pos[k])
        return pos
    for _ in range(64):
        pos = places()
        p0, p1, p2, p3, last, third = record_torsions(pos)
        bad = torsion_conditioning(p0, p1, p2, p3) < MIN_TORSION_CONDITIONING       # NaN (no torsion there) compares False
        if not bad.any():
            break
        # the first bond angle does not depend on the fourth atom: where it alone is too flat for any fourth atom to do, its own atom is drawn again too
        flat = bad & (torsion_conditioning(p0, p1, p2, p2 + np.cross(p1 - p0, p2 - p1)) < 4 * MIN_TORSION_CONDITIONING)
        again = set(zip(last[0][bad].tolist(), last[1][bad].tolist())) | set(zip(third[0][flat].tolist(), third[1][flat].tolist()))
        for k, r in sorted(again):
            if k == 1 or not has[k, r]:                    # the atom is the CA itself (or stands in for a missing N / C): a new step
                step[r] = unit()
            else:
                dirs[k, r] = unit()
    else:
        raise RuntimeError("synthetic_atom_records: ill-conditioned torsions left after 64 rounds of redraws")
    names, xyz, atom_ids = [], [], []
    for r, res_atoms in enumerate(atoms):
        for a in res_atoms:
            k = _PLACE_OF_NAME.get(a)
            xyz.append(pos[k, r] if k is not None else pos[1, r] + 2.4 * unit())
            names.append(a)
            atom_ids.append(ids[r])
    return types, np.array(atom_ids, dtype=np.int64), np.array(names, dtype="S4"), np.array(xyz, dtype=np.float32).reshape(-1, 3)
