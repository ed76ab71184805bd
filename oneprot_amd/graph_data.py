"""Input path of the pocket / struct_graph modalities (ref src/data/utils/struct_graph_utils.py:31-226, src/data/datasets/struct_graph_dataset.py):
the batch type the ProNet tower reads, the per-residue featurisation, and the dataset with its three train-only augmentations.  Host code.

* `GraphBatch` carries the attribute names of the PyG `Batch` the reference builds (x, coords_ca / _n / _c, bb_embs, side_chain_embs, batch, ptr,
  num_nodes, num_graphs, .to(device)); `GraphBatch.from_data_list(list)` concatenates per-protein `GraphData`.  torch_geometric is not needed; where it
  is installed a real `Batch` works too, because the tower reads attributes only.
* `get_atom_pos`, `calc_side_chain_embs`, `calc_bb_embs`, `compute_diherals`, `protein_to_graph`: the reference's signatures and arithmetic (pinned by
  tests/golden/struct_graph_feats.pt).  The cross products are written with dim=-1, which is what the reference's dimension-less torch.cross means
  for every protein that does not have exactly 3 residues.
* `protein_to_graph(..., h5_file=...)` takes a path (opened with h5py where that is importable) or any nested mapping with the reference's layout.
* `StructDataset`: the reference's constructor; sequence ids come from the ESM vocabulary of oneprot_amd.msa_data, not from a downloaded tokenizer.
"""
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


def _chain_arrays(chain_group, drop_x):
    seq = _value(chain_group["residues"]["seq1"])
    seq = seq.decode("utf-8") if isinstance(seq, (bytes, np.bytes_)) else str(seq)
    if drop_x:
        seq = seq.replace("X", "")
    pp = chain_group["polypeptide"]
    return [res1int[a] for a in seq], np.asarray(_value(pp["atom_amino_id"])), np.asarray(_value(pp["type"])), np.asarray(_value(pp["xyz"]))


def _open(h5_file):
    if isinstance(h5_file, (str, bytes)) or hasattr(h5_file, "__fspath__"):
        try:
            import h5py
        except ImportError:
            raise ImportError(f"protein_to_graph: {h5_file!r} is a path and h5py is not importable here; install h5py, or pass the opened file / a nested "
                              "mapping with the same layout") from None
        return h5py.File(h5_file, "r"), True
    return h5_file, False


def protein_to_graph(identifier, h5_file, dataset="non_pdb", chain="A", pockets=False):
    """ref struct_graph_utils.py:147-226: one protein of the structure file as a GraphData (x [n, 1], coords_ca / _n / _c, bb_embs [n, 6], side_chain_embs [n, 8])"""
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
    generator: torch Generator of the normals (both default to the global ones, as in the reference)."""
    if use_mask:
        u = np.random.uniform(0, 1) if rng is None else rng.uniform(0, 1)
        n = batch.num_nodes
        pick = (np.random.choice if rng is None else rng.choice)(n, int(n * u), replace=False)
        batch.x[torch.as_tensor(pick, dtype=torch.int64), 0] = 20
    if use_coord_noise:
        for k in ("coords_ca", "coords_n", "coords_c"):
            c = getattr(batch, k)
            c += torch.clip(torch.normal(0.0, 0.1, size=c.shape, generator=generator), min=-0.3, max=0.3)
    if use_deform:
        for k in ("coords_ca", "coords_n", "coords_c"):
            c = getattr(batch, k)
            c *= torch.clip(torch.normal(1.0, 0.1, size=(1, 3), generator=generator), min=0.9, max=1.1)
    return batch


class StructDataset(Dataset):
    """ref struct_graph_dataset.py:12-81, same constructor.  `seq_tokenizer` is accepted and not opened.  `h5_file` / `h5_file_seq` may be replaced after
    construction by an opened file or a nested mapping (protein_to_graph)."""

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
                    structure = protein_to_graph(seq_id, self.h5_file, "non_pdb", "A", pockets=self.pocket)
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
        batch_struct = GraphBatch.from_data_list(structures)
        if self.split == "train":
            augment_struct_batch(batch_struct, self.use_struct_mask, self.use_struct_coord_noise, self.use_struct_deform)
        return tokenize_sequences(sequences, self.max_length), batch_struct, "pocket" if self.pocket else "struct_graph", sequences


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
