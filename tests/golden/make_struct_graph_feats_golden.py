"""Generator of tests/golden/struct_graph_feats.pt: the reference's per-residue featurisation (src/data/utils/struct_graph_utils.py:31-144 there --
get_atom_pos, calc_side_chain_embs, calc_bb_embs) on a handful of synthetic proteins, inputs and outputs recorded.

TEST INFRASTRUCTURE, run by hand where a checkout of the reference is at hand:

    cd <a scratch directory> && python <repo>/tests/golden/make_struct_graph_feats_golden.py <reference checkout> [output file]

(from a scratch directory because the reference module opens a log file in the working directory when it is imported).  h5py and torch_geometric are
not needed by the three functions and are stubbed at import when they are missing; no reference source is copied.

The proteins (5 to 40 residues, none with exactly 2 or 3: the reference's dimension-less torch.cross is ambiguous on a [3, 3] operand) cover: CA-only
residues, residues without side-chain atoms, a residue with every atom of the chain N .. NH1, atom_amino_id that is not contiguous, and every
alternative name of the G / D / E / Z places."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

SIZES = (5, 8, 17, 40, 12)
# per residue kind: the atoms present, in file order
FULL = ["N", "CA", "C", "O", "CB", "CG", "CD", "NE", "CZ", "NH1", "NH2"]          # arginine-like: the whole chain N .. NH1
KINDS = {
    "full": FULL,
    "ca_only": ["CA"],
    "backbone": ["N", "CA", "C", "O"],
    "short": ["N", "CA", "C", "O", "CB", "OG"],                                   # serine-like
    "branched": ["N", "CA", "C", "O", "CB", "CG1", "CG2", "CD1"],                 # isoleucine-like
    "thio": ["N", "CA", "C", "O", "CB", "CG", "SD", "CE"],                        # methionine-like
    "lys": ["N", "CA", "C", "O", "CB", "CG", "CD", "CE", "NZ"],
    "his": ["N", "CA", "C", "O", "CB", "CG", "ND1", "CD2"],
    "glu": ["N", "CA", "C", "O", "CB", "CG", "CD", "OE1", "OE2"],
    "no_n": ["CA", "C", "O", "CB"],                                               # a missing N takes the CA position
}


def import_reference(ref):
    for name in ("h5py", "torch_geometric", "torch_geometric.data", "transformers"):
        try:
            importlib.import_module(name)
        except Exception:
            stub = types.ModuleType(name)
            for attr in ("Data", "InMemoryDataset", "Batch", "AutoTokenizer", "EsmModel", "EsmConfig", "File"):
                setattr(stub, attr, type(attr, (), {}))
            sys.modules[name] = stub
    spec = importlib.util.spec_from_file_location("_ref_struct_graph_utils", os.path.join(ref, "src", "data", "utils", "struct_graph_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_protein(n, rs, p_index):
    kinds = list(KINDS)
    chosen = [kinds[(k + p_index) % len(kinds)] for k in rs.permutation(n)]
    chosen[rs.randint(n)] = "full"
    chosen[rs.randint(n)] = "ca_only"
    ids = np.cumsum(rs.randint(1, 4, size=n)) + rs.randint(0, 50)                 # increasing, with gaps
    if p_index == 0:
        ids = np.arange(1, n + 1)                                                 # one protein numbered 1 .. n
    ca = np.cumsum(3.8 * rs.normal(size=(n, 3)) / np.sqrt(3.0), axis=0)
    names, amino_id, xyz = [], [], []
    for r in range(n):
        pos = ca[r]
        for atom in KINDS[chosen[r]]:
            names.append(atom)
            amino_id.append(ids[r])
            xyz.append(pos if atom == "CA" else ca[r] + rs.normal(size=3) * 1.5)
    return dict(amino_types=rs.randint(0, 21, size=n).tolist(), kinds=chosen, atom_names=names, atom_amino_id=np.array(amino_id, dtype=np.int64),
                atom_pos=np.array(xyz, dtype=np.float32))


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = import_reference(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "struct_graph_feats.pt")
    rs = np.random.RandomState(20240)
    proteins = []
    for k, n in enumerate(SIZES):
        p = make_protein(n, rs, k)
        names = np.array(p["atom_names"], dtype="S")
        pos = ref.get_atom_pos(p["amino_types"], names, p["atom_amino_id"], p["atom_pos"])
        side = ref.calc_side_chain_embs(*pos)
        bb = ref.calc_bb_embs(torch.cat((torch.unsqueeze(pos[0], 1), torch.unsqueeze(pos[1], 1), torch.unsqueeze(pos[2], 1)), 1))
        proteins.append(dict(amino_types=p["amino_types"], kinds=p["kinds"], atom_names=p["atom_names"], atom_amino_id=torch.from_numpy(p["atom_amino_id"]),
                             atom_pos=torch.from_numpy(p["atom_pos"]), pos=[t.clone() for t in pos], side_chain_embs=side.clone(), bb_embs=bb.clone()))
    torch.save({"proteins": proteins, "functions": ["get_atom_pos", "calc_side_chain_embs", "calc_bb_embs"]}, out_path)
    print(f"wrote {out_path}: {len(proteins)} proteins of {SIZES} residues, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
