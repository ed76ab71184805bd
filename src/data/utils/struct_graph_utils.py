"""`src.data.utils.struct_graph_utils` (ref): the per-residue featurisation of the pocket / struct_graph modalities."""
from oneprot_amd.graph_data import calc_bb_embs, calc_side_chain_embs, compute_diherals, get_atom_pos, protein_to_graph, res1int  # noqa: F401
