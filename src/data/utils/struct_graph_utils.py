"""`src.data.utils.struct_graph_utils` (ref): the per-residue featurisation of the pocket / struct_graph modalities, per protein (protein_to_graph) and
for a whole batch of records in one call (read_records + featurize_batch)."""
from oneprot_amd.graph_data import (calc_bb_embs, calc_side_chain_embs, compute_diherals, featurize_batch, get_atom_pos, prepare_batch,  # noqa: F401
                                    protein_to_graph, read_records, res1int, synthetic_atom_records)
