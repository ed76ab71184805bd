"""ref src/data/utils/msa_utils.py: the a3m reader and the greedy depth selection (oneprot_amd.msa_data: no Biopython, no scipy; the selection on the GPU)."""
from oneprot_amd.msa_data import filter_and_create_msa_file_list, greedy_select, read_msa, remove_insertions, select_batch  # noqa: F401
