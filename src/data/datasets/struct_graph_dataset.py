"""`_target_: src.data.datasets.struct_graph_dataset.StructDataset` (ref configs/data/modalities/{pocket,struct_graph}.yaml)."""
from oneprot_amd.graph_data import GraphBatch, GraphData, StructDataset  # noqa: F401
