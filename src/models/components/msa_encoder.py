"""`_target_: src.models.components.msa_encoder.MsaEncoder` (ref configs/model/components/msa.yaml:2)."""
from oneprot_amd.encoders import MsaEncoder  # noqa: F401
