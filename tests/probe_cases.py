"""What the CPU and GPU probe tests share: the golden written from the reference's own MLP, and the project's MLP built from one of its configurations."""
import os

from oneprot_amd import probe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "probe_mlp.pt")


def make(cfg, g, dropout_rate=0.0):
    return probe.MLP(g["input_dim"], g["output_dim"], cfg["hidden_dims"], dropout_rate, cfg["norm"] == "batch", cfg["norm"] == "layer", cfg["activation"], cfg["use_residual"])
