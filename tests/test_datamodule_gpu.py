"""End to end on the GPU: OneProtDataModule over temporary text and struct_token files, the text side tokenized by csrc/wordpiece.hip, two fit_steps of
the tiny towers of tests/test_step_parity_gpu.py, and the same batches from the host tokenizers."""
import csv
import functools
import json
import math
import os

import pytest
import torch

from tests.cases import esm_dir_from_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "protein", "bind", "##ing", "##s", "kinase", "a", ",", ".", "of", "zinc", "finger", "domain", "##like"]
WORDS = ["the", "protein", "binding", "binds", "kinase", "kinases", "a", ",", ".", "of", "zinc", "finger", "domain", "kinaselike", "membrane", "café"]
AA = "LAGVSERTIDPKQNFYMHWC"
FOLD = "pynwrqhgdlvtmfsaeikc"


def write_inputs(tmp_path, n=8):
    gen = torch.Generator().manual_seed(1881)
    pick = lambda letters, k: "".join(letters[int(i)] for i in torch.randint(0, len(letters), (k,), generator=gen))
    ids = [f"P{i}" for i in range(n)]
    seqs = {i: pick(AA, int(torch.randint(5, 30, (1,), generator=gen))) for i in ids}
    texts = {i: " ".join(WORDS[int(j)] for j in torch.randint(0, len(WORDS), (int(torch.randint(3, 40, (1,), generator=gen)),), generator=gen)) for i in ids}
    with open(tmp_path / "train_text.csv", "w", newline="") as f:
        csv.writer(f).writerows((i, texts[i]) for i in ids)
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    (tmp_path / "train_saprot.txt").write_text("\n".join(ids) + "\n")
    h5_seq = {i: {"structure": {"0": {"A": {"residues": {"seq1": seqs[i].encode()}}}}} for i in ids}
    h5_struct = {i: {"strucseq": "".join(a + b for a, b in zip(seqs[i], pick(FOLD + "#", len(seqs[i])))).encode()} for i in ids}
    return h5_seq, h5_struct


def build(tmp_path, h5_seq, h5_struct, device):
    from oneprot_amd.datamodule import OneProtDataModule
    cfg = {"struct_token": {"dataset": {"data_dir": str(tmp_path), "filename": h5_struct, "max_length": 24}, "batch_size": {"train": 4}, "attributes": {"device": device}},
           "text": {"dataset": {"data_dir": str(tmp_path), "text_tokenizer": str(tmp_path), "text_max_length": 20, "max_length": 24}, "batch_size": {"train": 4},
                    "attributes": {"device": device}}}
    dm = OneProtDataModule(cfg, num_workers=0, pin_memory=False, default_batch_size=4)
    dm.setup()
    dm.datasets["text_train"].h5_file = h5_seq
    torch.manual_seed(7)
    return list(dm.train_dataloader())


def test_data_module_to_two_fit_steps(golden_dir, tmp_path, monkeypatch):
    for k, v in dict(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1").items():
        monkeypatch.setenv(k, v)
    from oneprot_amd.optim import FusedAdam
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.components.text_encoder import TextEncoder
    from src.models.oneprot_module import OneProtLitModule
    h5_seq, h5_struct = write_inputs(tmp_path)
    batches = build(tmp_path, h5_seq, h5_struct, DEV)
    want = build(tmp_path, h5_seq, h5_struct, "cpu")
    assert len(batches) == len(want) == 2
    for got, ref in zip(batches, want):
        assert set(got) == set(ref) == {"struct_token", "text"}
        for m in got:
            assert got[m][0].is_cuda and got[m][1].is_cuda and not ref[m][0].is_cuda and got[m][2] == ref[m][2] == m and got[m][3] == ref[m][3]
            assert got[m][0].dtype == got[m][1].dtype == torch.int64
            assert torch.equal(got[m][0].cpu(), ref[m][0]) and torch.equal(got[m][1].cpu(), ref[m][1])
        assert int((got["text"][1] == 1).sum()) > 0 and int((got["text"][1] > 4).sum()) > int((got["text"][1] == 1).sum())       # some [UNK], mostly pieces
    g = torch.load(os.path.join(golden_dir, "esm_pair_hd16.pt"), weights_only=False)
    tb = torch.load(os.path.join(golden_dir, "bert_text.pt"), weights_only=False)
    p = esm_dir_from_cfg(str(tmp_path), g["cfg"], "esm")
    pb = os.path.join(str(tmp_path), "bert")
    os.makedirs(pb)
    c = tb["cfg"]
    with open(os.path.join(pb, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=c["vocab"], hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                       intermediate_size=c["ffn"], max_position_embeddings=c["max_pos"], pad_token_id=0, layer_norm_eps=c["eps"]), f)
    seq = SequenceEncoder(p, output_dim=48, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True)
    st = StructTokenEncoder(p, output_dim=48, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    tx = TextEncoder(pb, output_dim=48, pooling_type="cls", proj_type="mlp", use_logit_scale=True, frozen=True, use_lora=False)
    seq.load_state_dict(g["sd_seq"]); st.load_state_dict(g["sd_st"]); tx.load_state_dict(tb["sd"])
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st, "text": tx}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True).to(DEV)
    loss = module.fit_steps(batches)
    assert module.global_step == 4 and torch.isfinite(loss)


def test_train_script_runs_two_steps_validates_and_writes_a_checkpoint(golden_dir, tmp_path, monkeypatch):
    """src/train.py's train() on a config given as a dict: instantiate, two fit_steps over the data module, the validation hooks, the weights checkpoint"""
    for k, v in dict(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1").items():
        monkeypatch.setenv(k, v)
    from src import train
    from oneprot_amd.data import load_weights_only
    h5_seq, h5_struct = write_inputs(tmp_path)
    with open(tmp_path / "val_text.csv", "w", newline="") as f:
        csv.writer(f).writerows((f"P{i}", "the zinc finger domain binds a kinase .") for i in range(3))
    (tmp_path / "val_saprot.txt").write_text("P0\nP1\nP2\n")
    g = torch.load(os.path.join(golden_dir, "esm_pair_hd16.pt"), weights_only=False)
    c = torch.load(os.path.join(golden_dir, "bert_text.pt"), weights_only=False)["cfg"]
    p = esm_dir_from_cfg(str(tmp_path), g["cfg"], "esm")
    pb = os.path.join(str(tmp_path), "bert")
    os.makedirs(pb)
    with open(os.path.join(pb, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=c["vocab"], hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                       intermediate_size=c["ffn"], max_position_embeddings=c["max_pos"], pad_token_id=0, layer_norm_eps=c["eps"]), f)
    enc = "src.models.components."
    cfg = {"seed": 1881, "trainer": {"max_steps": 2}, "paths": {"output_dir": str(tmp_path / "out")},
           "data": {"_target_": "src.data.oneprot_datamodule.OneProtDataModule", "num_workers": 4, "pin_memory": False, "default_batch_size": 4,
                    "modalities": {"struct_token": {"dataset": {"data_dir": str(tmp_path), "filename": h5_struct, "max_length": 24}, "attributes": {"device": DEV}},
                                   "text": {"dataset": {"data_dir": str(tmp_path), "text_tokenizer": str(tmp_path), "text_max_length": 20, "max_length": 24},
                                            "attributes": {"device": DEV, "h5_file": h5_seq}}}},
           "model": {"_target_": "src.models.oneprot_module.OneProtLitModule", "loss_fn": "CLIP", "use_l1_regularization": True,
                     "optimizer": {"_target_": "oneprot_amd.optim.FusedAdam", "_partial_": True, "lr": 1e-3},
                     "components": {"sequence": {"_target_": enc + "sequence_encoder.SequenceEncoder", "model_name_or_path": p, "output_dim": 48, "pooling_type": "mean",
                                                 "proj_type": "mlp", "use_lora": False, "frozen": True},
                                    "struct_token": {"_target_": enc + "struct_token_encoder.StructTokenEncoder", "model_name_or_path": p, "output_dim": 48,
                                                     "pooling_type": "mean", "proj_type": "linear", "use_logit_scale": True},
                                    "text": {"_target_": enc + "text_encoder.TextEncoder", "model_name_or_path": pb, "output_dim": 48, "pooling_type": "cls",
                                             "proj_type": "mlp", "use_logit_scale": True, "frozen": True, "use_lora": False}}}}
    module, datamodule = train.train(cfg, DEV)
    assert module.global_step == 4 and datamodule.num_workers == 0                     # two steps of two sub-steps
    assert math.isfinite(float(module.train_loss.compute())) and math.isfinite(float(module.val_loss_best.compute()))
    path = tmp_path / "out" / "last.ckpt"
    assert path.exists()
    before = {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}
    load_weights_only(module, str(path))
    assert all(torch.equal(before[k], v.detach().cpu()) for k, v in module.state_dict().items())
