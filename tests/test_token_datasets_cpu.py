"""The text, struct_token and seqsim datasets, OneProtDataModule and src/train.py on the host: the pinned tokenizers and collate
(tests/golden/struct_token_tokenizer.json, seqsim_collate.json), nested-mapping and temporary-file inputs, missing ids, remove_hash, full, the CSV
reader against pandas, batch sizes, loader modes and skip-on-error.  The HDF5 branch (a path opened with h5py) runs only where h5py imports."""
import inspect
import json
import logging
import os
import random

import pytest
import torch

from oneprot_amd import datamodule as dm_mod
from oneprot_amd.collect import EsmSequenceTokenizer
from oneprot_amd.data import CombinedLoader
from oneprot_amd.datamodule import DATASET_CLASSES, OneProtDataModule
from oneprot_amd.msa_data import MsaBatchConverter
from oneprot_amd.packing import PackedTokens
from oneprot_amd.text_data import BertWordPieceTokenizer, TextDataset, read_csv_rows, sequence_tokenizer
from oneprot_amd.token_data import NEW_TOKENS, SequenceSimDataset, StructTokenDataset

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "the", "protein", "bind", "##ing", "##s", "kinase", "a", ",", ".", "of", "zinc"]


def golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def seq_entry(seq):
    return {"structure": {"0": {"A": {"residues": {"seq1": seq.encode()}}}}}


# ---------------------------------------------------------------------------------------------------------------- the pinned tokenizers and collate
def test_struct_token_tokenizer_equals_its_fixture():
    g = golden("struct_token_tokenizer.json")
    assert g["new_tokens"] == NEW_TOKENS and g["new_token_ids"] == list(range(33, 54))
    tok = sequence_tokenizer("facebook/esm2_t33_650M_UR50D", NEW_TOKENS)
    assert tok.tokens == MsaBatchConverter.all_toks + NEW_TOKENS and [tok.token_to_id[t] for t in NEW_TOKENS] == g["new_token_ids"]
    assert any("#" in s for s in g["struct"]) and any(s and "#" not in s for s in g["struct"]) and any(s.isupper() for s in g["seq"])
    for strings, ids, t in ((g["struct"], g["struct_ids"], tok), (g["seq"], g["seq_ids"], sequence_tokenizer("anything"))):
        flat, off = t.encode_all(strings, 1024)
        for s, a, b, want in zip(strings, off[:-1], off[1:], ids):
            assert flat[a:b].tolist() == want, s[:30]
    assert any(len(i) == 1024 for i in g["struct_ids"])


def write_seqsim_dir(path, files):
    for name, text in files.items():
        (path / name).write_text(text)


def test_seqsim_collate_equals_its_fixture(tmp_path):
    g = golden("seqsim_collate.json")
    assert g["redrawn"] >= 1
    write_seqsim_dir(tmp_path, g["files"])
    ds = SequenceSimDataset(str(tmp_path), "train", max_length=g["max_length"])
    assert len(ds) == g["len"]
    seq_id, row = ds[1]
    assert seq_id == g["files"]["train_seqsim.txt"].split()[1] and set(row) == {"req_seq", "aligned_seq"}
    redrawn = [0]
    apply = SequenceSimDataset._apply_mutation

    def counting(sequence, mutation):
        try:
            return apply(sequence, mutation)
        except AssertionError:
            redrawn[0] += 1
            raise
    ds._apply_mutation = counting
    for b in g["batches"]:
        random.seed(b["seed"])
        one, two, modality, raw = ds.collate_fn([ds[i] for i in b["indices"]])
        assert modality == "seqsim" and raw is one and one.dtype == two.dtype == torch.int64
        assert one.tolist() == b["input1"] and two.tolist() == b["input2"]
    assert redrawn[0] == g["redrawn"]
    # val / test: min(1000, rows), where the reference returns 1000 and indexes past a shorter file
    for name in ("seqsim.txt", "msa_seqsim.csv"):
        (tmp_path / f"val_{name}").write_text(g["files"][f"train_{name}"])
    assert len(SequenceSimDataset(str(tmp_path), "val")) == g["len"] < 1000
    ds.packed = True
    random.seed(0)
    one, two, _, raw = ds.collate_fn([ds[0]])
    assert isinstance(one, PackedTokens) and raw is one and len(one) == len(two) == 3


def test_constructor_signatures_are_the_references():
    want = {TextDataset: ["data_dir", "split", "max_length", "text_max_length", "text_tokenizer", "seq_tokenizer"],
            StructTokenDataset: ["data_dir", "filename", "split", "max_length", "seq_tokenizer", "remove_hash", "full"],
            SequenceSimDataset: ["data_dir", "split", "seq_tokenizer", "max_length", "modality"],
            OneProtDataModule: ["modalities", "num_workers", "pin_memory", "default_batch_size"]}
    defaults = {TextDataset: {"max_length": 1024, "text_max_length": 512, "text_tokenizer": "allenai/scibert_scivocab_uncased", "seq_tokenizer": "facebook/esm2_t33_650M_UR50D"},
                StructTokenDataset: {"max_length": 1024, "seq_tokenizer": "facebook/esm2_t33_650M_UR50D", "remove_hash": True, "full": False},
                SequenceSimDataset: {"seq_tokenizer": "facebook/esm2_t33_650M_UR50D", "max_length": 1024, "modality": "combined_seqsim_msa"}}
    for cls, names in want.items():
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1:] == names
        for k, v in defaults.get(cls, {}).items():
            assert params[k].default == v
    if os.path.isdir(os.path.join(REF, "src")):                      # the same from the reference's source text, where a checkout is at hand
        import ast
        for rel, cls in (("text_dataset.py", TextDataset), ("struct_token_dataset.py", StructTokenDataset), ("seqsim_dataset.py", SequenceSimDataset)):
            tree = ast.parse(open(os.path.join(REF, "src", "data", "datasets", rel)).read())
            init = next(n for c in tree.body if isinstance(c, ast.ClassDef) for n in c.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
            assert [a.arg for a in init.args.args][1:] == want[cls]
    import src.data.datasets.seqsim_dataset as a
    import src.data.datasets.struct_token_dataset as b
    import src.data.datasets.text_dataset as c
    import src.data.oneprot_datamodule as d
    assert a.SequenceSimDataset is SequenceSimDataset and b.StructTokenDataset is StructTokenDataset and c.TextDataset is TextDataset
    assert d.OneProtDataModule is OneProtDataModule and set(d.DATASET_CLASSES) == {"msa", "struct_graph", "pocket", "text", "struct_token", "seqsim"}


# ---------------------------------------------------------------------------------------------------------------- text
TEXT_ROWS = [("P1", "the protein binding kinases"), ("P2", 'a "zinc" kinase, of the protein.'), ("P3", "binds\nthe protein"), ("P1", "the second row of P1"),
             ("P4", "the zinc")]


def write_text_dir(path, split="train", rows=TEXT_ROWS):
    import csv
    with open(path / f"{split}_text.csv", "w", newline="") as f:
        csv.writer(f).writerows(rows)
    (path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")


def test_text_dataset(tmp_path):
    write_text_dir(tmp_path)
    ds = TextDataset(str(tmp_path), "train", max_length=12, text_max_length=8, text_tokenizer=str(tmp_path / "vocab.txt"))
    assert len(ds) == 5 and [ds[i] for i in range(5)] == ["P1", "P2", "P3", "P1", "P4"]
    rows = read_csv_rows(tmp_path / "train_text.csv")
    assert [tuple(r) for r in rows] == TEXT_ROWS
    pd = pytest.importorskip("pandas")
    df = pd.read_csv(tmp_path / "train_text.csv", header=None)
    assert df[0].tolist() == [r[0] for r in rows] and df[1].tolist() == [r[1] for r in rows]
    ds.h5_file = {"P1": seq_entry("MKTAYIAKQRQISFVKSHFSRQ"), "P2": seq_entry("LAGV"), "P3": {"structure": {"0": {"A": {"residues": {"seq1": "MK"}}}}}}
    ds.device = "cpu"
    seq, text, modality, raw = ds.collate_fn(["P2", "P4", "P1", "P3"])              # P4 is not in the structure file: both of its sides go
    assert modality == "text" and raw == ["LAGV", "MKTAYIAKQRQISFVKSHFSRQ", "MK"]
    assert seq.dtype == text.dtype == torch.int64 and seq.shape == (3, 12) and text.shape[0] == 3
    assert torch.equal(seq, EsmSequenceTokenizer()(raw, 12))
    tok = BertWordPieceTokenizer(VOCAB)
    assert torch.equal(text, tok([TEXT_ROWS[1][1], TEXT_ROWS[0][1], TEXT_ROWS[2][1]], max_length=8, device="cpu"))       # the first row of P1
    assert text.shape[1] == 8 and int(text[0, 0]) == 2 and int(text[0, -1]) == 3
    with pytest.raises(IndexError):
        ds.collate_fn(["P9"])
    ds.packed = ds.packed_text = True
    seq_p, text_p, _, _ = ds.collate_fn(["P2", "P4", "P1", "P3"])
    assert isinstance(seq_p, PackedTokens) and seq_p.pad_id == 1 and torch.equal(seq_p.to_padded(), seq)
    assert isinstance(text_p, PackedTokens) and text_p.pad_id == 0 and torch.equal(text_p.to_padded(), text)
    # val: min(1000, rows); a missing file: an empty dataset
    write_text_dir(tmp_path, "val", TEXT_ROWS[:2])
    assert len(TextDataset(str(tmp_path), "val", text_tokenizer=str(tmp_path))) == 2
    assert len(TextDataset(str(tmp_path), "test", text_tokenizer=str(tmp_path))) == 0
    with pytest.raises(ValueError, match="local path"):
        TextDataset(str(tmp_path), "train")
    try:
        import h5py  # noqa: F401
    except ImportError:
        ds.h5_file = str(tmp_path / "seqstruc.h5")
        with pytest.raises(ImportError, match="h5py"):
            ds.collate_fn(["P1"])


# ---------------------------------------------------------------------------------------------------------------- struct_token
def test_struct_token_dataset(tmp_path):
    (tmp_path / "train_saprot.txt").write_text("A1\nA2\nA3\nA9\n")
    (tmp_path / "train_saprot_full.txt").write_text("A1\nA2\nA3\nA9\nA4\n")
    (tmp_path / "val_saprot.txt").write_text("A1\nA2\n")
    h5 = {"A1": {"strucseq": b"MdKvTlAp"}, "A2": {"strucseq": b"M#KvT#Ap"}, "A3": {"strucseq": "#dKv"}, "A4": {"strucseq": b"Lc"}}
    ds = StructTokenDataset(str(tmp_path), h5, "train", max_length=8)
    assert len(ds) == 4 and ds[3] == "A9" and ds.remove_hash is True
    assert len(StructTokenDataset(str(tmp_path), h5, "train", full=True)) == 5
    assert len(StructTokenDataset(str(tmp_path), h5, "val", full=True)) == 2             # `full` is a train-only switch
    seq, struct, modality, raw = ds.collate_fn(["A1", "A9", "A2", "A3"])                  # A9 is not in the file
    assert modality == "struct_token" and raw == ["MKTA", "MKTA", "K"]
    assert torch.equal(seq, EsmSequenceTokenizer()(raw, 8))
    st = {t: 33 + i for i, t in enumerate(NEW_TOKENS)}
    assert struct.tolist() == [[0, st["d"], st["v"], st["l"], st["p"], 2], [0, st["v"], st["p"], 2, 1, 1], [0, st["d"], st["v"], 2, 1, 1]]
    keep = StructTokenDataset(str(tmp_path), h5, "train", max_length=8, remove_hash=False)
    _, struct2, _, raw2 = keep.collate_fn(["A2", "A3"])
    assert raw2 == ["MKTA", "K"] and struct2.tolist() == [[0, st["#"], st["v"], st["#"], st["p"], 2], [0, st["d"], st["v"], 2, 1, 1]]
    ds.max_length = 4
    seq3, struct3, _, _ = ds.collate_fn(["A1"])
    assert seq3.shape == struct3.shape == (1, 4) and int(struct3[0, -1]) == 2
    ds.packed = True
    seq4, struct4, _, _ = ds.collate_fn(["A1", "A2"])
    assert isinstance(seq4, PackedTokens) and isinstance(struct4, PackedTokens) and struct4.lengths == [4, 4]
    assert len(StructTokenDataset(str(tmp_path), h5, "test")) == 0                       # no test_saprot.txt: reported, an empty dataset


# ---------------------------------------------------------------------------------------------------------------- the data module
def module_config(tmp_path):
    write_text_dir(tmp_path)
    write_text_dir(tmp_path, "val", TEXT_ROWS[:3])
    (tmp_path / "train_saprot.txt").write_text("A1\nA2\nA3\nA1\nA2\nA3\nA1\n")
    (tmp_path / "val_saprot.txt").write_text("A1\nA2\n")
    return {"text": {"dataset": {"data_dir": str(tmp_path), "text_tokenizer": str(tmp_path), "text_max_length": 8, "max_length": 12},
                     "batch_size": {"train": 2, "val": 3}, "attributes": {"device": "cpu"}},
            "struct_token": {"dataset": {"_target_": "src.data.datasets.struct_token_dataset.StructTokenDataset", "data_dir": str(tmp_path),
                                         "filename": {"A1": {"strucseq": b"MdKvTlAp"}, "A2": {"strucseq": b"M#KvT#Ap"}, "A3": {"strucseq": b"LdKv"}}},
                             "batch_size": {"train": 3}},
            "seqsim": {"dataset": {"data_dir": str(tmp_path / "nowhere")}, "batch_size": {"train": 2}},
            "hologram": {"dataset": {}}}


def test_data_module(tmp_path, caplog):
    cfg = module_config(tmp_path)
    with caplog.at_level(logging.INFO, logger=dm_mod.__name__):
        dm = OneProtDataModule(cfg, num_workers=12, pin_memory=False, default_batch_size=4)
        dm.setup()
    assert dm.num_workers == 0 and "forced to 0" in caplog.text
    assert "Unknown modality: hologram" in caplog.text and "Error creating dataset for seqsim train" in caplog.text
    assert sorted(dm.datasets) == ["struct_token_test", "struct_token_train", "struct_token_val", "text_test", "text_train", "text_val"]
    assert dm.datasets["text_train"].device == "cpu" and dm.datasets["struct_token_train"].device is None
    h5 = {"P1": seq_entry("MKTA"), "P2": seq_entry("LAGV"), "P3": seq_entry("MK"), "P4": seq_entry("M")}
    for split in ("train", "val", "test"):
        dm.datasets[f"text_{split}"].h5_file = h5
    train = dm.train_dataloader()
    assert isinstance(train, CombinedLoader) and train.mode == "min_size" and set(train.iterables) == {"text", "struct_token"}
    assert train.iterables["text"].batch_size == 2 and train.iterables["struct_token"].batch_size == 3 and train.iterables["text"].num_workers == 0
    assert len(train) == 3                                            # text: 5 rows in 2s = 3 batches; struct_token: 7 ids in 3s = 3 batches
    torch.manual_seed(0)
    batches = list(train)
    assert len(batches) == 3 and all(set(b) == {"text", "struct_token"} for b in batches)
    assert sorted(s for b in batches for s in b["text"][3]) == sorted(["MKTA", "LAGV", "MK", "MKTA", "M"])          # shuffled, every row once
    assert [b["struct_token"][0].shape[0] for b in batches] == [3, 3, 1]
    val = dm.val_dataloader()
    assert val.mode == "sequential" and val.iterables["text"].batch_size == 3 and val.iterables["struct_token"].batch_size == 4       # the default
    out = list(val)
    assert [(bi, di, b[2]) for b, bi, di in out] == [(0, 0, "text"), (0, 1, "struct_token")]
    assert out[0][0][3] == ["MKTA", "LAGV", "MK"]                     # not shuffled
    assert len(dm.test_dataloader()) == 0
    dm.setup()                                                        # a second setup keeps the datasets
    assert dm.datasets["text_train"].h5_file is h5


def test_data_configs_and_train_script_compose(tmp_path):
    from oneprot_amd.config import compose, instantiate
    from src import train
    data = compose(os.path.join(ROOT, "configs"), "data/oneprot")["data"]
    assert data["_target_"] == "src.data.oneprot_datamodule.OneProtDataModule" and data["default_batch_size"] == 32 and data["pin_memory"] is False
    assert list(data["modalities"]) == ["pocket", "seqsim", "struct_graph", "text"]
    assert data["modalities"]["seqsim"] == {"dataset": {"data_dir": "/path/to/pretrain/datasets/", "seq_tokenizer": "facebook/esm2_t33_650M_UR50D", "max_length": 1024},
                                            "batch_size": {"train": 16, "val": 16, "test": 16}}
    if os.path.isdir(os.path.join(REF, "configs")):
        for name in ("data/default", "data/oneprot", "data/modalities/seqsim"):
            assert compose(os.path.join(ROOT, "configs"), name, resolve=False) == compose(os.path.join(REF, "configs"), name, resolve=False)
    header = open(os.path.join(ROOT, "configs", "data", "modalities", "struct_token.yaml")).read()
    assert "outside this build's scope" not in header and "StructTokenDataset" in header
    cfg = train.compose_config(["trainer.max_steps=3", "data.modalities.text.dataset.data_dir=/somewhere", "data.default_batch_size=8"])
    assert cfg["model"]["_target_"] == "src.models.oneprot_module.OneProtLitModule" and cfg["trainer"]["max_steps"] == 3
    assert cfg["data"]["modalities"]["text"]["dataset"]["data_dir"] == "/somewhere" and cfg["data"]["default_batch_size"] == 8
    dm = instantiate(cfg["data"])
    assert isinstance(dm, OneProtDataModule) and set(dm.modalities) == {"pocket", "seqsim", "struct_graph", "text"}
    assert set(train.compose_config(["model=oneprot_text"])["model"]["components"]) >= {"sequence", "text"}
    source = open(train.__file__).read()
    assert "lightning" not in source.lower().replace("without lightning", "") and "fit_steps" in source and "save_checkpoint" in source
