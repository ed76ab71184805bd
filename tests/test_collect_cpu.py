"""Embedding collection, host side (oneprot_amd/collect.py): the tokenizer against HF's EsmTokenizer, the batch plan, the CSV reader, the file layout against
downstream.load_data, the config."""
import json
import os
import random

import numpy as np
import pytest
import torch

from oneprot_amd import collect as C
from oneprot_amd import downstream, hip
from oneprot_amd.msa_data import LETTERS, MsaBatchConverter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ tokenizer
@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, "esm_tokenizer.json")) as f:
        return json.load(f)


def _rows(tok, strings, max_length=1024):
    flat, off = tok.encode_all(strings, max_length)
    return [flat[off[i]:off[i + 1]].tolist() for i in range(len(strings))]


def test_tokenizer_equals_hf_fixture(fixture):
    assert set(fixture) == {"strings", "ids"} and len(fixture["strings"]) == len(fixture["ids"]) >= 40
    tok = C.EsmSequenceTokenizer()
    assert _rows(tok, fixture["strings"]) == fixture["ids"]
    for s, ref in zip(fixture["strings"], fixture["ids"]):            # one by one: the result does not depend on what else is in the split
        assert _rows(tok, [s]) == [ref]
    padded = tok(fixture["strings"])
    assert padded.dtype == torch.int64 and padded.shape == (len(fixture["ids"]), 1024)
    for row, ref in zip(padded.tolist(), fixture["ids"]):
        assert row[:len(ref)] == ref and all(v == 1 for v in row[len(ref):])


def test_fixture_covers_every_rule(fixture):
    ss, ids = fixture["strings"], dict(zip(fixture["strings"], fixture["ids"]))
    vocab, space = set(LETTERS), set(" \t\n")
    plain = [s for s in ss if s and set(s) <= vocab]
    assert set("".join(plain)) == vocab                                 # all 25 letters plus . and -
    oov = lambda s: [c not in vocab and c not in space for c in s]
    no_special = [s for s in ss if "<" not in s and s.strip()]
    runs = lambda s: [len(r) for r in "".join("x" if o else " " for o in oov(s)).split()]
    assert any(runs(s) == [1] and s == s.upper() for s in no_special)                          # a single OOV character
    assert any(max(runs(s), default=0) > 1 and s == s.upper() for s in no_special)             # an OOV run
    assert any(oov(s)[0] and not all(oov(s)) for s in no_special) and any(oov(s)[-1] and not all(oov(s)) for s in no_special)
    assert any(s != s.upper() for s in no_special)                                              # lower case
    assert any(" " in s for s in ss) and any("\t" in s for s in ss)
    assert any("<mask>" in s and 32 in ids[s] for s in ss)
    assert "" in ids and ids[""] == [0, 2]
    assert {len(s) for s in plain} >= {1021, 1022, 1023, 1500}
    assert all(len(v) <= 1024 and v[0] == 0 and v[-1] == 2 for v in ids.values())
    assert len(ids[next(s for s in plain if len(s) == 1021)]) == 1023 and len(ids[next(s for s in plain if len(s) == 1500)]) == 1024
    # the rules tokenize_sequences does not follow are in there: it would fail this fixture
    from oneprot_amd.graph_data import tokenize_sequences
    differ = [s for s in ss if s and tokenize_sequences([s], 1024)[0].tolist() != ids[s]]
    assert len(differ) >= 10


def test_tokenizer_equals_hf_on_random_strings(tmp_path):
    transformers = pytest.importorskip("transformers")
    path = os.path.join(str(tmp_path), "vocab.txt")
    with open(path, "w") as f:
        f.write("\n".join(MsaBatchConverter.all_toks))
    hf = transformers.EsmTokenizer(path)
    alphabet = LETTERS + "Jmk*1 \t\n<>a_é"
    assert len(alphabet) == 40
    rng = random.Random(7)
    strings = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 48))) for _ in range(200)]
    strings[::7] = [s.replace("<", "<mask>").replace(">", "<eos>") for s in strings[::7]]
    ref = [hf(s, truncation=True, max_length=32)["input_ids"] for s in strings]
    for tok in (C.EsmSequenceTokenizer(), C.EsmSequenceTokenizer(path)):        # the built-in table and the same table read from a vocab.txt
        assert _rows(tok, strings, 32) == ref


def test_tokenizer_vocab_file_and_errors(tmp_path):
    path = os.path.join(str(tmp_path), "vocab.txt")
    with open(path, "w") as f:
        f.write("\n".join(["<pad>", "<cls>", "<eos>", "<unk>", "A", "AB", "ABC", "C"]))
    tok = C.EsmSequenceTokenizer(path)
    assert _rows(tok, ["ABCAB", "ABD", "xAy z"]) == [[1, 6, 5, 2], [1, 5, 3, 2], [1, 3, 4, 3, 3, 2]]      # leftmost-longest over the file's own entries
    assert tok(["A", "ABC C"]).tolist() == [[1, 4, 2, 0], [1, 6, 7, 2]]
    with pytest.raises(ValueError, match="<unk>"):
        C.EsmSequenceTokenizer(["<cls>", "<pad>", "<eos>", "A"])
    with pytest.raises(ValueError):
        C.EsmSequenceTokenizer().encode_all(["MK"], 1)
    flat, off = C.EsmSequenceTokenizer().encode_all([], 16)
    assert flat.size == 0 and off.tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------ plan
def _random_split(rng, n):
    aa = "LAGVSERTIDPKQNFYMHWC"
    return ["".join(rng.choice(aa) for _ in range(rng.choice([0, 1, 3, 17, 60, 61, 200, 1022, 1500]) + rng.randint(0, 2))) for _ in range(n)]


@pytest.mark.parametrize("seed,max_tokens,max_seqs", [(0, 1024, 4), (1, 2048, 8), (2, 4096, 1000), (3, 1024, 1)])
def test_plan_batches_properties(seed, max_tokens, max_seqs):
    rng = random.Random(seed)
    seqs = _random_split(rng, 150)
    tok = C.EsmSequenceTokenizer()

    def plan_of(rows):
        uniq, _ = C.unique_sequences(rows)
        flat, off = tok.encode_all(uniq)
        lengths = np.diff(off)
        batches = C.plan_batches(lengths, max_tokens, max_seqs)
        assert sorted(i for b in batches for i in b) == list(range(len(uniq)))            # every unique sequence exactly once
        assert all(sum(int(lengths[i]) for i in b) <= max_tokens and 1 <= len(b) <= max_seqs for b in batches)
        order = [i for b in batches for i in b]
        keys = [(int(lengths[i]), uniq[i].encode()) for i in order]
        assert keys == sorted(keys)                                                         # canonical: token count, then bytes
        for b, nxt in zip(batches[:-1], batches[1:]):                                       # greedy: the next sequence did not fit
            assert len(b) == max_seqs or sum(int(lengths[i]) for i in b) + int(lengths[nxt[0]]) > max_tokens
        # the same plan from unsorted input with explicit keys
        perm = list(range(len(uniq)))
        rng.shuffle(perm)
        shuffled = C.plan_batches([lengths[i] for i in perm], max_tokens, max_seqs, keys=[uniq[i] for i in perm])
        assert [[perm[i] for i in b] for b in shuffled] == batches
        return [[uniq[i] for i in b] for b in batches]

    base = plan_of(seqs)
    for _ in range(3):
        rows = list(seqs)
        rng.shuffle(rows)
        assert plan_of(rows) == base                                                        # any permutation of the file
    assert plan_of(seqs + [rng.choice(seqs) for _ in range(40)]) == base                    # added duplicates
    assert C.plan_sequences(seqs, 1024, max_tokens, max_seqs)["batches"] == C.plan_batches(np.diff(tok.encode_all(sorted(set(seqs)))[1]), max_tokens, max_seqs)


def test_plan_refuses_small_budget_and_ppi_uniqueness():
    with pytest.raises(ValueError, match="max_length"):
        C.plan_batches([5, 6], 1023, 8)
    with pytest.raises(ValueError, match="max_length"):
        C.plan_sequences(["MK"], 1024, 512, 8)
    assert C.plan_batches([5, 6], 64, 8, max_length=64) == [[0, 1]]
    with pytest.raises(ValueError):
        C.plan_batches([5], 1024, 0)
    uniq, (a, b) = C.unique_sequences(["MK", "TA", "MK"], ["TA", "GG", "MK"])         # ppi: one set over both columns
    assert uniq == ["GG", "MK", "TA"] and a.tolist() == [1, 2, 1] and b.tolist() == [2, 0, 1]


# ------------------------------------------------------------------------------------------------------------------ reader
def _write(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)
    return str(path)


CSVS = {
    "classification": ("name,sequence,label/fitness,stage\na,MKTA,3,train\nb,\"MK,TA\",0,train\n\nc,GG,7,train\n", ("sequence",), torch.int64, [3, 0, 7]),
    "regression": ("sequence,label/fitness\nMKTA,0.25\nGG,-1.5e-3\nTT,7\n", ("sequence",), torch.float32, [0.25, -1.5e-3, 7.0]),
    "multi-label": ("label/fitness,sequence\n\"[0, 1, 1]\",MKTA\n\"[1,0,0]\",GG\n", ("sequence",), torch.int32, [[0, 1, 1], [1, 0, 0]]),
    "ppi": ("sequence_1,sequence_2,label/fitness\nMKTA,GG,1\nGG,TT,0\n", ("sequence_1", "sequence_2"), torch.int64, [1, 0]),
}


@pytest.mark.parametrize("label_type", list(CSVS))
def test_read_task_csv(tmp_path, label_type):
    text, names, dtype, want = CSVS[label_type]
    path = _write(tmp_path / "x_train.csv", text)
    columns, labels = C.read_task_csv(path, label_type)
    assert len(columns) == len(names) and all(len(c) == len(want) for c in columns)
    assert labels.dtype == dtype and labels.tolist() == torch.tensor(want, dtype=dtype).tolist()
    if label_type == "classification":
        assert columns[0] == ["MKTA", "MK,TA", "GG"]
    if label_type == "ppi":
        assert columns == (["MKTA", "GG"], ["GG", "TT"])
    try:
        import pandas as pd
    except ImportError:
        return
    df = pd.read_csv(path)                                                # the reference's reader (SequenceDataset)
    for name, col in zip(names, columns):
        assert df[name].tolist() == col
    if label_type == "multi-label":
        import ast
        ref = torch.tensor(df["label/fitness"].apply(ast.literal_eval).tolist(), dtype=torch.int32)
    else:
        ref = torch.tensor(df["label/fitness"].values, dtype=dtype)
    assert torch.equal(ref, labels)


def test_read_task_csv_errors(tmp_path):
    p = _write(tmp_path / "a_train.csv", "sequence,label\nMK,1\n")
    with pytest.raises(ValueError, match="label/fitness"):
        C.read_task_csv(p, "classification")
    p = _write(tmp_path / "b_train.csv", "sequence,label/fitness\nMK,1\n")
    with pytest.raises(ValueError, match="sequence_1"):
        C.read_task_csv(p, "ppi")
    with pytest.raises(ValueError, match="ranking"):
        C.read_task_csv(p, "ranking")
    p = _write(tmp_path / "c_train.csv", "sequence,label/fitness\nMK,\"[0, 1]\"\nGG,\"[1]\"\n")
    with pytest.raises(ValueError, match="ragged"):
        C.read_task_csv(p, "multi-label")
    p = _write(tmp_path / "d_train.csv", "sequence,label/fitness\nMK,\"[0, 1\"\n")
    with pytest.raises(ValueError):
        C.read_task_csv(p, "multi-label")


def test_split_of():
    assert C.split_of("/data/EC/AF2_normal_train.csv") == "train"
    assert C.split_of("/data/train/AF2_normal_VALID.csv") == "valid"              # the basename only, lower-cased
    assert C.split_of("Comb826_test_seq.csv") == "test"
    assert C.split_of("latest_train.csv") == "train"                              # holds "test" too: train is asked first
    assert C.split_of("valid_test.csv") == "valid"
    with pytest.raises(ValueError):
        C.split_of("/data/train/holdout.csv")


# ------------------------------------------------------------------------------------------------------------------ files
def test_shards_and_combined_round_trip_through_load_data(tmp_path):
    emb_dir = str(tmp_path / "emb")
    cfg = {"output_dir": emb_dir + "/{model_name}", "batch_size": 2, "single_batch_mode": False, "tasks": {"EC": {"label_type": "multi-label"}}}
    model_cfg = {"name": "oneprot"}
    g = torch.Generator().manual_seed(0)
    want = {}
    for split, n in (("train", 23), ("valid", 5), ("test", 2)):
        emb, labels = torch.randn(n, 6, generator=g), torch.randint(0, 2, (n, 4), generator=g, dtype=torch.int32)
        shard_dir = os.path.join(emb_dir, "oneprot", "EC", split, "single_embs")
        assert C.write_shards(shard_dir, emb, labels, 2) == -(-n // 2)
        assert sorted(os.listdir(shard_dir)) == sorted(f"embeddings_rank0_batch{i}.pt" for i in range(-(-n // 2)))
        one = torch.load(os.path.join(shard_dir, "embeddings_rank0_batch1.pt"), weights_only=True) if n > 2 else None
        if one is not None:
            assert torch.equal(one["embeddings"], emb[2:4]) and one["embeddings"].untyped_storage().nbytes() == 2 * 6 * 4        # the slice, not its parent
        out = C.collect_task(cfg, model_cfg, "EC", f"/nowhere/AF2_{split}.csv")          # combining reads no CSV and loads no model
        assert out == os.path.join(emb_dir, "oneprot", "EC", split, f"EC_{split}_embeddings_labels.pt")
        want[split] = (emb, labels)
    data = downstream.load_data({"emb_dir": emb_dir, "model_type": "oneprot", "task_name": "EC", "evaluate_on": ["train", "valid", "test"],
                                 "threshold": float("-inf")})
    for split, (emb, labels) in want.items():                               # batch10, batch11 after batch2 ... batch9: numeric order is CSV order
        assert data[f"{split}_emb"].dtype == np.float32 and np.array_equal(data[f"{split}_emb"], emb.numpy())
        assert data[f"{split}_target"].dtype == np.int32 and np.array_equal(data[f"{split}_target"], labels.numpy())
    # a second, shorter run leaves no shard of the first behind
    shard_dir = os.path.join(emb_dir, "oneprot", "EC", "train", "single_embs")
    C.write_shards(shard_dir, want["train"][0][:3], want["train"][1][:3], 2)
    assert len(os.listdir(shard_dir)) == 2


def test_combine_takes_reference_shards_and_skips_missing(tmp_path, caplog):
    shard_dir = str(tmp_path / "single_embs")
    out = str(tmp_path / "combined.pt")
    with caplog.at_level("INFO", logger="oneprot_amd.collect"):
        assert C.combine_shards(shard_dir, out) is False                    # missing
        os.makedirs(shard_dir)
        assert C.combine_shards(shard_dir, out) is False                    # empty
    assert "Skipping" in caplog.text and not os.path.exists(out)
    rows = {}
    for rank, batch in ((1, 0), (0, 10), (0, 2), (0, 0), (1, 2)):
        rows[(rank, batch)] = torch.full((2, 3), float(rank * 100 + batch))
        torch.save({"embeddings": rows[(rank, batch)], "labels_fitness": torch.full((2,), rank * 100 + batch)},
                   os.path.join(shard_dir, f"embeddings_rank{rank}_batch{batch}.pt"))
    assert C.combine_shards(shard_dir, out) is True
    both = torch.load(out, weights_only=True)
    assert both["labels_fitness"].tolist() == [0, 0, 2, 2, 10, 10, 100, 100, 102, 102]
    assert both["embeddings"][:, 0].tolist() == [0, 0, 2, 2, 10, 10, 100, 100, 102, 102]


# ------------------------------------------------------------------------------------------------------------------ config, errors
def test_config_composes_with_the_known_keys():
    from oneprot_amd.config import compose
    cfg = compose(os.path.join(ROOT, "configs"), "collect_embeddings")
    assert set(cfg) == set(C.CONFIG_KEYS)
    assert "{model_name}" in cfg["output_dir"] and isinstance(cfg["batch_size"], int) and isinstance(cfg["single_batch_mode"], bool)
    assert all("name" in m for m in cfg["models"])
    for task, t in cfg["tasks"].items():
        assert t["label_type"] in C.LABEL_TYPES and [C.split_of(p) for p in t["csv_files"]] == ["train", "valid", "test"]


def test_script_reexports_the_module():
    import src.collect_embeddings as S
    assert S.embed_sequences is C.embed_sequences and S.collect_task is C.collect_task and callable(S.main)


def test_embed_sequences_refusals(tmp_path, monkeypatch):
    from tests.cases import esm_dir
    from oneprot_amd.encoders import SequenceEncoder
    monkeypatch.setenv("ONEPROT_ALLOW_RANDOM_INIT", "1")
    enc = SequenceEncoder(esm_dir(tmp_path, "esm", 1, 320, 20, 640), output_dim=32, proj_type="linear", use_lora=False)
    enc.train()
    for kind in ("oneprot", "esm2"):
        with pytest.raises((hip.HipKernelError, hip.HipLibraryMissing)):
            C.embed_sequences(enc, ["MKTA"], kind)
    assert enc.training
    with pytest.raises(NotImplementedError, match="446"):
        C.embed_sequences(enc, ["MKTA"], "saprot")
    with pytest.raises(NotImplementedError, match="446"):
        C.load_model({}, {"name": "saprot"})
    with pytest.raises(ValueError):
        C.embed_sequences(enc, ["MKTA"], "esm1b")
    with pytest.raises(OSError):                                            # as SequenceEncoder("not/a-model")
        C.load_model({"esm_model": "not/a-model"}, {"name": "esm2"})
    with pytest.raises(FileNotFoundError):
        C.load_model({}, {"name": "mine", "config_path": str(tmp_path / "none.yaml"), "ckpt_path": None})
