#!/usr/bin/env python
"""Device against host for the BERT WordPiece tokenizer: writes profiles/text_tokenize.json.

Three paths on the same texts, alternating in one process, every timed window closed by a device synchronise:
  device      BertWordPieceTokenizer.encode_device: the UTF-8 encode, the copy of the bytes and the offsets to the GPU and the one launch (csrc/wordpiece.hip);
  tokenizers  `tokenizers.BertWordPieceTokenizer.encode_batch` (HF's fast tokenizer, the reference's path) on the box's threads (RAYON_NUM_THREADS, else OMP_NUM_THREADS, else 16), where it imports;
  host_rule   BertWordPieceTokenizer.encode_all, the library's host path, one thread, with its word cache cleared before every call.
Texts are drawn from a fixed word list (whole words, words split into pieces, a few unknown ones) so that the share of [UNK] is small, long enough to be
truncated at 512 tokens.  Shapes: 256 texts (the bench's cfg-4 batch) and 16 texts (the shipped config's batch), then single texts from 64 bytes upwards
for the crossover behind text_data.DEVICE_MIN_BYTES.  --bench-line FILE: the JSON line of `bench.py --gpus 1 --pair text` from the same box; the file
then records whether the device call is below that run's sub-step time.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oneprot_amd import text_data as T  # noqa: E402

STEMS = ("protein kinase domain bind catalytic activity membrane receptor transport zinc finger nuclear cytoplasm signal peptide enzyme substrate complex "
         "subunit regulate transcription factor dna rna repair replication cell cycle apoptosis pathway phosphorylate ubiquitin ligase hydrolase transferase "
         "oxidoreductase mitochondrial ribosomal synthase atp gtp calcium ion channel the of and in to a is that by with for as this from which may be involved "
         "required response stress growth development human mouse yeast homolog family member conserved region terminal residue site active").split()
SUFFIXES = ["s", "ing", "ed", "ion", "like", "ase", "al", "ly"]
UNKNOWN = ["xq7z", "zzvq", "qxj"]


def vocabulary():
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + sorted(set(STEMS)) + ["##" + s for s in SUFFIXES] + list(",.;:()-/%") + [str(d) for d in range(10)]
    return vocab + ["##" + str(d) for d in range(10)]


def draw_texts(seed, n, words_each):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        words = []
        for _ in range(words_each):
            r = rng.random()
            if r < 0.62:
                words.append(rng.choice(STEMS))
            elif r < 0.86:
                words.append(rng.choice(STEMS) + rng.choice(SUFFIXES))
            elif r < 0.93:
                words.append(rng.choice(",.;:()-/%"))
            elif r < 0.98:
                words.append(str(rng.randrange(1000)))
            else:
                words.append(rng.choice(UNKNOWN))
        out.append(" ".join(words).capitalize())
    return out


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), reps=len(xs))


def host_rule(tok, texts, max_length):
    tok._words.clear()
    return tok.encode_all(texts, max_length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-length", type=int, default=512)
    ap.add_argument("--words", type=int, default=520, help="words per text: more than max_length pieces, so every text is truncated")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--bench-line", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_tokenize.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_tokenize_ab.py measures the device path: no GPU, no number")
    dev = torch.device("cuda:0")
    vocab = vocabulary()
    tok = T.BertWordPieceTokenizer(vocab)
    threads = os.environ.get("RAYON_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS") or "16"          # the box's share of the host, not the host's core count
    os.environ["RAYON_NUM_THREADS"] = threads
    try:
        import tempfile

        import tokenizers
        tmp = tempfile.mkdtemp()
        with open(os.path.join(tmp, "vocab.txt"), "w") as f:
            f.write("\n".join(vocab) + "\n")
        fast = tokenizers.BertWordPieceTokenizer(os.path.join(tmp, "vocab.txt"), lowercase=True)
        fast.enable_truncation(max_length=a.max_length)
        fast.enable_padding()
        fast_note = f"tokenizers {tokenizers.__version__}, encode_batch, {threads} threads"
    except ImportError:
        fast, fast_note = None, "tokenizers is not importable on this box: the device call is reported against the host rule only"
    out = dict(device=torch.cuda.get_device_name(0), max_length=a.max_length, words_per_text=a.words, vocab=len(vocab), tokenizers=fast_note, shapes={}, single_text={})
    tok.encode_device(draw_texts(0, 4, 50), a.max_length, dev)                       # code object, tables on the device, the pinned allocator
    torch.cuda.synchronize()
    for B in (256, 16):
        texts = draw_texts(B, B, a.words)
        n_bytes = sum(len(t.encode("utf-8")) for t in texts)
        times = dict(device=[], tokenizers=[], host_rule=[])
        sync_time(lambda: tok.encode_device(texts, a.max_length, dev))
        for rep in range(a.reps):
            t, (ids, lengths) = sync_time(lambda: tok.encode_device(texts, a.max_length, dev))
            times["device"].append(t)
            if fast is not None:
                t0 = time.perf_counter()
                enc = fast.encode_batch(texts)
                times["tokenizers"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            flat, off = host_rule(tok, texts, a.max_length)
            times["host_rule"].append((time.perf_counter() - t0) * 1e3)
        lens = lengths.cpu().tolist()
        dev_rows = [row[:n] for row, n in zip(ids.cpu().tolist(), lens)]
        rec = dict(texts=B, bytes=n_bytes, tokens=sum(lens), unk_share=sum(r.count(tok.unk_id) for r in dev_rows) / sum(lens),
                   device=stats(times["device"]), host_rule=stats(times["host_rule"]),
                   device_equals_host_rule=dev_rows == [flat[x:y].tolist() for x, y in zip(off[:-1], off[1:])])
        rec["host_rule_over_device"] = rec["host_rule"]["median_ms"] / rec["device"]["median_ms"]
        if fast is not None:
            rec["tokenizers"] = stats(times["tokenizers"])
            rec["tokenizers_over_device"] = rec["tokenizers"]["median_ms"] / rec["device"]["median_ms"]
            rec["device_equals_tokenizers"] = dev_rows == [[i for i, m in zip(e.ids, e.attention_mask) if m] for e in enc]
        out["shapes"][f"b{B}"] = rec
        print(f"B {B}: {n_bytes} bytes, {rec['tokens']} tokens, device {rec['device']['median_ms']:.3f} ms, tokenizers "
              f"{rec.get('tokenizers', {}).get('median_ms', float('nan')):.3f} ms, host rule {rec['host_rule']['median_ms']:.3f} ms, [UNK] {rec['unk_share']:.3%}", flush=True)
    for words in (8, 16, 32, 64, 128, 256, 512, 1024, 4096):                            # one text: where the device starts to pay
        texts = draw_texts(words, 1, words)
        d, h = [], []
        sync_time(lambda: tok.encode_device(texts, 1 << 15, dev))
        for _ in range(max(a.reps, 9)):
            d.append(sync_time(lambda: tok.encode_device(texts, 1 << 15, dev))[0])
            t0 = time.perf_counter()
            host_rule(tok, texts, 1 << 15)
            h.append((time.perf_counter() - t0) * 1e3)
        n_bytes = len(texts[0].encode("utf-8"))
        out["single_text"][str(n_bytes)] = dict(bytes=n_bytes, device=stats(d), host_rule=stats(h))
        print(f"single text of {n_bytes} bytes: device {statistics.median(d):.3f} ms, host rule {statistics.median(h):.3f} ms", flush=True)
    faster = [int(k) for k, v in out["single_text"].items() if v["device"]["median_ms"] < v["host_rule"]["median_ms"]]
    out["smallest_bytes_where_device_wins"] = min(faster) if faster else None
    out["DEVICE_MIN_BYTES"] = T.DEVICE_MIN_BYTES
    if a.bench_line:
        with open(a.bench_line) as f:
            line = [json.loads(s) for s in f.read().splitlines() if s.startswith("{")][-1]
        substep = 256 / float(line["value"]) * 1e3
        out["cfg4"] = dict(source="bench.py --gpus 1 --pair text on the same box", pairs_per_s=line["value"], substep_ms_b256=substep,
                           device_tokenize_ms_b256=out["shapes"]["b256"]["device"]["median_ms"],
                           device_call_below_substep=out["shapes"]["b256"]["device"]["median_ms"] < substep)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v["device"]["median_ms"] for k, v in out["shapes"].items()}))


if __name__ == "__main__":
    main()
