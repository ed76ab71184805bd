"""Cross-modal evaluation on the device (ref src/eval.py, configs/eval.yaml): one test table embedded in every modality, every modality pair ranked in both
directions, `retrieval_metrics.csv` written.  No pandas, Lightning, Hydra, sklearn, HF tokenizers, fair-esm or torch_geometric.

  read_table             the reference's `pd.read_csv(header=None, names=COLUMN_NAMES)` + drop of row 0, on Python's csv module: seven positional columns, the
                         first line dropped whatever it holds, every cell a string.  An empty or missing cell is "" (pandas gives NaN, which the reference's
                         tokenizers then refuse); ids stay strings, numeric-looking ones too.
  CombinedDataset        the reference's constructor, __len__, __getitem__ and collate_fn (its dict; graphs as a GraphBatch).  `device` None is the host path; a
                         device runs WordPiece and featurize_batch there.
  encode_inputs          the reference's loop over one collated batch, for users who call it.
  embed_modalities       the path main takes: a whole-dataset pass.  Token modalities: the distinct strings, tokenised once, filled into token budgets
                         (collect.plan_batches), every batch one PackedTokens stream (collect.run_plan).  Graph modalities: consecutive rows in file order.
  calculate_retrieval_metrics / write_results_to_csv     retrieval.retrieval_table with cosine similarity (L2-normalise + dot), the reference's file format.
  main                   python src/eval.py [--config configs/eval.yaml] key=value ...

Stated differences from the reference:
  * Missing ids.  A row whose struct_graph, pocket or sequence id its file does not hold is dropped from every modality and from `ids`, with one log line.
    The reference drops it from three of its lists and keeps it in the other two, which shifts every later row of that batch against its partner.
  * Ties.  Distinct strings are embedded once, so duplicate rows are bit-identical and tie exactly with the matching pair.  The table written to
    output.csv_path counts the optimistic rank (strict >); when any row ties, `<stem>_pessimistic.csv` holds rank + ties (oneprot_sim_rank_ties) next to it.
    The reference's number for such rows is whatever its unstable argsort did.
  * Graph batches.  ProNet's (i -+ 1) mod N neighbours wrap over the batch (unpinned choice 3), so a graph's first and last node see
    the batch composition, here as in the reference.  embed_modalities therefore keeps file order and closes a batch at `max_graphs` (default
    dataloader.batch_size): with max_nodes=None the compositions are the reference's.  A node budget changes them and, with them, those two nodes.
  * The MSA members the reference's dataset builds and never reads are not built; msa_model_name_or_path, msa_depth and max_length are accepted and ignored.

There is no CPU path for the towers: a CPU model raises hip.HipKernelError."""
import csv
import logging
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import collect, hip
from .graph_data import GraphBatch, _open, _value, featurize_batch, protein_to_graph, read_records
from .retrieval import retrieval_table
from .text_data import BertWordPieceTokenizer, as_str, sequence_tokenizer
from .token_data import NEW_TOKENS

logger = logging.getLogger(__name__)

COLUMN_NAMES = ("ids", "msa_files", "text", "struct_token", "struct_graph", "sequence", "pocket")
MODALITIES = ("sequence", "struct_token", "text", "struct_graph", "pocket")          # the keys of collate_fn's dict after `ids`, in its order
TOKEN_MODALITIES, GRAPH_MODALITIES = ("sequence", "struct_token", "text"), ("struct_graph", "pocket")
KS = (1, 10, 100, 500)
_TEXT_CHUNK = 65536                                                                    # texts per oneprot_wordpiece_encode launch of the whole-dataset pass


def _sub(cfg, key, default=None):
    """cfg[key] of a mapping or cfg.key of an attribute bag"""
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


# ---- 1. table ---------------------------------------------------------------------------------------------------------------------------------------------
def read_table(path):
    """the rows of the evaluation CSV as dicts over COLUMN_NAMES; the first line is dropped; blank lines are skipped, short rows are filled with "" """
    with open(path, newline="", encoding="utf-8") as f:
        rows = [row for row in csv.reader(f) if row]
    out = []
    for k, row in enumerate(rows[1:], start=2):
        if len(row) > len(COLUMN_NAMES):
            raise ValueError(f"{path}, record {k}: {len(row)} fields, the table has {len(COLUMN_NAMES)} columns ({', '.join(COLUMN_NAMES)})")
        out.append(dict(zip(COLUMN_NAMES, row + [""] * (len(COLUMN_NAMES) - len(row)))))
    return out


# ---- 2. dataset -------------------------------------------------------------------------------------------------------------------------------------------
class CombinedDataset(Dataset):
    """ref eval.py:27-112.  cfg.dataset: csv_file_path, data_dir, max_sequence_length, text_max_length, text_tokenizer (a local vocab.txt or a directory
    that holds one), seq_tokenizer (as text_data.sequence_tokenizer takes it), remove_hash; the MSA keys are ignored.  struct_file / pocket_file: a
    path (default <data_dir>/seqstruc.h5, <data_dir>/pockets_100_residues.h5; opened with h5py where it imports), an opened file or a nested mapping."""

    def __init__(self, cfg, struct_file=None, pocket_file=None):
        self.cfg = _sub(cfg, "dataset")
        c = self.cfg
        self.column_names = list(COLUMN_NAMES)
        self.data = read_table(_sub(c, "csv_file_path"))
        self.struct_h5_file = f"{_sub(c, 'data_dir')}/seqstruc.h5" if struct_file is None else struct_file
        self.pocket_h5_file = f"{_sub(c, 'data_dir')}/pockets_100_residues.h5" if pocket_file is None else pocket_file
        self.max_sequence_length = int(_sub(c, "max_sequence_length", 1024))
        self.text_max_length = int(_sub(c, "text_max_length", 512))
        self.remove_hash = bool(_sub(c, "remove_hash", True))
        self.sequence_tokenizer = sequence_tokenizer(_sub(c, "seq_tokenizer"))
        self.structure_tokenizer = sequence_tokenizer(_sub(c, "seq_tokenizer"), extra_tokens=NEW_TOKENS)
        self.text_tokenizer = BertWordPieceTokenizer(_sub(c, "text_tokenizer"))
        self.device = None

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        return self.data[index]

    def resolve(self, batch, records=False):
        """dict of lists over the rows of `batch` that all three files hold: ids, sequence (the strings of the structure file), struct_token (remove_hash
        applied), text, struct_graph and pocket -- GraphData per row, or with records=True the atom records featurize_batch takes.  A dropped row is logged."""
        out = {k: [] for k in ("ids",) + MODALITIES}
        struct_file, struct_opened = _open(self.struct_h5_file)
        try:
            pocket_file, pocket_opened = _open(self.pocket_h5_file)
            try:
                read = read_records if records else protein_to_graph
                for item in batch:
                    try:
                        seq = as_str(_value(struct_file[item["sequence"]]["structure"]["0"]["A"]["residues"]["seq1"]))
                        graph = read(item["struct_graph"], struct_file, "non_pdb", "A", pockets=False)
                        pocket = read(item["pocket"], pocket_file, "non_pdb", "A", pockets=True)
                    except KeyError:
                        logger.warning(f"row {item['ids']} dropped from every modality: sequence {item['sequence']}, struct_graph {item['struct_graph']} or "
                                       f"pocket {item['pocket']} is not in its file")
                        continue
                    out["ids"].append(item["ids"])
                    out["sequence"].append(seq)
                    out["struct_token"].append(item["struct_token"].replace("#", "") if self.remove_hash else item["struct_token"])
                    out["text"].append(item["text"])
                    out["struct_graph"].append(graph)
                    out["pocket"].append(pocket)
            finally:
                if pocket_opened:
                    pocket_file.close()
        finally:
            if struct_opened:
                struct_file.close()
        return out

    def collate_fn(self, batch):
        """ref eval.py:66-103: {ids, sequence, struct_token, text: int64 [B, longest] as padding=True, truncation=True give them; struct_graph, pocket: GraphBatch}"""
        on_device = self.device is not None and torch.device(self.device).type != "cpu"
        rows = self.resolve(batch, records=on_device)
        if not rows["ids"]:
            raise ValueError("CombinedDataset.collate_fn: every row of the batch was dropped")
        out = {"ids": rows["ids"],
               "sequence": self.sequence_tokenizer(rows["sequence"], self.max_sequence_length).long(),
               "struct_token": self.structure_tokenizer(rows["struct_token"], self.max_sequence_length).long(),
               "text": self.text_tokenizer(rows["text"], max_length=self.text_max_length, device=self.device if on_device else "cpu")}
        for name in GRAPH_MODALITIES:
            out[name] = featurize_batch(rows[name], self.device) if on_device else GraphBatch.from_data_list(rows[name])
        if on_device:
            out["sequence"], out["struct_token"] = out["sequence"].to(self.device), out["struct_token"].to(self.device)
        return out


def create_dataloader(cfg):
    """ref eval.py:139-142, in the parent process (num_workers is accepted and ignored: the collate function may launch kernels)"""
    from torch.utils.data import DataLoader
    dataset = CombinedDataset(cfg)
    dl = _sub(cfg, "dataloader")
    return DataLoader(dataset, batch_size=int(_sub(dl, "batch_size", 50)), shuffle=bool(_sub(dl, "shuffle", False)), num_workers=0, collate_fn=dataset.collate_fn)


# ---- 3. model ---------------------------------------------------------------------------------------------------------------------------------------------
def load_custom_model(cfg):
    """ref eval.py:114-137: cfg.model.config_path composed and instantiated, cfg.model.ckpt_path loaded (collect.load_module), the whole module on the GPU in
    eval mode"""
    m = _sub(cfg, "model")
    model = collect.load_module(_sub(m, "config_path"), _sub(m, "ckpt_path"))
    if torch.cuda.is_available():
        model.cuda()
    model.eval()
    return model


def encode_inputs(model, batch):
    """ref eval.py:144-156: every entry of a collated batch but `ids` through model(data, modality)"""
    model.eval()
    encoded = {}
    device = next(model.parameters()).device
    with torch.no_grad():
        for modality, data in batch.items():
            if modality != "ids":
                encoded[modality] = model(data.to(device), modality)
    return encoded


# ---- 4. the whole-dataset pass ------------------------------------------------------------------------------------------------------------------------------
def plan_tokens(strings, encode_all, max_length, max_tokens=None, max_seqs=None, pad_id=1):
    """collect.plan_sequences for any tokenizer: the distinct strings sorted by bytes, encode_all(strings, max_length) -> (flat, off) once, plan_batches over
    the token counts.  A function of the set of strings: permuting the rows permutes `inverse` only."""
    max_tokens = collect.DEFAULT_MAX_TOKENS if max_tokens is None else int(max_tokens)
    max_seqs = collect.DEFAULT_MAX_SEQS if max_seqs is None else int(max_seqs)
    uniq, (inverse,) = collect.unique_sequences(list(strings))
    flat, off = encode_all(uniq, max_length)
    return dict(uniq=uniq, inverse=inverse, flat=flat, off=off, pad_id=pad_id,
                batches=collect.plan_batches(np.diff(off), max_tokens, max_seqs, max_length=max_length))


def plan_graphs(n_nodes, max_graphs, max_nodes=None):
    """[(lo, hi)]: consecutive rows in file order; a batch is closed when it holds max_graphs graphs or when the next graph would take its node count past
    max_nodes (None: no node budget, the reference's compositions).  A graph larger than max_nodes is a batch of its own."""
    if max_graphs < 1:
        raise ValueError("plan_graphs: max_graphs must be at least 1")
    out, lo, nodes = [], 0, 0
    for i, n in enumerate(n_nodes):
        if i > lo and (i - lo == max_graphs or (max_nodes is not None and nodes + int(n) > max_nodes)):
            out.append((lo, i))
            lo, nodes = i, 0
        nodes += int(n)
    if len(n_nodes) > lo:
        out.append((lo, len(n_nodes)))
    return out


def _encode_texts_device(tokenizer, texts, max_length, device):
    """(flat, off) of BertWordPieceTokenizer.encode_all from the device kernel: the ids and lengths of the whole set are read back once, to plan on the host"""
    flats, lens = [], []
    for lo in range(0, len(texts), _TEXT_CHUNK):
        ids, n = tokenizer.encode_device(texts[lo:lo + _TEXT_CHUNK], max_length, device)
        keep = torch.arange(max_length, device=ids.device)[None, :] < n[:, None]
        flats.append(ids[keep].to(torch.int64).cpu().numpy())
        lens.append(n.to(torch.int64).cpu().numpy())
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    return np.concatenate(flats), off


def _model_device(model):
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise hip.HipKernelError("OneProt HIP path needs CUDA(ROCm) tensors; there is no CPU fallback (move the model to the device)")
    hip.lib()
    return dev


def embed_graphs(encoder, records, dev, max_graphs, max_nodes=None, timings=None):
    """fp32 [N, D] on `dev`: the records (read_records) in file order, batch by batch of plan_graphs through featurize_batch(records, dev) and the tower.
    Eval mode under no_grad, training flags put back; nothing is read back."""
    batches = plan_graphs([len(r[0]) for r in records], max_graphs, max_nodes)
    flags = [(m, m.training) for m in encoder.modules()]
    encoder.eval()
    out = None
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            for lo, hi in batches:
                if timings is not None:
                    timings.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    timings[-1][0].record()
                feats = encoder(featurize_batch(records[lo:hi], dev))
                if out is None:
                    out = torch.empty(len(records), feats.shape[1], dtype=torch.float32, device=dev)
                out[lo:hi] = feats
                if timings is not None:
                    timings[-1][1].record()
        return out
    finally:
        for m, flag in flags:
            m.training = flag


class Embeddings(dict):
    """embed_modalities' {modality: fp32 [N, D]}; ids: the N kept rows' ids"""
    ids = None


def embed_modalities(model, dataset, modalities=None, max_tokens=None, max_seqs=None, max_nodes=None, max_graphs=None, timings=None):
    """{name: fp32 [N, D] on the model's device} in row order, N the rows of the table that all three files hold; the dict's `.ids` are theirs.

    Token modalities (sequence, struct_token, text) are a whole-dataset pass: the distinct strings are tokenised once, filled into token budgets of
    max_tokens / max_seqs (collect.plan_batches), each batch one PackedTokens stream (text with pad id 0) staged from pinned memory on a copy stream while
    the previous batch runs, the results written into a resident [U, D] buffer and gathered to row order (collect.run_plan).  With dataset.device set the
    texts are tokenised by the WordPiece kernel and their ids read back once for the whole set; nothing is read back per batch.

    Graph modalities (struct_graph, pocket) keep file order on purpose: ProNet's (i -+ 1) mod N neighbours wrap over the batch, so a graph's first and last
    node depend on the batch composition, here as in the reference.  A batch is closed at max_graphs (default 50, the reference's dataloader.batch_size) or
    at max_nodes; with max_nodes=None the compositions are those of the reference's 50-row loop and the rows are bit-identical to it.

    modalities: default the dataset's five, intersected with model.network's keys.  The model runs in eval mode under no_grad and its training flags are put
    back.  timings: a dict that receives, per modality, a list of (start, end) timing events per batch."""
    dev = _model_device(model)
    if modalities is None:
        modalities = [m for m in MODALITIES if m in model.network]
    unknown = [m for m in modalities if m not in MODALITIES or m not in model.network]
    if unknown:
        raise ValueError(f"embed_modalities: {unknown} not among the dataset's modalities {MODALITIES} and the model's {list(model.network)}")
    rows = dataset.resolve(dataset.data, records=True)
    if not rows["ids"]:
        raise ValueError("embed_modalities: no row of the table is held by all three files")
    on_device = dataset.device is not None and torch.device(dataset.device).type != "cpu"
    out = Embeddings()
    out.ids = rows["ids"]
    for name in modalities:
        encoder = model.network[name]
        log = None if timings is None else timings.setdefault(name, [])
        if name in GRAPH_MODALITIES:
            out[name] = embed_graphs(encoder, rows[name], dev, 50 if max_graphs is None else int(max_graphs), max_nodes, log)
            continue
        if name == "text":
            tok = dataset.text_tokenizer
            encode = (lambda texts, n: _encode_texts_device(tok, texts, n, dev)) if on_device else tok.encode_all
            plan = plan_tokens(rows[name], encode, dataset.text_max_length, max_tokens, max_seqs, pad_id=tok.pad_id)
        else:
            tok = dataset.sequence_tokenizer if name == "sequence" else dataset.structure_tokenizer
            plan = plan_tokens(rows[name], tok.encode_all, dataset.max_sequence_length, max_tokens, max_seqs, pad_id=tok.pad_id)
        out[name] = collect.run_plan(encoder, encoder, plan, dev, log)
    return out


# ---- 5. metrics and files -----------------------------------------------------------------------------------------------------------------------------------
class RetrievalResults(dict):
    """the reference's {f"{mod1}-{mod2}": metrics}; tie_rows: {pair: (rows with at least one tie mod1 -> mod2, mod2 -> mod1)}; bound: which rank it holds"""
    tie_rows = None
    bound = "optimistic"

    @property
    def any_ties(self):
        return any(a or b for a, b in self.tie_rows.values())


def calculate_retrieval_metrics(embeddings, bound="optimistic", slab_rows=None):
    """ref eval.py:158-184 on the device: cosine similarity is L2-normalise + dot (retrieval_table(normalize=True)), ranks counted without the N x N matrix.
    embeddings: {modality: [N, D]}, device tensors or host arrays (copied to the current device).  bound "optimistic" counts
    strict > (a tie does not push the matching pair down), "pessimistic" rank + ties.  The median rank is an int, as in the reference."""
    feats = {}
    for name, x in embeddings.items():
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
        feats[name] = x if x.is_cuda else x.to("cuda")
    tie_rows = {}
    results = RetrievalResults(retrieval_table(feats, KS, normalize=True, slab_rows=slab_rows, bound=bound, tie_rows=tie_rows))
    for metrics in results.values():
        for key in metrics:
            if key.endswith("median_rank"):
                metrics[key] = int(metrics[key])
    results.tie_rows, results.bound = tie_rows, bound
    return results


def write_results_to_csv(results, output_path):
    """the reference's file, byte for byte (eval.py:185-208): padded headers, one row per direction (mod1-mod2 first), R@k as %.3f and six spaces, the median
    rank left-aligned in 11, csv's \\r\\n line ends"""
    with open(output_path, "w", newline="") as f:
        writer = csv.writer(f, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL)
        writer.writerow([f"{'Modality Pair':<24}"] + [f"{name:<11}" for name in ("R@1", "R@10", "R@100", "R@500", "MR")])
        for pair, metrics in results.items():
            first, second = pair.split("-")
            for direction, label in (("seq_to_mod", f"{first}-{second}"), ("mod_to_seq", f"{second}-{first}")):
                writer.writerow([f"{label:<25}"] + [f"{metrics[f'{direction}_R@{k}']:.3f}" + " " * 6 for k in KS] + [f"{metrics[f'{direction}_median_rank']:<11}"])


def pessimistic_path(csv_path):
    stem, ext = os.path.splitext(str(csv_path))
    return f"{stem}_pessimistic{ext}"


def evaluate(cfg, model=None, dataset=None):
    """model, dataset, embed_modalities, both tables; writes output.csv_path and, when any row ties, the pessimistic file.  Returns (results, embeddings)."""
    model = load_custom_model(cfg) if model is None else model
    if dataset is None:
        dataset = CombinedDataset(cfg)
        dataset.device = next(model.parameters()).device
    dl = _sub(cfg, "dataloader") or {}
    emb = embed_modalities(model, dataset, max_tokens=_sub(dl, "max_tokens"), max_seqs=_sub(dl, "max_seqs"), max_nodes=_sub(dl, "max_nodes"),
                           max_graphs=int(_sub(dl, "batch_size", 50)))
    for name, x in emb.items():
        logger.info(f"Final dimensions of {name} embeddings: {tuple(x.shape)}")
    results = calculate_retrieval_metrics(emb)
    out_path = _sub(_sub(cfg, "output"), "csv_path")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    write_results_to_csv(results, out_path)
    for pair, (a, b) in results.tie_rows.items():
        first, second = pair.split("-")
        logger.info(f"{first}-{second}: {a} of {len(emb.ids)} rows tie with their matching pair; {second}-{first}: {b}")
    if results.any_ties:
        write_results_to_csv(calculate_retrieval_metrics(emb, bound="pessimistic"), pessimistic_path(out_path))
        logger.info(f"Ties present: rank + ties written to {pessimistic_path(out_path)}")
    logger.info(f"Retrieval metrics calculation completed. Results written to {out_path}")
    return results, emb


def main(argv=None, default_config=None):
    """python src/eval.py [--config configs/eval.yaml] [key=value ...]"""
    import argparse
    import yaml
    from . import config as config_mod
    if default_config is None:
        default_config = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "eval.yaml")
    ap = argparse.ArgumentParser(description="one test table -> retrieval_metrics.csv for every modality pair, on the HIP towers")
    ap.add_argument("--config", default=default_config)
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    cfg = config_mod.compose(os.path.dirname(os.path.abspath(args.config)), os.path.basename(args.config), resolve=False)
    cfg.pop("hydra", None)                                      # a reference user's file carries Hydra's run-directory block
    for ov in args.overrides:
        key, _, value = ov.partition("=")
        node, parts = cfg, key.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = yaml.safe_load(value)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    results, _ = evaluate(cfg)
    return results
