"""Downstream metrics on the device: the scoring rules of the reference's downstream benchmark (ref src/utils/downstream.py:12-59 `count_f1_max`; ref
src/saprot_fit_cls.py:41-65, src/saprot_fit_reg.py:30-41 and src/saprot_fit_mlp.py:298-330, which score with sklearn's roc_auc_score / accuracy_score /
f1_score(micro) / mean_squared_error / r2_score and scipy's spearmanr).

Everything except accuracy and MSE / R2 is an order statistic.  The kernels (csrc/metrics.hip) are a stable radix sort, midranks, ordered scans and an fp64
moments reduction; every metric here is a few launches of those and ONE readback of a handful of doubles at the end.  Two runs give the same bits.

Tie rules:
  * `argsort`: equal keys keep ascending index in both directions; -0.0 and +0.0 are equal keys.  NaN is outside the contract (as in retrieval.py).
  * `count_f1_max`: descending score, ascending flat index, F read after every element.  On tie-free input this IS the reference's function (whose two
    unstable argsorts leave the order of equal scores undefined).
  * `binary_auc` / `spearman_rho`: average ranks (midranks), as roc_auc_score and spearmanr.

Inputs: device tensors are used in place.  CPU tensors, numpy arrays and lists -- what the reference's call sites pass -- are accepted and copied to the
current device: a deliberate difference from retrieval.py, which refuses host tensors, because these functions stand in for sklearn / scipy calls on host
arrays.  Scores are computed on their fp32 values.  A missing library raises hip.HipLibraryMissing; there is no host fallback.  Shape mismatches, empty
inputs, more than two dimensions, more than 2^31 - 1 elements and (for host data) targets outside {0, 1} raise ValueError before the device is touched."""
import math
import os

import numpy as np
import torch

from . import hip

MAX_ELEMENTS = 2 ** 31 - 1
MAX_RANKED = 2 ** 30 - 1      # twice a rank is an int32 up to here; AUC and Spearman take no more
BINARY_TASKS = ("MetalIonBinding", "DeepLoc2", "HumanPPI")                  # ref saprot_fit_cls.py:41
MULTILABEL_TASKS = ("EC", "GO-BP", "GO-MF", "GO-CC")                        # ref saprot_fit_cls.py:49
REGRESSION_TASKS = ("ThermoStability",)                                      # ref saprot_fit_cls.py:53
MULTICLASS_TASKS = ("DeepLoc10", "TopEnzyme")                                # the reference's `else` branch; the names are saprot_fit_mlp.py:146-149


def _as_tensor(x, what):
    """the input as a torch tensor, still wherever it lives; shape rules that hold for every function"""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        try:
            t = torch.as_tensor(np.asarray(x))
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: a tensor, numpy array or nested list of numbers is expected ({e})") from None
    if t.dim() > 2:
        raise ValueError(f"{what}: {t.dim()} dimensions; at most 2 are taken")
    if t.numel() == 0:
        raise ValueError(f"{what}: empty input")
    if t.numel() > MAX_ELEMENTS:
        raise ValueError(f"{what}: {t.numel()} elements, more than 2^31 - 1")
    if t.dtype.is_complex:
        raise ValueError(f"{what}: complex input")
    return t


def _flat(x, what):
    t = _as_tensor(x, what)
    if t.dim() == 2 and 1 not in t.shape:
        raise ValueError(f"{what}: shape {tuple(t.shape)}; a vector (or [n, 1] / [1, n]) is expected")
    return t.reshape(-1)


def _check_binary(t, what):
    """host data only: a device tensor is not read back for this"""
    if not t.is_cuda and not bool(((t == 0) | (t == 1)).all()):
        raise ValueError(f"{what}: values outside {{0, 1}}")


def _device(t, dtype):
    hip.lib()                                                   # HipLibraryMissing before any device work
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    return t.to(dtype).contiguous()


def _labels_dtype(*ts):
    return torch.float32 if any(t.dtype.is_floating_point for t in ts) else torch.int32


def _ranked(x, what):
    t = _flat(x, what)
    if t.numel() > MAX_RANKED:
        raise ValueError(f"{what}: {t.numel()} elements, 2^30 or more")
    return t


def argsort(x, descending=False):
    """int32 device tensor [n]: the stable argsort of a vector by its fp32 values (replaces `x.argsort(descending=...)`, ref downstream.py:27,35)"""
    t = _flat(x, "argsort: x")
    return hip.sort_f32(_device(t, torch.float32), descending=descending)[0]


def midranks(x):
    """float64 device tensor [n]: the average 1-based rank of every element (scipy.stats.rankdata(x, "average")), from the kernel's exact integer 2 * rank"""
    t = _ranked(x, "midranks: x")
    return hip.midranks_f32(_device(t, torch.float32)).to(torch.float64) * 0.5


def count_f1_max(pred, target):
    """F1 score with the optimal threshold (ref downstream.py:12-59), as a Python float; prints nothing.

    pred [B, N] scores, target [B, N] in {0, 1}.  All B * N scores are walked in descending order, equal scores in ascending flat index; after every element
    the mean precision of the rows seen so far and the mean recall of all rows give an F1, and the largest is returned."""
    return float(f1_max_and_threshold(pred, target)[0])


def f1_max_and_threshold(pred, target):
    """(F1-max, the score at which it is first reached) as Python floats"""
    p, t = _as_tensor(pred, "count_f1_max: pred"), _as_tensor(target, "count_f1_max: target")
    if p.dim() != 2:
        raise ValueError(f"count_f1_max: pred has shape {tuple(p.shape)}; [B, N] is expected")
    if p.shape != t.shape:
        raise ValueError(f"count_f1_max: pred {tuple(p.shape)} and target {tuple(t.shape)} must have the same shape")
    _check_binary(t, "count_f1_max: target")
    p = _device(p, torch.float32)
    t = _device(t, torch.float32 if t.dtype.is_floating_point else torch.int32).to(p.device)
    out = hip.f1max(p, t).cpu()
    return float(out[0]), float(out[1])


def binary_auc(y_true, y_score):
    """Area under the ROC curve by the midrank Mann-Whitney statistic, (sum of the positives' midranks - P (P + 1) / 2) / (P * Nneg): what
    sklearn.metrics.roc_auc_score returns, ties included.  ValueError when only one class is present, as sklearn raises."""
    yt, ys = _ranked(y_true, "binary_auc: y_true"), _ranked(y_score, "binary_auc: y_score")
    if yt.numel() != ys.numel():
        raise ValueError(f"binary_auc: {yt.numel()} labels and {ys.numel()} scores")
    _check_binary(yt, "binary_auc: y_true")
    one_class = "Only one class present in y_true. ROC AUC score is not defined in that case."
    if not yt.is_cuda and bool((yt == yt[0]).all()):
        raise ValueError(one_class)
    rank2 = hip.midranks_f32(_device(ys, torch.float32))
    m = hip.moments(rank2, _device(yt != 0, torch.int32).to(rank2.device)).cpu().tolist()
    n, pos, twice_rank_sum = m[0], m[2], m[5]
    if pos == 0 or pos == n:
        raise ValueError(one_class)
    return (0.5 * twice_rank_sum - pos * (pos + 1) / 2) / (pos * (n - pos))


def spearman_rho(a, b):
    """Spearman's rank correlation: Pearson's r of the midranks, centred with their known mean (n + 1) / 2 (scipy.stats.spearmanr(a, b)[0]).  NaN when
    either input is constant."""
    ta, tb = _ranked(a, "spearman_rho: a"), _ranked(b, "spearman_rho: b")
    if ta.numel() != tb.numel():
        raise ValueError(f"spearman_rho: {ta.numel()} and {tb.numel()} elements")
    ra = hip.midranks_f32(_device(ta, torch.float32))
    rb = hip.midranks_f32(_device(tb, torch.float32).to(ra.device))
    n = ta.numel()
    # twice the ranks have mean n + 1 exactly; the kernel subtracts the nearest fp32 and the remainder is undone here
    shift = float(np.float32(n + 1))
    delta = float(n + 1) - shift
    m = hip.moments(ra, rb, shift_a=shift, shift_b=shift).cpu().tolist()
    va, vb, cov = m[3] - n * delta * delta, m[4] - n * delta * delta, m[5] - n * delta * delta
    if va <= 0.0 or vb <= 0.0:
        return float("nan")
    return cov / math.sqrt(va * vb)


def _pair(y_true, y_pred, what):
    yt, yp = _flat(y_true, f"{what}: y_true"), _flat(y_pred, f"{what}: y_pred")
    if yt.numel() != yp.numel():
        raise ValueError(f"{what}: {yt.numel()} targets and {yp.numel()} predictions")
    return yt, yp


def accuracy(y_true, y_pred):
    """the fraction of equal labels (sklearn's accuracy_score; on single-label predictions also f1_score(average="micro"))"""
    yt, yp = _pair(y_true, y_pred, "accuracy")
    dt = _labels_dtype(yt, yp)
    a = _device(yt, dt)
    m = hip.moments(a, _device(yp, dt).to(a.device)).cpu().tolist()
    return m[7] / m[0]


def regression_scores(y_true, y_pred):
    """(MSE, R2) as sklearn's mean_squared_error and r2_score: R2 = 1 - sum (y - p)^2 / sum (y - mean y)^2; a constant y_true gives 1.0 for a perfect
    prediction and 0.0 otherwise, as r2_score does."""
    yt, yp = _pair(y_true, y_pred, "regression_scores")
    a = _device(yt, torch.float32)
    n, sa, _, saa, _, _, sdd, _ = hip.moments(a, _device(yp, torch.float32).to(a.device)).cpu().tolist()
    ss_tot = saa - sa * sa / n
    if ss_tot <= 0.0:
        r2 = 1.0 if sdd == 0.0 else 0.0
    else:
        r2 = 1.0 - sdd / ss_tot
    return sdd / n, r2


def evaluate_predictions(task_name, y_pred, y_true, partition):
    """The result dict of ref saprot_fit_cls.py:41-65 / saprot_fit_mlp.py:298-330 for one partition, with the reference's keys."""
    out = {}
    if task_name in BINARY_TASKS:
        yp = _flat(y_pred, "evaluate_predictions: y_pred")
        acc = accuracy(y_true, (yp > 0.5).to(torch.int32))
        out[f"{partition}_accuracy"] = acc
        out[f"{partition}_f1_micro"] = acc                      # micro-F1 of single-label predictions is their accuracy
        out[f"{partition}_auc"] = binary_auc(y_true, yp)
    elif task_name in MULTILABEL_TASKS:
        out[f"{partition}_f1_max"] = count_f1_max(y_pred, y_true)
    elif task_name in REGRESSION_TASKS:
        mse, r2 = regression_scores(y_true, y_pred)
        out[f"{partition}_mse"] = mse
        out[f"{partition}_r2"] = r2
        out[f"{partition}_spearman_rho"] = spearman_rho(y_true, y_pred)
    elif task_name in MULTICLASS_TASKS:
        acc = accuracy(y_true, y_pred)
        out[f"{partition}_accuracy"] = acc
        out[f"{partition}_f1_micro"] = acc
    else:
        known = BINARY_TASKS + MULTILABEL_TASKS + REGRESSION_TASKS + MULTICLASS_TASKS
        raise ValueError(f"evaluate_predictions: unknown task {task_name!r}; the reference's tasks are {', '.join(known)}")
    return out


def load_data(cfg):
    """ref src/utils/downstream.py:121-147: for every partition of cfg["evaluate_on"] the file
    <emb_dir>/<model_type>/<task_name>/<partition>/<task_name>_<partition>_embeddings_labels.pt with `embeddings` and `labels_fitness`, as host numpy arrays under
    "<partition>_emb" / "<partition>_target"; a finite cfg["threshold"] binarises the EMBEDDINGS (> threshold -> 1.0, else 0.0), as the reference does.  A
    missing file raises FileNotFoundError (the reference goes on with the previous partition's arrays, or a NameError for the first)."""
    out = {}
    task, model_type = cfg["task_name"], cfg["model_type"]
    for partition in cfg["evaluate_on"]:
        path = os.path.join(cfg["emb_dir"], f"{model_type}/{task}/{partition}/{task}_{partition}_embeddings_labels.pt")
        if not os.path.exists(path):
            raise FileNotFoundError(f"load_data: {path} not found")
        both = torch.load(path, map_location="cpu", weights_only=True)
        emb, target = both["embeddings"], both["labels_fitness"]
        if not math.isinf(float(cfg["threshold"])):
            emb = torch.where(emb > float(cfg["threshold"]), torch.tensor(1.0), torch.tensor(0.0))
        out[f"{partition}_emb"] = emb.cpu().numpy()
        out[f"{partition}_target"] = target.cpu().numpy()
    return out


def save_results_to_csv(results, cfg):
    """ref src/utils/downstream.py:62-118 on Python's csv module: one row appended to <results_dir>/downstream_results/<task>_<downstream model>_results.csv
    (the header only when the file is new).  Columns: model_type, every `test_*` result, then the other results, downstream_model, task_name, threshold and
    one `param_<key>` per key of cfg.downstream_model but `_target_`; every cell padded to 20 characters, numbers as %.3f.  Returns the file's path."""
    import csv
    dm = cfg["downstream_model"]
    row = dict(results)
    row.update(model_type=cfg["model_type"], downstream_model=dm["name"], task_name=cfg["task_name"], threshold=cfg["threshold"])
    for param, value in dm.items():
        if param != "_target_":
            row[f"param_{param}"] = value
    first = ["model_type"] + [c for c in row if c.startswith("test_")]
    columns = first + [c for c in row if c not in first]
    width = 20

    def cell(value):
        return (f"{value:.3f}" if isinstance(value, (int, float, np.number)) else str(value)).ljust(width)

    out_dir = os.path.join(str(cfg["results_dir"]), "downstream_results")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{cfg['task_name']}_{dm['name']}_results.csv")
    new = not os.path.exists(path)
    with open(path, "w" if new else "a", newline="") as f:
        writer = csv.writer(f)
        if new:
            writer.writerow([c.ljust(width) for c in columns])
        writer.writerow([cell(row[c]) for c in columns])
    print(f"Results appended to {path}")
    print("\nResults:")
    for c in columns:
        print(f"{c.ljust(30)}: {cell(row[c])}")
    return path
