"""fp64 numpy restatements of the downstream scoring rules (oneprot_amd/downstream.py states them; csrc/metrics.hip computes them).  Independent of the
kernels: a sequential walk for F1-max and a vectorised twin for larger inputs, midranks, AUC, Spearman, accuracy, MSE / R2; and the decoder of the inputs
stored in tests/golden/downstream_metrics.json.  Scores are taken at their fp32 values, as the device path takes them."""
import numpy as np


def descending_order(flat):
    """flat indices by descending fp32 score, equal scores in ascending index"""
    return np.argsort(-np.asarray(flat, np.float32).astype(np.float64), kind="stable")


def f1_max_walk(pred, target):
    """(F1-max, the score at which it is first reached): the rule, element by element"""
    pred = np.asarray(pred, np.float32)
    tgt = (np.asarray(target).reshape(pred.shape) != 0).astype(np.float64)
    B, N = pred.shape
    flat, t = pred.reshape(-1), tgt.reshape(-1)
    T = tgt.sum(1)
    cnt, tp, prec, rec = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    sum_p = sum_r = 0.0
    started, best, at = 0, -1.0, 0.0
    for k in descending_order(flat):
        i = k // N
        if cnt[i] == 0:
            started += 1
        cnt[i] += 1
        tp[i] += t[k]
        p, r = tp[i] / cnt[i], tp[i] / (T[i] + 1e-10)
        sum_p += p - prec[i]
        sum_r += r - rec[i]
        prec[i], rec[i] = p, r
        P, R = sum_p / started, sum_r / B
        f = 2 * P * R / (P + R + 1e-10)
        if f > best:
            best, at = f, float(flat[k])
    return float(best), at


def f1_max_vectorised(pred, target):
    """the same rule with sorts and cumulative sums (numpy's cumsum is a sequential fp64 chain): the first maximum of f1_curve"""
    f, scores = f1_curve(pred, target)
    k = int(np.argmax(f))
    return float(f[k]), float(scores[k])


def f1_curve(pred, target):
    """(F_k for every k, the fp32 score of element k) in the walk's order"""
    pred = np.asarray(pred, np.float32)
    tgt = (np.asarray(target).reshape(pred.shape) != 0).astype(np.float64)
    B, N = pred.shape
    order = descending_order(pred.reshape(-1))
    by_row = np.argsort(order // N, kind="stable")
    tp = np.cumsum(tgt.reshape(-1)[order[by_row]].reshape(B, N), 1)
    prec, rec = tp / np.arange(1, N + 1), tp / (tp[:, -1:] + 1e-10)
    inc = np.empty((3, B * N))
    start = np.zeros((B, N))
    start[:, 0] = 1
    inc[0, by_row], inc[1, by_row], inc[2, by_row] = np.diff(prec, axis=1, prepend=0.0).reshape(-1), np.diff(rec, axis=1, prepend=0.0).reshape(-1), start.reshape(-1)
    P, Rc = np.cumsum(inc[0]) / np.cumsum(inc[2]), np.cumsum(inc[1]) / B
    return 2 * P * Rc / (P + Rc + 1e-10), pred.reshape(-1)[order]


def tie_free(pred):
    flat = np.asarray(pred, np.float32).reshape(-1) + np.float32(0)
    return len(np.unique(flat)) == flat.size


def midranks(x):
    """average 1-based ranks of the fp32 values (-0 and +0 equal)"""
    x = np.asarray(x, np.float32).reshape(-1) + np.float32(0)
    _, inv, counts = np.unique(x, return_inverse=True, return_counts=True)
    first = np.cumsum(counts) - counts
    return (first + (counts + 1) / 2.0)[inv.reshape(-1)]


def binary_auc(y_true, y_score):
    y = np.asarray(y_true).reshape(-1) != 0
    r = midranks(y_score)
    pos, n = float(y.sum()), float(y.size)
    return (r[y].sum() - pos * (pos + 1) / 2) / (pos * (n - pos))


def spearman_rho(a, b):
    ra, rb = midranks(a), midranks(b)
    mean = (ra.size + 1) / 2.0
    ra, rb = ra - mean, rb - mean
    va, vb = (ra * ra).sum(), (rb * rb).sum()
    if va == 0 or vb == 0:
        return float("nan")
    return float((ra * rb).sum() / np.sqrt(va * vb))


def accuracy(y_true, y_pred):
    return float(np.mean(np.asarray(y_true).reshape(-1) == np.asarray(y_pred).reshape(-1)))


def regression_scores(y_true, y_pred):
    y, p = np.asarray(y_true, np.float32).astype(np.float64).reshape(-1), np.asarray(y_pred, np.float32).astype(np.float64).reshape(-1)
    ss_res, ss_tot = ((y - p) ** 2).sum(), ((y - y.mean()) ** 2).sum()
    return float(ss_res / y.size), float(1 - ss_res / ss_tot)


# ---- the fixture's stored inputs
def f1_inputs(case):
    """(pred fp32 [B, N], target int32 [B, N]) of an F1 case: the scores are stored as their ranks, pred = (rank + 0.5) / (B * N), distinct in fp32"""
    B, N = case["shape"]
    pred = ((np.asarray(case["rank"], np.float64) + 0.5) / (B * N)).astype(np.float32).reshape(B, N)
    target = np.array([[int(c) for c in row] for row in case["target"]], np.int32).reshape(B, N)
    return pred, target


def levels(values, scale):
    """tied scores are stored as small integers; value = integer * scale, exact in fp32 for the scales the generator uses"""
    return (np.asarray(values, np.float64) * scale).astype(np.float32)
