"""Independent restatement of the gradient-boosted tree rule (Chen & Guestrin 2016, the `hist` method on fixed-point histograms): numpy,
int64 histograms, fp64 gains, plain loops.  A helper module like tests/probe_ref.py, not a test; it never calls a kernel and is written from the rule, not
from csrc/gbt.hip.  It draws nothing: the row and feature masks of a sampled fit are handed in (tests rebuild them with tests/philox_ref.py).

`fit` also reports the margin of its own decisions: the smallest relative gap, over all nodes that split, between the best gain and the best gain of a
candidate with a DIFFERENT (GL_int, HL_int).  Candidates with equal integer pairs are exact ties (empty bins make them the normal case below the root) and the
lowest-feature / lowest-cut order settles them; a small gap between different pairs is where another rounding could choose another tree."""
import math

import numpy as np

FRAC = 20
LOGISTIC, SQUARED, SOFTMAX = "binary:logistic", "reg:squarederror", "multi:softmax"
f32 = np.float32


def make_cuts(X, B):
    """(list of F ascending fp32 cut arrays, bins uint8 [N, F]): candidates v[floor(k N / B)], k = 1 .. B-1, of every ascending column, -0.0 read as +0.0;
    the distinct ones are the cuts; bin(x) = number of cuts <= x"""
    X = np.asarray(X, dtype=f32)
    N, F = X.shape
    cuts, bins = [], np.zeros((N, F), dtype=np.uint8)
    for f in range(F):
        v = np.sort(X[:, f] + f32(0.0))
        cand = [v[(k * N) // B] + f32(0.0) for k in range(1, B)]
        c = []
        for x in cand:
            if not c or x != c[-1]:
                c.append(x)
        c = np.asarray(c, dtype=f32)
        cuts.append(c)
        bins[:, f] = np.searchsorted(c, X[:, f], side="right")
    return cuts, bins


def initial_margin(objective, base_score):
    b = f32(base_score)
    if objective == LOGISTIC:
        return f32(math.log(float(b) / (1.0 - float(b))))
    return b


def gradients(m, y, objective):
    """fp32 (g, h) [N, K] from the fp32 margin [N, K]; y [N, K] floats, or int labels [N] for softmax"""
    m = np.asarray(m, dtype=f32)
    if objective == SQUARED:
        return m - np.asarray(y, dtype=f32), np.ones_like(m)
    if objective == LOGISTIC:
        with np.errstate(over="ignore"):                               # exp(-m) = inf gives p = 0, as on the device
            p = f32(1.0) / (f32(1.0) + np.exp(-m, dtype=f32))
        return p - np.asarray(y, dtype=f32), p * (f32(1.0) - p)
    mx = m.max(axis=1, keepdims=True)
    ex = np.exp(m - mx, dtype=f32)
    s = np.zeros((m.shape[0], 1), dtype=f32)
    for k in range(m.shape[1]):                                    # the row sum in ascending k, fp32
        s[:, 0] = s[:, 0] + ex[:, k]
    p = ex / s
    onehot = (np.arange(m.shape[1])[None, :] == np.asarray(y).reshape(-1, 1)).astype(f32)
    return p - onehot, f32(2.0) * p * (f32(1.0) - p)


def exponent(g, kept, objective):
    """e of the fixed point of g: 0 unless reg:squarederror, then the smallest integer with max |g| < 2^e over the kept rows (0 if that max is 0, at least -100)"""
    if objective != SQUARED:
        return 0
    mx = float(np.abs(g[kept]).max()) if kept.any() else 0.0
    if not mx > 0.0:
        return 0
    return max(math.frexp(mx)[1], -100)


def quantise(g, h, kept, e):
    """int64 (gq, hq): rint(x 2^(FRAC - e)) in fp32 for g, rint(h 2^FRAC) for h; 0 on dropped rows"""
    gq = np.rint(np.ldexp(g.astype(f32), FRAC - e).astype(f32)).astype(np.int64)
    hq = np.rint(np.ldexp(h.astype(f32), FRAC).astype(f32)).astype(np.int64)
    gq[~kept] = 0
    hq[~kept] = 0
    return gq, hq


def histogram(bins, gq, hq, rows, B):
    """int64 [F, B, 2] over the given rows"""
    F = bins.shape[1]
    H = np.zeros((F, B, 2), dtype=np.int64)
    for f in range(F):
        np.add.at(H[f, :, 0], bins[rows, f], gq[rows])
        np.add.at(H[f, :, 1], bins[rows, f], hq[rows])
    return H


def _thr(G, alpha):
    a = abs(G) - alpha
    return (a if G >= 0 else -a) if a > 0 else 0.0


def score(G, H, alpha, lam):
    t = _thr(G, alpha)
    return t * t / (H + lam)


def weight(G, H, alpha, lam):
    d = H + lam
    return -_thr(G, alpha) / d if d > 0 else 0.0


def best_split(H, ncuts, feat_keep, e, *, min_child_weight=1.0, gamma=0.0, reg_alpha=0.0, reg_lambda=1.0):
    """the decision of one node from its int64 histogram [F, B, 2]: dict(valid, split, gain, f, j, GL, HL, G, H, gap).  Parameters are taken as fp32 values used
    in fp64.  gap: (best gain - best gain among candidates with another (GL, HL)) / |best gain| (inf when there is no such candidate)."""
    mcw, gamma, alpha, lam = (float(f32(v)) for v in (min_child_weight, gamma, reg_alpha, reg_lambda))
    sg, sh = math.ldexp(1.0, e - FRAC), math.ldexp(1.0, -FRAC)
    best = None
    cands = []
    Gt = Ht = 0
    for f in range(H.shape[0]):
        if not feat_keep[f]:
            continue
        G, Hs = int(H[f, :ncuts[f] + 1, 0].sum()), int(H[f, :ncuts[f] + 1, 1].sum())
        Gt, Ht = G, Hs
        if Hs <= 0:
            continue
        sN = score(G * sg, Hs * sh, alpha, lam)
        GL = HL = 0
        for j in range(ncuts[f]):
            GL += int(H[f, j, 0])
            HL += int(H[f, j, 1])
            HR = Hs - HL
            if HL <= 0 or HR <= 0 or not HL * sh >= mcw or not HR * sh >= mcw:
                continue
            gain = (score(GL * sg, HL * sh, alpha, lam) + score((G - GL) * sg, HR * sh, alpha, lam)) - sN
            cands.append((gain, GL, HL))
            if best is None or gain > best[0]:                     # ascending (f, j): the first of equal gains stays
                best = (gain, f, j, GL, HL)
    out = dict(valid=best is not None, split=False, gain=-math.inf, f=-1, j=-1, GL=0, HL=0, G=Gt, H=Ht, gap=math.inf)
    if best is None:
        return out
    gain, f, j, GL, HL = best
    others = [c[0] for c in cands if (c[1], c[2]) != (GL, HL)]
    gap = (gain - max(others)) / abs(gain) if others and gain != 0 else math.inf
    out.update(split=gain > max(gamma, 0.0), gain=gain, f=f, j=j, GL=GL, HL=HL, gap=gap)
    return out


def n_keep_features(F, rate):
    return F if rate >= 1.0 else max(1, int(math.floor(F * float(rate))))


def fit(X, y, objective, *, n_estimators, max_depth, learning_rate=0.3, max_bin=256, base_score=0.5, min_child_weight=1.0, gamma=0.0, reg_alpha=0.0,
        reg_lambda=1.0, row_masks=None, feat_masks=None):
    """dict(cuts, trees, margin, gap, margins): trees[t][k] = dict(feat, bin, thr, leaf) arrays over the 2^(max_depth+1) - 1 heap nodes; margin fp32 [N, K] after
    the last round; margins the list of it after every round; gap as the module docstring says.  row_masks / feat_masks: per round bool [N] / [F], or None."""
    X = np.asarray(X, dtype=f32)
    N, F = X.shape
    y = np.asarray(y)
    if objective == SOFTMAX:
        K = int(y.max()) + 1 if np.ndim(y) == 1 else None
    else:
        y = y.astype(f32).reshape(N, -1)
        K = y.shape[1]
    cuts, bins = make_cuts(X, max_bin)
    ncuts = [len(c) for c in cuts]
    NN = 2 ** (max_depth + 1) - 1
    lr = float(f32(learning_rate))
    alpha, lam = float(f32(reg_alpha)), float(f32(reg_lambda))
    sh = math.ldexp(1.0, -FRAC)
    m = np.full((N, K), initial_margin(objective, base_score), dtype=f32)
    trees, gap, margins = [], math.inf, []
    for t in range(n_estimators):
        kept = np.ones(N, dtype=bool) if row_masks is None else np.asarray(row_masks[t], dtype=bool)
        fk = np.ones(F, dtype=bool) if feat_masks is None else np.asarray(feat_masks[t], dtype=bool)
        g, h = gradients(m, y, objective)
        round_trees = []
        for k in range(K):
            e = exponent(g[:, k], kept, objective)
            sg = math.ldexp(1.0, e - FRAC)
            gq, hq = quantise(g[:, k], h[:, k], kept, e)
            feat, tbin = np.full(NN, -1, dtype=np.int32), np.zeros(NN, dtype=np.int32)
            thr, leaf = np.zeros(NN, dtype=f32), np.zeros(NN, dtype=f32)
            pos = np.zeros(N, dtype=np.int64)
            for level in range(max_depth):
                for nid in range(2 ** level - 1, 2 ** (level + 1) - 1):
                    rows = np.nonzero(pos == nid)[0]
                    Hn = histogram(bins, gq, hq, rows, max_bin)
                    d = best_split(Hn, ncuts, fk, e, min_child_weight=min_child_weight, gamma=gamma, reg_alpha=reg_alpha, reg_lambda=reg_lambda)
                    leaf[nid] = f32(lr * weight(d["G"] * sg, d["H"] * sh, alpha, lam))
                    if d["split"]:
                        gap = min(gap, d["gap"])
                        feat[nid], tbin[nid], thr[nid] = d["f"], d["j"], cuts[d["f"]][d["j"]]
                        leaf[2 * nid + 1] = f32(lr * weight(d["GL"] * sg, d["HL"] * sh, alpha, lam))
                        leaf[2 * nid + 2] = f32(lr * weight((d["G"] - d["GL"]) * sg, (d["H"] - d["HL"]) * sh, alpha, lam))
                        right = bins[rows, d["f"]] > d["j"]
                        pos[rows] = 2 * nid + 1 + right
            m[:, k] = m[:, k] + leaf[pos]
            round_trees.append(dict(feat=feat, bin=tbin, thr=thr, leaf=leaf, pos=pos.copy(), expo=e))
        trees.append(round_trees)
        margins.append(m.copy())
    return dict(cuts=cuts, ncuts=ncuts, bins=bins, trees=trees, margin=m, gap=gap, margins=margins, K=K)


def predict_margin(model, X, objective, base_score=0.5):
    """the ensemble walk on raw rows: x < threshold goes left; one fp32 chain per (row, output) in round order"""
    X = np.asarray(X, dtype=f32)
    N, K = X.shape[0], model["K"]
    m = np.full((N, K), initial_margin(objective, base_score), dtype=f32)
    for round_trees in model["trees"]:
        for k, tr in enumerate(round_trees):
            for i in range(N):
                p = 0
                while tr["feat"][p] >= 0:
                    p = 2 * p + 1 + (0 if X[i, tr["feat"][p]] < tr["thr"][p] else 1)
                m[i, k] = m[i, k] + tr["leaf"][p]
    return m


# ---- the sampling rule, from uniforms handed in (tests/philox_ref.py supplies the 16-bit slices)
def row_mask_from_slices(slices, rate):
    """kept iff slice / 65536 < rate, compared in fp32 as slice < rate * 65536; rate >= 1 keeps every row"""
    if rate >= 1.0:
        return np.ones(len(slices), dtype=bool)
    return np.asarray(slices, dtype=f32) < f32(rate) * f32(65536.0)


def feat_mask_from_slices(slices, rate):
    """the max(1, floor(F rate)) features with the smallest uniforms, equal uniforms to the lower index"""
    F = len(slices)
    n = n_keep_features(F, rate)
    order = np.argsort(np.asarray(slices, dtype=np.int64), kind="stable")
    mask = np.zeros(F, dtype=bool)
    mask[order[:n]] = True
    return mask
