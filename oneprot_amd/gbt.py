"""Gradient-boosted tree probes on the device (ref src/saprot_fit_cls.py, src/saprot_fit_reg.py: xgboost.XGBClassifier / XGBRegressor with tree_method
gpu_hist): fit, predict and score embeddings with no xgboost, Hydra or sklearn.

`XGBClassifier` / `XGBRegressor` carry the constructor keywords the reference's configs and sweeps use and run on csrc/gbt.hip: quantile cuts and uint8 bins once
per fit, then per round one gradient launch and, per level, histogram -> split search -> row partition; the trees are written straight into the ensemble's
arrays.  `fit` reads back once (the finiteness check of X) before its final state; all max_depth levels always launch and a node that does not split has empty
children.  Histograms of K outputs are built in chunks of outputs that fit ONEPROT_GBT_HIST_BYTES (default 1 GiB); the chunking is a pure function of (K, F,
max_bin, max_depth, budget) and cannot change a bit of the result, because every output is built by its own work-groups and every sum is an integer sum.

Depth: XGBClassifier builds max_depth 1 .. 6, XGBRegressor (one output) 1 .. 9, as the reference's regression sweep asks (3, 5, 9).  Levels 0 .. 5 keep every
node of a level in one LDS tile; levels 6 .. 8 run through oneprot_amd/gbt_deep.py: the rows in node order once per level, then histogram -> split search per
group of nodes (plan_node_groups: the largest power of two of nodes that fits the same budget), then one partition launch for the level.  The grouping is a
pure function of (F, max_bin, level, budget) and cannot change a bit either.  The rule is one rule at every depth.

NOT pinned: parity with xgboost, which is not installed here.  The rule is the published one (Chen & Guestrin 2016, the `hist` method,
fixed-point histograms as gpu_hist keeps them), stated exactly in DESIGN.md section 7 and restated independently in tests/gbt_ref.py; every random draw comes
from this library's own Philox streams.  Bit-identical between runs: gradients are integers before they are summed."""
import itertools
import math
import os

import numpy as np
import torch

from . import downstream, gbt_deep, hip, rng

RNG_DOMAIN_GBT = rng.DOMAINS["gbt"]
FRAC = 20                      # fraction bits of the fixed-point gradients (csrc/gbt.hip GBT_FRAC)
MAX_DEPTH = 9                  # the largest depth this module builds (XGBRegressor; every class has its own cap, `_max_depth`)
SHALLOW_DEPTH = 6              # up to here a level's nodes share one LDS tile (levels 0 .. 5); deeper levels run through gbt_deep
OBJECTIVES = {"binary:logistic": 0, "reg:squarederror": 1, "multi:softmax": 2}
_KNOWN = ("n_estimators", "max_depth", "learning_rate", "objective", "booster", "tree_method", "n_jobs", "min_child_weight", "gamma", "subsample",
          "colsample_bytree", "reg_alpha", "reg_lambda", "eval_metric", "base_score", "max_bin", "random_state")


def hist_bytes_budget():
    return int(os.environ.get("ONEPROT_GBT_HIST_BYTES", str(1 << 30)))


def plan_chunks(K, F, max_bin, max_depth, budget=None):
    """[(k0, k1), ...]: consecutive chunks of outputs whose deepest-level histograms fit `budget` bytes together.  A pure function of its arguments; a budget
    that does not admit one output raises ValueError."""
    budget = hist_bytes_budget() if budget is None else int(budget)
    per_output = (1 << (max_depth - 1)) * F * max_bin * 16
    kc = min(K, budget // per_output)
    tiles = -(-F // (64 >> (max_depth - 1)))                                   # feature tiles of the deepest level's histogram launch: tiles x outputs stays below 2^22 work-groups
    kc = min(kc, max(1, ((1 << 22) - 1) // tiles), 65535) if kc >= 1 else kc
    if kc < 1:
        raise ValueError(f"ONEPROT_GBT_HIST_BYTES = {budget} does not hold one output's histogram ({per_output} bytes at depth {max_depth}, {F} features, {max_bin} bins)")
    return [(k0, min(K, k0 + kc)) for k0 in range(0, K, kc)]


def plan_node_groups(F, max_bin, level, budget=None):
    """[(node0, node1), ...]: the 2^level nodes of a level in consecutive groups whose histograms (F x max_bin x 16 bytes a node) fit `budget` bytes.  The group
    size is the largest power of two that is at most min(2^level, budget // bytes of a node).  A pure function of its arguments; a budget that does not hold
    one node raises ValueError."""
    budget = hist_bytes_budget() if budget is None else int(budget)
    per_node, L = F * max_bin * 16, 1 << level
    fit = min(L, budget // per_node)
    if fit < 1:
        raise ValueError(f"ONEPROT_GBT_HIST_BYTES = {budget} does not hold one node's histogram ({per_node} bytes at {F} features, {max_bin} bins)")
    g = 1 << (fit.bit_length() - 1)
    return [(n0, n0 + g) for n0 in range(0, L, g)]


def stream_of(local):
    """the Philox stream of draw number `local` of a fit: rows of round t draw from stream t, features from stream n_estimators + t"""
    return rng.stream_id(RNG_DOMAIN_GBT, None, local)


def _to_device(x, dtype, what):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    hip.lib()                                                                  # HipLibraryMissing before any device work
    return t.detach().to(torch.device("cuda", torch.cuda.current_device()), dtype).contiguous()


def build_cuts(X, max_bin):
    """(cuts fp32 [F, max_bin - 1] with +inf in unused slots, ncuts int32 [F], bins uint8 [N, F]) of a device X fp32 [N, F].  The grouping "all values ascending
    inside each feature" comes from the two stable sorts of csrc/metrics.hip: by value, then by feature id."""
    N, F = X.shape
    if N * F > downstream.MAX_ELEMENTS:
        raise ValueError(f"gbt: X has {N * F} elements, more than 2^31 - 1 (the sort's limit)")
    flat = X.t().contiguous().view(-1)                                         # element f N + i
    perm, by_value = hip.sort_f32(flat, want_keys=True)
    if F > 1:
        fid = torch.div(perm, N, rounding_mode="floor").to(torch.int32)
        _, bits = hip.sort_i32(fid, max(1, (F - 1).bit_length()), values=by_value.view(torch.int32), want_keys=False)
        grouped = bits.view(torch.float32)
    else:
        grouped = by_value
    cuts = torch.empty(F, max_bin - 1, dtype=torch.float32, device=X.device)
    ncuts = torch.empty(F, dtype=torch.int32, device=X.device)
    hip.call("oneprot_gbt_cuts", grouped, N, F, max_bin, cuts, ncuts)
    bins = torch.empty(N, F, dtype=torch.uint8, device=X.device)
    hip.call("oneprot_gbt_bin", X, cuts, ncuts, bins, N, F, max_bin)
    return cuts, ncuts, bins


class _GBT:
    """what XGBClassifier and XGBRegressor share: the keywords, the round loop, the ensemble walk and the state dict"""
    _default_objective = None
    _max_depth = SHALLOW_DEPTH

    def __init__(self, *, n_estimators=100, max_depth=6, learning_rate=0.3, objective=None, booster="gbtree", tree_method="auto", n_jobs=None, min_child_weight=1.0,
                 gamma=0.0, subsample=1.0, colsample_bytree=1.0, reg_alpha=0.0, reg_lambda=1.0, eval_metric=None, base_score=0.5, max_bin=256, random_state=0,
                 **kwargs):
        if booster is not None and booster != "gbtree":
            raise NotImplementedError(f"booster={booster!r}: only gbtree is built")
        max_depth, n_estimators, max_bin = int(max_depth), int(n_estimators), int(max_bin)
        if not 1 <= max_depth <= self._max_depth:
            raise NotImplementedError(f"max_depth={max_depth}: {type(self).__name__} builds 1 .. {self._max_depth}")
        if n_estimators < 1:
            raise ValueError("n_estimators must be at least 1")
        if not 2 <= max_bin <= 256:
            raise ValueError(f"max_bin={max_bin}: 2 .. 256 (bins are uint8)")
        objective = self._default_objective if objective is None else objective
        if objective not in OBJECTIVES:
            raise NotImplementedError(f"objective={objective!r}: one of {', '.join(OBJECTIVES)}")
        if not 0 < float(subsample) <= 1 or not 0 < float(colsample_bytree) <= 1:
            raise ValueError("subsample and colsample_bytree are rates in (0, 1]")
        if float(reg_lambda) < 0 or float(reg_alpha) < 0 or float(min_child_weight) < 0:
            raise ValueError("reg_lambda, reg_alpha and min_child_weight must not be negative")
        if not 0 < float(base_score) < 1 and objective == "binary:logistic":
            raise ValueError("base_score of binary:logistic is a probability in (0, 1)")
        self.n_estimators, self.max_depth, self.max_bin, self.objective = n_estimators, max_depth, max_bin, objective
        self.learning_rate, self.min_child_weight, self.gamma = float(learning_rate), float(min_child_weight), float(gamma)
        self.subsample, self.colsample_bytree, self.reg_alpha, self.reg_lambda = float(subsample), float(colsample_bytree), float(reg_alpha), float(reg_lambda)
        self.base_score, self.random_state = float(base_score), 0 if random_state is None else int(random_state)
        self.booster, self.tree_method, self.n_jobs, self.eval_metric = "gbtree", tree_method, n_jobs, eval_metric     # accepted and kept; nothing here depends on them
        self.kwargs = dict(kwargs)                                             # `name` and other unknown keywords, kept as xgboost keeps them
        self._state = None
        self.train_margin_ = self.train_pos_ = None

    def get_params(self):
        return {**{k: getattr(self, k) for k in _KNOWN}, **self.kwargs}

    # ---- geometry
    @property
    def tree_nodes(self):
        return (2 << self.max_depth) - 1

    def init_margin(self):
        """base_score for regression and softmax, logit(base_score) for logistic, as fp32"""
        b = float(np.float32(self.base_score))
        return float(np.float32(math.log(b / (1.0 - b)))) if self.objective == "binary:logistic" else b

    def _targets(self, y, N):
        """(target fp32 [N, K] or None, labels int32 [N] or None, K) on the device"""
        t = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
        if t.shape[0] != N:
            raise ValueError(f"fit: {N} rows and {t.shape[0]} targets")
        if self.objective == "multi:softmax":
            if t.dim() != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError(f"fit: multi:softmax takes integer class labels [rows]; got {t.dtype} {tuple(t.shape)}")
            # the number of classes: the `num_class` keyword, else the largest label + 1 as xgboost infers it (host labels cost no device readback; labels
            # that are already on the device cost one more: hand num_class over to avoid it)
            K = self.kwargs.get("num_class") or int(t.max()) + 1
            if not t.is_cuda and (int(t.min()) < 0 or int(t.max()) >= K):
                raise ValueError(f"fit: class labels outside [0, {K})")
            return None, _to_device(t, torch.int32, "y"), int(K)
        if t.dim() == 2 and self.objective == "reg:squarederror" and t.shape[1] != 1:
            raise ValueError("fit: reg:squarederror takes one target per row")
        if t.dim() > 2:
            raise ValueError(f"fit: targets of shape {tuple(t.shape)}")
        t = t.reshape(N, -1)
        return _to_device(t, torch.float32, "y"), None, int(t.shape[1])

    # ---- fit
    def fit(self, X, y):
        x = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"fit: X of shape {tuple(x.shape)}; a non-empty [rows, features] is expected")
        N, F = x.shape
        if N > (1 << 24) or F > 65535:
            raise ValueError(f"fit: X [{N}, {F}]; at most 2^24 rows and 65535 features")
        x = _to_device(x, torch.float32, "X")
        if not bool(torch.isfinite(x).all()):                                  # the one readback before the final state
            raise ValueError("fit: X holds NaN or inf")
        target, labels, K = self._targets(y, N)
        dev, D, NN, B, T = x.device, self.max_depth, self.tree_nodes, self.max_bin, self.n_estimators
        DS = min(D, SHALLOW_DEPTH)                                             # levels 0 .. DS - 1 in chunks of outputs, levels DS .. D - 1 (one output) in groups of nodes
        groups = {level: plan_node_groups(F, B, level) for level in range(DS, D)}
        if groups and K != 1:
            raise NotImplementedError(f"max_depth={D} with {K} outputs: levels beyond {SHALLOW_DEPTH - 1} are built for one output")
        # a deep fit has one output: the budget sizes its node groups, and its levels 0 .. 5 take the 32 nodes of level 5 whatever the budget says (the floor
        # of a deep fit's histogram buffer) -- plan_chunks, whose values are pinned, would refuse a budget below them
        chunks = [(0, 1)] if groups else plan_chunks(K, F, B, D)
        cuts, ncuts, bins = build_cuts(x, B)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        tree_feat = torch.full((T, K, NN), -1, dtype=torch.int32, device=dev)
        tree_bin = torch.zeros((T, K, NN), dtype=torch.int32, device=dev)
        tree_thr = torch.zeros((T, K, NN), dtype=torch.float32, device=dev)
        tree_leaf = torch.zeros((T, K, NN), dtype=torch.float32, device=dev)
        margin = torch.full((N, K), self.init_margin(), dtype=torch.float32, device=dev)
        gq, hq, pos, expo, gmax = i32(K, N), i32(K, N), i32(K, N), i32(K), i32(1)
        row_keep = torch.empty(N, dtype=torch.uint8, device=dev)
        feat_keep = torch.empty(F, dtype=torch.uint8, device=dev)
        feat_u = i32(F)
        kc_max = max(k1 - k0 for k0, k1 in chunks)
        deep = gbt_deep.DeepLevels(N, F, B, D, groups, dev) if groups else None
        hist = torch.empty(max(kc_max * hip.query("oneprot_gbt_hist_bytes", F, B, DS - 1), deep.hist_bytes if deep else 0) // 8, dtype=torch.int64, device=dev)
        split_ws = torch.empty(hip.query("oneprot_gbt_split_workspace", F, DS - 1, kc_max), dtype=torch.uint8, device=dev)
        n_keep = F if self.colsample_bytree >= 1.0 else max(1, int(math.floor(F * self.colsample_bytree)))
        obj, seed = OBJECTIVES[self.objective], self.random_state & 0xFFFFFFFFFFFFFFFF
        for t in range(T):
            hip.call("oneprot_gbt_sample", row_keep, feat_keep, feat_u, N, F, self.subsample, n_keep, seed, stream_of(t), stream_of(T + t))
            hip.call("oneprot_gbt_grad", margin, target, labels, row_keep, gq, hq, expo, gmax, N, K, obj)
            pos.zero_()
            for k0, k1 in chunks:
                kc = k1 - k0
                tf, tb, tt, tl = tree_feat[t, k0:k1], tree_bin[t, k0:k1], tree_thr[t, k0:k1], tree_leaf[t, k0:k1]
                for level in range(DS):
                    hip.call("oneprot_gbt_hist", bins, gq[k0:k1], hq[k0:k1], pos[k0:k1], hist, N, F, B, level, kc)
                    hip.call("oneprot_gbt_split", hist, cuts, ncuts, feat_keep, expo[k0:k1], tf, tb, tt, tl, None, split_ws, split_ws.numel(), F, B, level, kc, NN, self.min_child_weight,
                             self.gamma, self.reg_alpha, self.reg_lambda, self.learning_rate)
                    hip.call("oneprot_gbt_partition", bins, tf, tb, pos[k0:k1], N, F, level, kc, NN)
                for level in range(DS, D):
                    deep.run(level, hist, bins, gq, hq, pos, cuts, ncuts, feat_keep, expo, tf, tb, tt, tl, NN, self.min_child_weight, self.gamma, self.reg_alpha,
                             self.reg_lambda, self.learning_rate)
                hip.call("oneprot_gbt_update", margin, pos[k0:k1], tl, N, K, k0, kc, NN)
        self._state = dict(cuts=cuts, ncuts=ncuts, tree_feat=tree_feat, tree_bin=tree_bin, tree_thr=tree_thr, tree_leaf=tree_leaf)
        self.n_outputs_, self.n_features_in_ = K, F
        self.train_margin_ = margin                                            # the margin fit ended with: predict_margin of the training rows gives the same bits
        self.train_pos_ = pos                                                  # int32 [K, N]: the heap node every row ended in, in the last round
        return self

    # ---- predict
    def predict_margin(self, X):
        """fp32 device tensor [N, K]: the initial margin plus the leaves in round order"""
        if self._state is None:
            raise RuntimeError("predict before fit (or load_state_dict)")
        x = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
        if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"predict: X of shape {tuple(x.shape)}; a non-empty [rows, {self.n_features_in_}] is expected")
        x = _to_device(x, torch.float32, "X")
        s = self._state
        out = torch.empty(x.shape[0], self.n_outputs_, dtype=torch.float32, device=x.device)
        hip.call("oneprot_gbt_predict", x, s["tree_feat"], s["tree_thr"], s["tree_leaf"], out, x.shape[0], x.shape[1], self.n_outputs_, s["tree_feat"].shape[0],
                 self.tree_nodes, self.init_margin())
        return out

    def state_dict(self):
        """plain tensors: the cuts, the per-tree feature / cut / value / leaf arrays, the objective id and K"""
        if self._state is None:
            raise RuntimeError("state_dict before fit")
        return {**self._state, "objective": torch.tensor(OBJECTIVES[self.objective]), "n_outputs": torch.tensor(self.n_outputs_),
                "base_score": torch.tensor(self.base_score, dtype=torch.float64), "max_depth": torch.tensor(self.max_depth)}

    def load_state_dict(self, sd):
        names = {v: k for k, v in OBJECTIVES.items()}
        self.objective, self.n_outputs_ = names[int(sd["objective"])], int(sd["n_outputs"])
        self.base_score, self.max_depth = float(sd["base_score"]), int(sd["max_depth"])
        hip.lib()
        dev = torch.device("cuda", torch.cuda.current_device())
        self._state = {k: sd[k].to(dev).contiguous() for k in ("cuts", "ncuts", "tree_feat", "tree_bin", "tree_thr", "tree_leaf")}
        if self._state["tree_feat"].shape[2] != self.tree_nodes or self._state["tree_feat"].shape[1] != self.n_outputs_:
            raise ValueError("load_state_dict: the tree arrays do not match max_depth / n_outputs")
        self.n_features_in_, self.n_estimators = int(self._state["cuts"].shape[0]), int(self._state["tree_feat"].shape[0])
        self.max_bin = int(self._state["cuts"].shape[1]) + 1
        return self


class XGBClassifier(_GBT):
    """ref saprot_fit_cls.py:32-38.  objective binary:logistic with y [N] (binary) or y [N, L] (multi-label, one tree per label and round), or multi:softmax with
    integer y [N]; a classifier built without an objective takes binary:logistic."""
    _default_objective = "binary:logistic"

    def __init__(self, **kw):
        super().__init__(**kw)
        if self.objective == "reg:squarederror":
            raise ValueError("XGBClassifier with objective reg:squarederror: use XGBRegressor")

    def predict_proba(self, X):
        """[N, 2] (binary: 1 - p, p), [N, L] (multi-label) or [N, C] (softmax), fp32 on the device"""
        m = self.predict_margin(X)
        if self.objective == "multi:softmax":
            return torch.softmax(m, dim=1)
        p = torch.sigmoid(m)
        return torch.cat([1.0 - p, p], dim=1) if self.n_outputs_ == 1 else p

    def predict(self, X):
        """class labels: 0 / 1 [N] (binary), 0 / 1 [N, L] (multi-label: margin > 0, i.e. p > 0.5), argmax [N] (softmax; the first of equal margins); int64"""
        m = self.predict_margin(X)
        if self.objective == "multi:softmax":
            return torch.argmax(m, dim=1)
        lab = (m > 0).to(torch.int64)
        return lab.squeeze(1) if self.n_outputs_ == 1 else lab


class XGBRegressor(_GBT):
    """ref saprot_fit_reg.py:26-32.  One output, so depths 7 .. 9 are built too (levels 6 .. 8 in groups of nodes: oneprot_amd/gbt_deep.py), as the reference's
    regression sweep asks (max_depth 3, 5, 9)."""
    _default_objective = "reg:squarederror"
    _max_depth = MAX_DEPTH

    def predict(self, X):
        return self.predict_margin(X).squeeze(1)


# ---------------------------------------------------------------------------------------------------------------------------------
TARGETS = {"xgboost.XGBClassifier": XGBClassifier, "xgboost.XGBRegressor": XGBRegressor, "oneprot_amd.gbt.XGBClassifier": XGBClassifier,
           "oneprot_amd.gbt.XGBRegressor": XGBRegressor}


def objective_of(task_name):
    """ref saprot_fit_cls.py:23-30"""
    if task_name in downstream.BINARY_TASKS or task_name in downstream.MULTILABEL_TASKS:
        return "binary:logistic"
    if task_name in downstream.REGRESSION_TASKS:
        return "reg:squarederror"
    return "multi:softmax"


def build_model(cfg):
    """hydra.utils.instantiate(cfg.downstream_model) (ref saprot_fit_cls.py:32, saprot_fit_reg.py:26) without Hydra: `_target_` xgboost.XGBClassifier /
    xgboost.XGBRegressor resolve to the classes of this module; the classifier's objective follows the task (ref :23-30)"""
    dm = dict(cfg["downstream_model"])
    target = dm.pop("_target_", None)
    if target not in TARGETS:
        raise ValueError(f"downstream_model._target_ = {target!r}; one of {', '.join(TARGETS)}")
    cls = TARGETS[target]
    if cls is XGBClassifier:
        dm["objective"] = objective_of(cfg["task_name"])
    return cls(**dm)


def evaluate(cfg, data, scores="labels"):
    """ref evaluate (saprot_fit_cls.py:22-67, saprot_fit_reg.py:25-41): fit on `train`, predict `valid` and `test`, and return the reference's result dict.
    scores="labels" (the default) feeds predict's LABELS into AUC and F1-max, as the reference does; scores="proba" feeds the probabilities.  The fitted model is
    left in evaluate.last."""
    if scores not in ("labels", "proba"):
        raise ValueError("scores: 'labels' or 'proba'")
    task = cfg["task_name"]
    model = build_model(cfg)
    model.fit(data["train_emb"], data["train_target"])
    results = {}
    for partition in ("valid", "test"):
        x = data[f"{partition}_emb"]
        if scores == "proba" and isinstance(model, XGBClassifier) and model.objective == "binary:logistic":
            pred = model.predict_proba(x)
            pred = pred[:, 1] if model.n_outputs_ == 1 else pred
        else:
            pred = model.predict(x)
        if task in downstream.BINARY_TASKS or task in downstream.MULTILABEL_TASKS:
            pred = pred.to(torch.float32)
        results.update(downstream.evaluate_predictions(task, pred, data[f"{partition}_target"], partition))
    evaluate.last = model
    return results


SWEEP_KEYS = ("max_depth", "learning_rate", "min_child_weight", "n_estimators", "gamma", "subsample", "colsample_bytree", "reg_alpha", "reg_lambda", "task_name",
              "model_type")


def sweep(cfg, data):
    """the basic sweeper's product over cfg["sweep"] (ref configs/saprot_sweep_xgboost_{cls,reg}.yaml): one row per combination, {the combination's values,
    the results}.  data: one mapping as evaluate takes it, or a callable (cfg) -> mapping that loads a combination's task (load_data)."""
    keys = [k for k in SWEEP_KEYS if k in cfg["sweep"]]
    rows = []
    for combo in itertools.product(*(cfg["sweep"][k] for k in keys)):
        c = {k: cfg[k] for k in cfg.keys() if k not in ("sweep", "downstream_model")}
        c["downstream_model"] = dict(cfg["downstream_model"])
        for k, v in zip(keys, combo):
            if k in ("task_name", "model_type"):
                c[k] = v
            else:
                c["downstream_model"][k] = v
        results = evaluate(c, data(c) if callable(data) else data)
        rows.append({**dict(zip(keys, combo)), **results})
    return rows


load_data = downstream.load_data


def cli_main(argv, default_config, description):
    """the command line of src/saprot_fit_cls.py / src/saprot_fit_reg.py: yaml + key=value overrides on dotted keys, no Hydra"""
    import argparse
    import json
    import yaml
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--config", default=default_config)
    ap.add_argument("--one", action="store_true", help="one fit of the `downstream_model:` block instead of the sweep")
    ap.add_argument("--scores", default="labels", choices=("labels", "proba"), help="what AUC and F1-max are fed with (the reference feeds predict's labels)")
    ap.add_argument("overrides", nargs="*")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        cfg = yaml.safe_load(f)
    dm = cfg.get("downstream_model")
    if isinstance(dm, str):                                                    # the name of a file under configs/downstream_model/, as Hydra's defaults list names it
        with open(os.path.join(os.path.dirname(os.path.abspath(args.config)), "downstream_model", dm + ".yaml")) as f:
            cfg["downstream_model"] = yaml.safe_load(f)
    for ov in args.overrides:
        key, _, value = ov.partition("=")
        node, parts = cfg, key.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = yaml.safe_load(value)
    if args.one:
        print(json.dumps({"task_name": cfg["task_name"], "model_type": cfg["model_type"], **evaluate(cfg, load_data(cfg), scores=args.scores)}))
    else:
        for row in sweep(cfg, load_data):
            print(json.dumps(row))
