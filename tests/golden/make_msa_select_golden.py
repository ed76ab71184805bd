#!/usr/bin/env python
"""Writes tests/golden/msa_select.json: the reference's greedy_select on drawn alignments.

TEST INFRASTRUCTURE, like make_golden.py: it runs only where the reference checkout is mounted read-only at /root/reference, imports the reference's
src/data/utils/msa_utils.py (scipy is needed; a stub module stands in for `Bio`, which greedy_select never touches) and records
  - greedy_select's output (ref msa_utils.py:21-40) as index lists, on inputs kept as strings;
  - the parameter names and defaults of greedy_select and of MSADataset.__init__ (ref msa_dataset.py:9-10; stubs stand in for `esm` and, when absent,
    `transformers`, which only the constructor body uses).
No reference source is copied.

Every recorded case is TIE-FREE: at no step does the exact rule (tests/msa_select_ref.py) see two unselected rows share the best score.  On such inputs
the reference's fp64 means order the rows as the integer sums do; with a tie its pick is rounding noise.  Seeds are drawn until
there are CASES_PER_MODE such cases per mode with N >= 20, num_seqs >= 4 and L >= 100 (12 of 34 draws at these depths; about one in eight at depths up to 50)."""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
CASES_PER_MODE = 6


def _import_reference():
    if not os.path.isdir(REF):
        raise SystemExit("reference checkout not present; goldens are generated in the build container only")
    bio = types.ModuleType("Bio")
    bio.SeqIO = types.ModuleType("Bio.SeqIO")
    sys.modules.setdefault("Bio", bio)
    sys.modules.setdefault("Bio.SeqIO", bio.SeqIO)
    sys.modules.setdefault("esm", types.ModuleType("esm"))
    try:
        import transformers  # noqa: F401
    except Exception:
        tr = types.ModuleType("transformers")
        tr.AutoTokenizer = object
        sys.modules["transformers"] = tr
    # by file: the reference's package __init__ files import every dataset and their third-party libraries
    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    saved = {m: sys.modules.pop(m) for m in [m for m in sys.modules if m == "src" or m.startswith("src.")]}
    msa_utils = load("src.data.utils.msa_utils", "src/data/utils/msa_utils.py")
    try:
        for pkg in ("src", "src.data", "src.data.utils"):
            sys.modules[pkg] = types.ModuleType(pkg)
        sys.modules["src.data.utils.msa_utils"] = msa_utils
        msa_dataset = load("src.data.datasets.msa_dataset", "src/data/datasets/msa_dataset.py")
    finally:
        for name in [m for m in sys.modules if m == "src" or m.startswith("src.")]:
            del sys.modules[name]
        sys.modules.update(saved)
    return msa_utils, msa_dataset


def _signature(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        if p.name == "self":
            continue
        out.append([p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty])
    return out


def main():
    sys.path.insert(0, ROOT)
    from tests import msa_select_ref as R
    msa_utils, msa_dataset = _import_reference()
    cases, drawn = [], 0
    for mode in ("max", "min"):
        have, seed = 0, 0
        while have < CASES_PER_MODE:
            seed += 1
            drawn += 1
            rng = np.random.default_rng([seed, mode == "min"])
            N, L, k = int(rng.integers(20, 41)), int(rng.integers(100, 141)), int(rng.integers(4, 9))
            seqs = R.draw(int(rng.integers(1 << 30)), N, L, kind="iid" if seed % 2 else "mutated")
            want, _, tie_free = R.greedy(R.to_bytes(seqs), k, mode)
            if not tie_free:
                continue
            msa = [(f"r{i}", s) for i, s in enumerate(seqs)]
            got = [int(desc[1:]) for desc, _ in msa_utils.greedy_select(msa, num_seqs=k, mode=mode)]
            cases.append(dict(mode=mode, num_seqs=k, seqs=seqs, selected=got))
            have += 1
            if got != want:
                raise SystemExit(f"seed {seed} mode {mode}: tie-free, yet the reference selects {got} and the exact rule {want}")
    out = dict(source="ref src/data/utils/msa_utils.py:21-40 greedy_select, numpy %s" % np.__version__, draws=drawn, cases=cases,
               signatures=dict(greedy_select=_signature(msa_utils.greedy_select), MSADataset=_signature(msa_dataset.MSADataset.__init__)))
    path = os.path.join(HERE, "msa_select.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{path}: {len(cases)} tie-free cases out of {drawn} draws, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
