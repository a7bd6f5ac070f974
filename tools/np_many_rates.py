#!/usr/bin/env python3
"""One slot, two model searches of the non-probabilistic models on the GDSC matrix (622 x 138), fitted one by one and then batched
(MatrixCrossValidation(batched=True): the folds of a slot in one bnmtf_np_run_many call), in the same process:

    np_nmtf_xval   25 (K, L) settings, K, L in {2, 4, 6, 8, 10}, x 5 folds; init_FG='kmeans', init_S='exponential'
    np_nmf_xval    K in {2, ..., 10} x 10 folds; init_UV='random'

with fewer iterations than the experiment scripts (--iters).  Per job: the wall seconds of both runs, whether their performances
and log files are identical, and the launches per iteration -- one by one, the sum over the models of their records; batched,
the launch sites of the longest chain and their splits (launch_info, from a direct bnmtf_np_run_many of the job's models).  One
JSON line per job; --out also writes them to a file.

    python tools/np_many_rates.py [--out profiles/np_many_rates.json] [--iters 300]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnmtf_amd import _lib, data, NMF, NMTF                        # noqa: E402
from bnmtf_amd.cross_validation import MatrixCrossValidation      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def gdsc():
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, "gdsc.txt")
        with gzip.open(os.path.join(HERE, "..", "tests", "golden", "gdsc_ic50.txt.gz"), "rb") as fi, open(path, "wb") as fo:
            fo.write(fi.read())
        _, X_min, M = data.load_gdsc(path)[:3]
    finally:
        shutil.rmtree(tmp)
    return X_min, M


def records_per_iteration(kind, K, L):
    """Launches of one model's own iteration (api_np.inc: np_iteration)."""
    return 3 if kind == "NMF" else 2 + (K * L + 1) + 6


def cv(method, X, M, search, config, folds, batched, path):
    random.seed(0); np.random.seed(0)
    t0 = time.perf_counter()
    c = MatrixCrossValidation(method=method, X=X, M=M, K=folds, parameter_search=search, train_config=config, file_performance=path,
                              batched=batched)
    c.run()
    c.fout.close()
    return time.perf_counter() - t0, c.all_performances, open(path).read()


def launch_info(method, X, M, search, folds):
    """launch_info of one bnmtf_np_run_many call over the job's models (every setting x folds, one iteration): the models,
    the argument-list uploads = the launches of the first iteration."""
    ms = []
    np.random.seed(0)
    for p in search:
        for f in range(folds):
            m = method(X, M, verbose=False, **p)
            if method is NMTF:
                m.initialise("random", "random")
            else:
                m.initialise("random")
            m._push()
            ms.append(m)
    hs = (C.c_void_p * len(ms))(*[m._handle().value for m in ms])
    info = np.zeros(2, dtype=np.int32)
    _lib.check(_lib.lib().bnmtf_np_run_many(hs, len(ms), 1, None, None, None, _lib.ptr(info)))
    for m in ms:
        m.close()
    return int(info[0]), int(info[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=300)
    a = ap.parse_args()
    X, M = gdsc()
    lines = []
    tmp = tempfile.mkdtemp()
    jobs = [("np_nmtf_xval", NMTF, [{"K": K, "L": L} for K in (2, 4, 6, 8, 10) for L in (2, 4, 6, 8, 10)],
             {"iterations": a.iters, "init_FG": "kmeans", "init_S": "exponential"}, 5),
            ("np_nmf_xval", NMF, [{"K": K} for K in range(2, 11)], {"iterations": a.iters, "init_UV": "random"}, 10)]
    try:
        for name, method, search, config, folds in jobs:
            cv(method, X[:40], M[:40], search[:1], dict(config, iterations=2), 2, True, os.path.join(tmp, "warm.txt"))   # (library, kernels)
            t1, p1, log1 = cv(method, X, M, search, config, folds, False, os.path.join(tmp, name + "_1.txt"))
            tb, pb, logb = cv(method, X, M, search, config, folds, True, os.path.join(tmp, name + "_b.txt"))
            n_models, first_launches = launch_info(method, X, M, search, folds)
            one = sum(records_per_iteration(method.__name__, p["K"], p.get("L", 0)) for p in search) * folds
            d = {"job": name, "shape": list(X.shape), "settings": len(search), "folds": folds, "iterations": a.iters,
                 "wall_s_one_by_one": t1, "wall_s_batched": tb, "speedup": t1 / tb,
                 "launches_per_iteration_one_by_one": one, "launches_per_iteration_batched": first_launches,
                 "models_sharing_launches": n_models, "identical_performances": p1 == pb, "identical_logs": log1 == logb}
            s = json.dumps(d)
            print(s, flush=True)
            lines.append(s)
    finally:
        shutil.rmtree(tmp)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
