#!/usr/bin/env python3
"""Variational tri-factorisations one by one against many per launch (bnmtf_vb_run_many, csrc/api_many.inc), on one GPU, every
alternative in the same process:

  1. microseconds per model-iteration of 1, 10 and 40 GDSC-shaped models (622 x 138, 19 % missing; (K, L) in 5..10 x folds;
     --iters iterations): each model's own run() in turn against ONE bnmtf_amd.run_many of them (the device's clock of the calls,
     and the wall clock), alternated --reps times; the fastest of the repetitions;
  2. the wall seconds of the greedy-search cross-validation job of experiments_gdsc/cross_validation/vb_nmtf/greedysearch_xval_vb.py
     on synthetic 622 x 138 data with 19 % missing (--folds folds, K, L in 5..10, init S random / F, G k-means, --cv-iters
     iterations, AIC) with one slot: an unbatched ReplicaPool against ReplicaPool(batched=True), and whether the two choose and
     score the same.

One JSON line per measurement; --out also writes them to a file.

    python tools/trivb_many_rates.py [--out profiles/trivb_many_rates.json] [--iters 300] [--cv-iters 1000] [--folds 10]
"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnmtf_amd import bnmtf_vb_optimised, run_many                                          # noqa: E402
from bnmtf_amd.cross_validation.greedy_search_cross_validation import GreedySearchCrossValidation   # noqa: E402
from bnmtf_amd.cross_validation.replicas import ReplicaPool                                 # noqa: E402
from bnmtf_amd.synthetic import generate_bnmtf                                              # noqa: E402

PRI = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
KL = [(K, L) for K in range(5, 11) for L in range(5, 11)]


def models(n, R):
    """n models of the GDSC shape: (K, L) from 5..10 (in turn), every one on a fold mask of its own"""
    out = []
    for i in range(n):
        K, L = KL[(7 * i) % len(KL)]
        rs = np.random.RandomState(100 + i)
        M = (rs.rand(*R.shape) >= 0.19).astype(float)
        np.random.seed(200 + i); random.seed(300 + i)
        m = bnmtf_vb_optimised(R, M, K, L, PRI, verbose=False)
        m.initialise("random", "random")
        out.append(m)
    return out


def per_model_iteration(n, R, iters, reps):
    best = {}
    for _ in range(reps):
        for how in ("in_turn", "run_many") if n > 1 else ("in_turn",):
            ms = models(n, R)
            random.seed(0)
            t0 = time.perf_counter()
            if how == "in_turn":
                for m in ms:
                    m.run(iters)
                dev = sum(m.all_times[-1] for m in ms)
            else:
                run_many(ms, iters)
                dev = ms[0].all_times[-1]
            wall = time.perf_counter() - t0
            us_dev, us_wall = dev / (n * iters) * 1e6, wall / (n * iters) * 1e6
            if how not in best or us_dev < best[how][0]:
                best[how] = (us_dev, us_wall, ms[0]._many_info[:2] if how == "run_many" else None)
    d = {"measure": "us_per_model_iteration", "models": n, "shape": list(R.shape), "iterations": iters, "reps": reps}
    for how, (dv, wl, info) in best.items():
        d[how + "_device_us"] = round(dv, 2); d[how + "_wall_us"] = round(wl, 2)
        if info:
            d["run_many_models_sharing_launches"], d["run_many_uploads"] = info
    if "run_many" in best:
        d["gain_device"] = round(best["in_turn"][0] / best["run_many"][0], 2)
    return d


def greedy(R, M, folds, iters, batched, path):
    random.seed(0); np.random.seed(0)
    pool = ReplicaPool(devices=[0], shared={"R": R}, batched=batched)
    t0 = time.perf_counter()
    cv = GreedySearchCrossValidation(classifier=bnmtf_vb_optimised, R=R, M=M, values_K=list(range(5, 11)), values_L=list(range(5, 11)),
                                     folds=folds, priors=PRI, init_S="random", init_FG="kmeans", iterations=iters, restarts=1,
                                     quality_metric="AIC", file_performance=path, pool=pool, seed=7)
    cv.run()
    dt = time.perf_counter() - t0
    pool.close()
    cv.fout.close()
    return dt, cv.performances, open(path).read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cv-iters", type=int, default=1000)
    ap.add_argument("--folds", type=int, default=10)
    ap.add_argument("--skip-cv", action="store_true")
    a = ap.parse_args()
    R, M, _, _, _ = generate_bnmtf(622, 138, 8, 8, 0.19, seed_data=1, seed_mask=2)
    R = np.asarray(R, dtype=float)
    lines = []
    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)
    run_many(models(2, R), 3)                                      # (library, kernels)
    for n in (1, 10, 40):
        emit(per_model_iteration(n, R, a.iters, a.reps))
    if not a.skip_cv:
        tmp = tempfile.mkdtemp()
        try:
            t1, p1, log1 = greedy(R, M, a.folds, a.cv_iters, False, os.path.join(tmp, "one.txt"))
            tb, pb, logb = greedy(R, M, a.folds, a.cv_iters, True, os.path.join(tmp, "batched.txt"))
        finally:
            shutil.rmtree(tmp)
        emit({"measure": "greedysearch_xval_vb", "shape": list(R.shape), "missing": 0.19, "folds": a.folds, "values_K": "5..10", "values_L": "5..10",
              "iterations": a.cv_iters, "wall_s_unbatched": round(t1, 2), "wall_s_batched": round(tb, 2), "speedup": round(t1 / tb, 2),
              "identical_performances": p1 == pb, "identical_logs": log1 == logb})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
