#!/usr/bin/env python3
"""Iteration rates of the non-probabilistic models (bnmtf_amd.nmf_np.NMF, bnmtf_amd.nmtf_np.NMTF) on one GPU: NMF at 4096^2,
K = 32 and 8192^2, K = 64; NMTF at the GDSC shape (622 x 138, 80 % observed, K = L = 5) and 4096^2, K = L = 32; and the wall
time of a GDSC-shaped 1 000-iteration NMF.train.  One JSON line per case; --out also writes them to a file.

    python tools/np_rates.py [--out profiles/np_rates.json] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnmtf_amd.nmf_np import NMF          # noqa: E402
from bnmtf_amd.nmtf_np import NMTF        # noqa: E402


def problem(I, J, frac, seed=0):
    rs = np.random.RandomState(seed)
    R = rs.rand(I, J) * 4 + 0.5
    M = (rs.rand(I, J) < frac).astype(float)
    M[:, 0] = 1; M[0, :] = 1
    return R, M


def rate(model, iters, warm):
    model.run(warm)                       # (the device state carries over: the timed run continues the chain)
    t0 = time.perf_counter()
    model.run(iters)
    dt = time.perf_counter() - t0
    return iters / dt, dt, model.all_times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer iterations")
    a = ap.parse_args()
    q = 0.2 if a.quick else 1.0
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    for I, K, iters in [(4096, 32, 200), (8192, 64, 40)]:
        R, M = problem(I, I, 0.8)
        np.random.seed(0)
        n = NMF(R, M, K, verbose=False); n.initialise("random")
        r, dt, dev = rate(n, max(2, int(iters * q)), 3)
        emit({"model": "NMF", "shape": [I, I], "K": K, "observed": 0.8, "it_per_s": r, "wall_s": dt, "device_s": dev})
        n.close()
    for I, J, K, iters in [(622, 138, 5, 1000), (4096, 4096, 32, 3)]:
        R, M = problem(I, J, 0.8)
        np.random.seed(0)
        t = NMTF(R, M, K, K, verbose=False); t.initialise("random", "random")
        r, dt, dev = rate(t, max(2, int(iters * q)), 1)
        emit({"model": "NMTF", "shape": [I, J], "K": K, "L": K, "observed": 0.8, "it_per_s": r, "wall_s": dt, "device_s": dev})
        t.close()
    R, M = problem(622, 138, 0.8)
    np.random.seed(0)
    n = NMF(R, M, 10, verbose=False)
    t0 = time.perf_counter()
    n.train(1000, init_UV="random")
    emit({"model": "NMF", "case": "GDSC-shaped train(1000), construction included", "shape": [622, 138], "K": 10,
          "wall_s": time.perf_counter() - t0, "device_s": n.all_times[-1]})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
