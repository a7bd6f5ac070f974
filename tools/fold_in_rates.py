"""What bnmtf_amd.fold_in costs, beside the same chain in NumPy fp64 on the same host.

    python tools/fold_in_rates.py --out profiles/fold_in_rates.json

Per configuration a fresh child process (this one never touches the GPU): an exponential fixed factor of m = 4096 rows and rank W,
n_new units of c entries each (values of rank 8, rates 1), and fold_in.from_factors(other, new, 1.0, tau, 1000): a Gibbs chain of
T = 1000 sweeps per unit in one launch.  Timed: the wall time of the call -- host clock around it, everything in it included: the
sort of the entries, the checks, the fp32 copies of the fixed factor, the device allocations, the uploads, the kernel, the download
-- `--repeats` times after one untimed call (every time and the median are reported), and of each call the upload and the kernel
time from the events on the call's own stream (bnmtf_fold_in_times).  From the kernel time: unit-sweeps/s = n_new T / t and
draws/s = n_new T W / t.  The NumPy side runs the same chain -- the residual rebuilt at every sweep, the columns in order, the draws
by oracle/rng.tn_draw with the fold-in stream -- vectorised over the units, for `numpy_sweeps` sweeps only, and the time is scaled
to T: the file says from how many.  The shader clock is read beside a few more calls (bench.py's helper)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M_ROWS, T, TAU, SEED = 4096, 1000, 2.0, 11
CONFIGS = {"w%d_n%d_c%d" % (W, n, c): (W, n, c) for W in (32, 256) for n in (1, 256, 4096) for c in (32, 400)}


def problem(W, n, c, seed=0):
    from bnmtf_amd import Entries
    rs = np.random.RandomState(seed)
    other = rs.exponential(1.0, (M_ROWS, W)).astype(np.float32).astype(np.float64)
    k = min(W, 8)
    truth = rs.exponential(1.0, (n, k))
    idx = np.stack([np.sort(rs.choice(M_ROWS, size=c, replace=False)) for _ in range(n)])          # [n][c]
    vals = np.einsum('nk,nck->nc', truth, other[:, :k][idx]).astype(np.float32).astype(np.float64)
    new = Entries((n, M_ROWS), np.repeat(np.arange(n), c), idx.ravel(), vals.ravel())
    return other, new, idx, vals


def numpy_chain(other, idx, vals, sweeps):
    """seconds for `sweeps` sweeps of every unit's chain in fp64"""
    from oracle import rng
    n, c = idx.shape
    W = other.shape[1]
    X = np.ones((n, W))
    elem = np.arange(n)
    t0 = time.perf_counter()
    A = np.stack([(other[idx, k] ** 2).sum(1) for k in range(W)], axis=1)                   # a_k, once
    for t in range(sweeps):
        E = vals.copy()
        for k in range(W):
            E -= X[:, k, None] * other[idx, k]
        for k in range(W):
            y = other[idx, k]
            tau_p = TAU * A[:, k]
            mu = (-1.0 + TAU * ((E * y).sum(1) + X[:, k] * A[:, k])) / tau_p
            x = rng.tn_draw(mu, tau_p, elem, k, t, 4, SEED)
            E -= (x - X[:, k])[:, None] * y
            X[:, k] = x
    return time.perf_counter() - t0


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    import ctypes as C
    from bnmtf_amd import _lib, fold_in
    W, n, c = CONFIGS[a.child]
    other, new, idx, vals = problem(W, n, c)

    def call():
        return fold_in.from_factors(other, new, 1.0, TAU, T, seed=SEED)

    F = call()
    wall, upload, kernel = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        F = call()
        wall.append(time.perf_counter() - t0)
        up, kn = C.c_double(), C.c_double()
        _lib.check(_lib.lib().bnmtf_fold_in_times(C.byref(up), C.byref(kn)))
        upload.append(up.value); kernel.append(kn.value)
    clock = bench._clock_beside(helper, call, lambda: None) if helper is not None else None
    k_s = statistics.median(kernel) * 1e-3
    out = {"config": a.child, "m": M_ROWS, "W": W, "n_new": n, "entries_per_unit": c, "sweeps": T,
           "wall_s": [round(t, 4) for t in wall], "wall_s_median": round(statistics.median(wall), 4),
           "upload_ms": [round(t, 3) for t in upload], "kernel_ms": [round(t, 3) for t in kernel],
           "upload_ms_median": round(statistics.median(upload), 3), "kernel_ms_median": round(statistics.median(kernel), 3),
           "unit_sweeps_per_s": float("%.4g" % (n * T / k_s)), "draws_per_s": float("%.4g" % (n * T * W / k_s)),
           "us_per_column_of_one_unit": round(k_s * 1e6 / (T * W), 3),
           "mean_of_the_means": float("%.6g" % F.mean.mean()),
           "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    if not a.no_numpy:
        sweeps = 1 if float(n) * c * W > 2e7 else (3 if float(n) * c * W > 1e6 else 10)
        s = numpy_chain(other, idx, vals, sweeps)
        out.update({"numpy_sweeps": sweeps, "numpy_s_measured": round(s, 3), "numpy_s_scaled_to_all_sweeps": round(s * T / sweeps, 1),
                    "numpy_over_device_wall": round(s * T / sweeps / out["wall_s_median"], 1)})
    print("FOLD_IN_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_in_rates.json"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--no-clock", action="store_true")
    p.add_argument("--no-numpy", action="store_true")
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--repeats", str(a.repeats)]
        cmd += ["--no-clock"] if a.no_clock else []
        cmd += ["--no-numpy"] if a.no_numpy else []
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("FOLD_IN_RATES ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("child failed: %s" % cfg)          # (nothing more is started on the GPU)
        results.append(json.loads(line[0][len("FOLD_IN_RATES "):]))
        print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "bnmtf_amd.fold_in.from_factors(other, new, 1.0, tau, 1000) -- a Gibbs chain of 1000 sweeps per new unit in one launch, "
                               "fixed factor of 4096 rows: wall time of the call in s (host clock, everything included), upload and kernel time in ms "
                               "from events on the call's stream, unit-sweeps/s and draws/s over the kernel time, beside the same chain in NumPy fp64 on "
                               "the same host, timed on numpy_sweeps sweeps and scaled to 1000; sclk_mhz: the shader clock (rocm-smi) beside further "
                               "calls; tools/fold_in_rates.py",
                       "configs": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
