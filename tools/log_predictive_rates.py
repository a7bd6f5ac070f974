"""What bnmtf_amd.log_predictive costs, beside bnmtf_amd.posterior_predictive on the same inputs in the same process -- the same
gather, so the difference is the price of the five accumulators and the exp -- and beside NumPy fp64 on the same host.

    python tools/log_predictive_rates.py --out profiles/log_predictive_rates.json

Per configuration (tools/predictive_rates.py's three) a fresh child process (this one never touches the GPU): a model with
layout='observed' on a synthetic matrix of which about a tenth is observed, run for as many iterations as samples are wanted
(store_samples=True: the samples sit in the page-locked arrays of _lib.sample_buffer), and a list of entries drawn uniformly from
the whole matrix, repeats included, with the matrix's own values plus unit noise.  Timed: the wall time of log_predictive(model,
Entries, 0, 1) and of posterior_predictive(model, Entries, 0, 1) -- host clock around the call, everything in it included --
`--repeats` times each after one untimed call, and of each call the upload and the kernel time from the events on the call's own
stream (bnmtf_log_predictive_times, bnmtf_predictive_times).  The NumPy side forms l_t in fp64 over the first `--numpy-samples`
samples only, with their two-pass log-sum-exp, mean and variance, and is scaled to all samples: its time is linear in them.  lpd
and mean over that subset are compared.  The shader clock is read beside a few more calls (bench.py's helper)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from predictive_rates import CONFIGS, problem  # noqa: E402


def numpy_statistics(rows, cols, values, factors, taus, samples):
    """(lpd, mean, variance) over the first `samples` samples, fp64"""
    l = np.empty((samples, len(rows)))
    for t in range(samples):
        a = factors[0][t].astype(np.float64)
        if len(factors) == 3:
            a = a @ factors[1][t].astype(np.float64)
        d = values - np.einsum('ek,ek->e', a[rows], factors[-1][t].astype(np.float64)[cols])
        l[t] = 0.5 * (np.log(taus[t]) - np.log(2.0 * np.pi)) - 0.5 * taus[t] * d * d
    m = l.max(0)
    return m + np.log(np.exp(l - m).sum(0)) - np.log(float(samples)), l.mean(0), l.var(0, ddof=1)


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    import ctypes as C
    from bnmtf_amd import Entries, _lib, bnmf_gibbs_optimised, bnmtf_gibbs_optimised, log_predictive, posterior_predictive
    n, K, L, entries, samples = CONFIGS[a.child]
    R, M = problem(n, K, L)
    np.random.seed(0)
    if L:
        m = bnmtf_gibbs_optimised(R, M, K, L, dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.), seed=1, verbose=False, layout='observed')
    else:
        m = bnmf_gibbs_optimised(R, M, K, dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.), seed=1, verbose=False, layout='observed')
    m.initialise()
    t0 = time.perf_counter()
    m.run(samples)
    run_s = time.perf_counter() - t0
    rs = np.random.RandomState(1)
    rows, cols = rs.randint(0, n, entries).astype(np.int32), rs.randint(0, n, entries).astype(np.int32)
    E = Entries((n, n), rows, cols, R[rows, cols].astype(np.float64) + rs.randn(entries))
    factors = [getattr(m, "all_" + f) for f in m._FACTORS]
    taus = np.asarray(m.all_tau, dtype=np.float64)

    def timed(call, times):
        call()
        wall, upload, kernel = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = call()
            wall.append(time.perf_counter() - t0)
            up, kn = C.c_double(), C.c_double()
            _lib.check(times(C.byref(up), C.byref(kn)))
            upload.append(up.value); kernel.append(kn.value)
        return out, {"wall_s": [round(t, 4) for t in wall], "wall_s_median": round(statistics.median(wall), 4),
                     "upload_ms": [round(t, 2) for t in upload], "kernel_ms": [round(t, 2) for t in kernel],
                     "upload_ms_median": round(statistics.median(upload), 2), "kernel_ms_median": round(statistics.median(kernel), 2),
                     "kernel_share_of_call": round(statistics.median(kernel) * 1e-3 / statistics.median(wall), 3)}

    def call():
        return log_predictive(m, E, 0, 1)

    Q, new = timed(call, _lib.lib().bnmtf_log_predictive_times)
    P, old = timed(lambda: posterior_predictive(m, E, 0, 1), _lib.lib().bnmtf_predictive_times)
    clock = bench._clock_beside(helper, call, lambda: None) if helper is not None else None
    # NumPy on the same host, over the first samples only
    t0 = time.perf_counter()
    ref = numpy_statistics(rows, cols, E.values, factors, taus, a.numpy_samples)
    numpy_s = time.perf_counter() - t0
    sub = log_predictive.from_samples(factors, taus, (n, n), rows, cols, E.values, range(a.numpy_samples))
    sample_bytes = sum(f[0].nbytes for f in factors)
    W = L if L else K
    out = {"config": a.child, "I": n, "J": n, "K": K, "L": L, "entries": entries, "samples": samples, "model_run_s": round(run_s, 2),
           "sample_bytes_uploaded": sample_bytes * samples, "multiply_adds": float(entries) * W * samples,
           "log_predictive": new, "posterior_predictive_same_inputs": old,
           "kernel_ms_over_posterior_predictive": round(new["kernel_ms_median"] / old["kernel_ms_median"], 2),
           "accumulator_bytes_per_entry_sample": {"log_predictive": 88, "posterior_predictive": 40, "gathered": 4 * W},
           "upload_GB_per_s": round(sample_bytes * samples / (new["upload_ms_median"] * 1e-3) / 1e9, 2),
           "numpy_samples_timed": a.numpy_samples, "numpy_s_timed": round(numpy_s, 3), "numpy_s_scaled_to_all_samples": round(numpy_s * samples / a.numpy_samples, 2),
           "numpy_over_device": round(numpy_s * samples / a.numpy_samples / new["wall_s_median"], 1),
           "lpd_largest_difference_on_the_subset": float(np.max(np.abs(sub.lpd - ref[0]))),
           "mean_largest_relative_difference_on_the_subset": float(np.max(np.abs(sub.mean - ref[1]) / np.abs(ref[1]))),
           "lppd": Q.lppd(), "p_waic": Q.p_waic(), "waic": Q.waic(), "se": Q.se(),
           "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    print("LOG_PREDICTIVE_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_predictive_rates.json"))
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--numpy-samples", type=int, default=4)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--no-clock", action="store_true")
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--repeats", str(a.repeats), "--numpy-samples", str(a.numpy_samples)]
        if a.no_clock:
            cmd.append("--no-clock")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("LOG_PREDICTIVE_RATES ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("child failed: %s" % cfg)          # (nothing more is started on the GPU)
        results.append(json.loads(line[0][len("LOG_PREDICTIVE_RATES "):]))
        print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "bnmtf_amd.log_predictive over the stored samples of a layout='observed' model (page-locked sample arrays), and "
                               "bnmtf_amd.posterior_predictive on the same inputs in the same process: wall time of the call in s (host clock, "
                               "everything included), upload and kernel time in ms from events on the call's stream, beside NumPy fp64 on the "
                               "same host over the first numpy_samples_timed samples scaled to all of them; sclk_mhz: the shader clock "
                               "(rocm-smi) beside further calls; tools/log_predictive_rates.py",
                       "configs": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
