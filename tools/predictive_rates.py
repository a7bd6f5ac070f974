"""What bnmtf_amd.posterior_predictive costs, beside NumPy fp64 computing the same statistics on the same host.

    python tools/predictive_rates.py --out profiles/predictive_rates.json

Per configuration a fresh child process (this one never touches the GPU): a model with layout='observed' on a synthetic matrix of
which about a tenth is observed, run for as many iterations as samples are wanted (store_samples=True: the samples sit in the
page-locked arrays of _lib.sample_buffer), and a list of entries drawn uniformly from the whole matrix, repeats included.  Timed:
the wall time of posterior_predictive(model, (rows, cols), 0, 1) -- host clock around the call, everything in it included: the
sort of the list, the device allocations, the uploads, the kernel, the download, the two divisions -- `--repeats` times after one
untimed call, and of each call the upload and the kernel time from the events on the call's own stream (bnmtf_predictive_times).
The NumPy side runs the same shifted sums (p of the first sample, sums of p_t - p_first and of its square) in fp64 over the first
`--numpy-samples` samples only -- the file says from how many -- and is scaled to all of them: its time is linear in the samples.
Both means over that subset are compared.  The shader clock is read beside a few more calls (bench.py's helper)."""
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
# name -> (I = J, K, L, entries to predict, samples)
CONFIGS = {"bnmf_4096_k32": (4096, 32, 0, 1600000, 200), "bnmf_8192_k64": (8192, 64, 0, 1000000, 100), "bnmtf_4096_k32_l32": (4096, 32, 32, 1600000, 200)}


def problem(n, K, L, seed=0):
    rs = np.random.RandomState(seed)
    U = rs.exponential(1.0, (n, K)).astype(np.float32)
    V = rs.exponential(1.0, (n, L if L else K)).astype(np.float32)
    R = (U @ rs.exponential(1.0, (K, L)).astype(np.float32) @ V.T) if L else U @ V.T
    M = np.zeros((n, n), dtype=np.float32)
    for i0 in range(0, n, 1024):
        M[i0:i0 + 1024] = rs.random_sample((min(n, i0 + 1024) - i0, n)) < 0.1
    M[np.arange(n), rs.randint(0, n, n)] = 1; M[rs.randint(0, n, n), np.arange(n)] = 1
    return R, M


def numpy_sums(rows, cols, factors, samples):
    """(p_first, sum_d, sum_d2) over the first `samples` samples, fp64"""
    p_first = sum_d = sum_d2 = None
    for t in range(samples):
        a = factors[0][t].astype(np.float64)
        if len(factors) == 3:
            a = a @ factors[1][t].astype(np.float64)
        p = np.einsum('ek,ek->e', a[rows], factors[-1][t].astype(np.float64)[cols])
        if t == 0:
            p_first, sum_d, sum_d2 = p, np.zeros_like(p), np.zeros_like(p)
        else:
            d = p - p_first
            sum_d += d; sum_d2 += d * d
    return p_first, sum_d, sum_d2


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    import ctypes as C
    from bnmtf_amd import _lib, bnmf_gibbs_optimised, bnmtf_gibbs_optimised, posterior_predictive, predictive
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
    factors = [getattr(m, "all_" + f) for f in m._FACTORS]

    def call():
        return posterior_predictive(m, (rows, cols), 0, 1)

    call()
    wall, upload, kernel = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        P = call()
        wall.append(time.perf_counter() - t0)
        up, kn = C.c_double(), C.c_double()
        _lib.check(_lib.lib().bnmtf_predictive_times(C.byref(up), C.byref(kn)))
        upload.append(up.value); kernel.append(kn.value)
    clock = bench._clock_beside(helper, call, lambda: None) if helper is not None else None
    # NumPy on the same host, over the first samples only
    t0 = time.perf_counter()
    ref = numpy_sums(rows, cols, factors, a.numpy_samples)
    numpy_s = time.perf_counter() - t0
    sub = predictive.from_samples(factors, m.all_tau, (n, n), rows, cols, range(a.numpy_samples))
    ref_mean = ref[0] + ref[1] / a.numpy_samples
    sample_bytes = sum(f[0].nbytes for f in factors)
    out = {"config": a.child, "I": n, "J": n, "K": K, "L": L, "entries": entries, "samples": samples, "model_run_s": round(run_s, 2),
           "sample_bytes_uploaded": sample_bytes * samples, "multiply_adds": float(entries) * (L if L else K) * samples,
           "wall_s": [round(t, 4) for t in wall], "wall_s_median": round(statistics.median(wall), 4),
           "upload_ms": [round(t, 2) for t in upload], "kernel_ms": [round(t, 2) for t in kernel],
           "upload_ms_median": round(statistics.median(upload), 2), "kernel_ms_median": round(statistics.median(kernel), 2),
           "upload_GB_per_s": round(sample_bytes * samples / (statistics.median(upload) * 1e-3) / 1e9, 2),
           "numpy_samples_timed": a.numpy_samples, "numpy_s_timed": round(numpy_s, 3), "numpy_s_scaled_to_all_samples": round(numpy_s * samples / a.numpy_samples, 2),
           "numpy_over_device": round(numpy_s * samples / a.numpy_samples / statistics.median(wall), 1),
           "mean_largest_relative_difference_on_the_subset": float(np.max(np.abs(sub.mean - ref_mean) / np.abs(ref_mean))),
           "variance_median": float(np.median(P.variance)), "noise": P.noise,
           "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    print("PREDICTIVE_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_rates.json"))
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
        line = [l for l in r.stdout.splitlines() if l.startswith("PREDICTIVE_RATES ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("child failed: %s" % cfg)          # (nothing more is started on the GPU)
        results.append(json.loads(line[0][len("PREDICTIVE_RATES "):]))
        print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "bnmtf_amd.posterior_predictive over the stored samples of a layout='observed' model (page-locked sample arrays): wall "
                               "time of the call in s (host clock, everything included), upload and kernel time in ms from events on the call's "
                               "stream, beside NumPy fp64 on the same host over the first numpy_samples_timed samples scaled to all of them; "
                               "sclk_mhz: the shader clock (rocm-smi) beside further calls; tools/predictive_rates.py",
                       "configs": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
