"""What bnmtf_amd.variational_predictive costs, beside the NumPy fp64 restatement of the same closed form on the same host.

    python tools/predictive_q_rates.py --out profiles/predictive_q_rates.json

Per configuration a fresh child process (this one never touches the GPU): the moments of a q of that shape (exponential means,
small variances: no model is fitted, the call takes the arrays a fitted class holds) and a list of entries drawn uniformly from the
whole matrix, repeats included.  Timed: the wall time of variational_predictive.from_moments(...) -- host clock around the call,
everything in it included: the checks of the moments, the sort of the list, the device allocations, the upload, the kernels, the
download -- `--repeats` times after one untimed call, and of each call the upload and the kernel time from the events on the call's
own stream (bnmtf_predictive_moments_times; the kernel time is the table pass and the entry pass together).  The NumPy side
computes the same two numbers per entry in fp64: row gathers and einsum for two factors, the K x L and J x K tables by matrix
products and then gathers for three.  Both answers are compared.  The shader clock is read beside a few more calls (bench.py's
helper).  The parent commit has no such call: there is no before."""
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
# name -> (I, J, K, L, entries)
CONFIGS = {"two_4096_k32": (4096, 4096, 32, 0, 1600000), "tri_4096_k32_l32": (4096, 4096, 32, 32, 1600000),
           "two_8192_k64": (8192, 8192, 64, 0, 1000000), "two_200000x150000_k32": (200000, 150000, 32, 0, 600000)}


def numpy_closed_form(rows, cols, EA, VA, ES, VS, EB, VB):
    if ES is None:
        f, a, g, c = EA[rows], VA[rows], EB[cols], VB[cols]
        return np.einsum('ek,ek->e', f, g), np.einsum('ek,ek->e', a, g * g) + np.einsum('ek,ek->e', c, f * f + a)
    P, H, u, w = EA @ ES, EB @ ES.T, VA @ (ES * ES), (EA * EA + VA) @ VS
    g, c, p = EB[cols], VB[cols], P[rows]
    return (np.einsum('el,el->e', p, g),
            np.einsum('ek,ek->e', VA[rows], H[cols] ** 2) + np.einsum('el,el->e', c, p * p + u[rows]) + np.einsum('el,el->e', g * g + c, w[rows]))


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    import ctypes as C
    from bnmtf_amd import _lib, variational_predictive
    n_i, n_j, K, L, entries = CONFIGS[a.child]
    rs = np.random.RandomState(0)
    W = L if L else K
    EA, VA = rs.exponential(1.0, (n_i, K)), 0.05 * rs.exponential(1.0, (n_i, K))
    ES, VS = (rs.exponential(1.0, (K, L)), 0.05 * rs.exponential(1.0, (K, L))) if L else (None, None)
    EB, VB = rs.exponential(1.0, (n_j, W)), 0.05 * rs.exponential(1.0, (n_j, W))
    rows, cols = rs.randint(0, n_i, entries).astype(np.int32), rs.randint(0, n_j, entries).astype(np.int32)
    factors = ((EA, VA), (ES, VS), (EB, VB)) if L else ((EA, VA), (EB, VB))

    def call():
        return variational_predictive.from_moments(factors, (n_i, n_j), rows, cols, alpha_s=100.0, beta_s=50.0)

    call()
    wall, upload, kernel = [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        P = call()
        wall.append(time.perf_counter() - t0)
        up, kn = C.c_double(), C.c_double()
        _lib.check(_lib.lib().bnmtf_predictive_moments_times(C.byref(up), C.byref(kn)))
        upload.append(up.value); kernel.append(kn.value)
    clock = bench._clock_beside(helper, call, lambda: None) if helper is not None else None
    numpy_s = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        ref = numpy_closed_form(rows, cols, EA, VA, ES, VS, EB, VB)
        numpy_s.append(time.perf_counter() - t0)
    operand_bytes = sum(x.nbytes for pair in factors for x in pair) + 8 * entries
    gathered = 8 * (K + 2 * L) if L else 16 * K                          # bytes of the column operands an entry's lane walks
    kn_s = statistics.median(kernel) * 1e-3
    out = {"config": a.child, "I": n_i, "J": n_j, "K": K, "L": L, "entries": entries,
           "wall_s": [round(t, 4) for t in wall], "wall_s_median": round(statistics.median(wall), 4),
           "upload_ms": [round(t, 3) for t in upload], "kernel_ms": [round(t, 3) for t in kernel],
           "upload_ms_median": round(statistics.median(upload), 3), "kernel_ms_median": round(statistics.median(kernel), 3),
           "bytes_uploaded": operand_bytes, "upload_GB_per_s": round(operand_bytes / (statistics.median(upload) * 1e-3) / 1e9, 2),
           "gathered_bytes_per_entry": gathered, "gather_TB_per_s_over_the_kernel_time": round(gathered * entries / kn_s / 1e12, 3),
           "table_pass_fma": float(n_j) * K * L, "staging_fma_at_most": 3.0 * min(n_i, entries) * K * L,
           "entries_per_s_over_the_kernel_time": round(entries / kn_s, 0),
           "numpy_s": [round(t, 4) for t in numpy_s], "numpy_s_median": round(statistics.median(numpy_s), 4),
           "numpy_over_device": round(statistics.median(numpy_s) / statistics.median(wall), 2),
           "mean_largest_relative_difference": float(np.max(np.abs(P.mean - ref[0]) / ref[0])),
           "variance_largest_relative_difference": float(np.max(np.abs(P.variance - ref[1]) / ref[1])),
           "variance_median": float(np.median(P.variance)), "noise": P.noise,
           "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    print("PREDICTIVE_Q_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_q_rates.json"))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--no-clock", action="store_true")
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in a.configs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--repeats", str(a.repeats)]
        if a.no_clock:
            cmd.append("--no-clock")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("PREDICTIVE_Q_RATES ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("child failed: %s" % cfg)          # (nothing more is started on the GPU)
        results.append(json.loads(line[0][len("PREDICTIVE_Q_RATES "):]))
        print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "bnmtf_amd.variational_predictive.from_moments on synthetic moments of q: wall time of the call in s (host clock, "
                               "everything included), upload and kernel time in ms from events on the call's stream (kernel: the table pass and "
                               "the entry pass together), beside the NumPy fp64 closed form on the same host; the parent commit has no such "
                               "call, so there is no before; sclk_mhz: the shader clock (rocm-smi) beside further calls; "
                               "tools/predictive_q_rates.py",
                       "configs": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
