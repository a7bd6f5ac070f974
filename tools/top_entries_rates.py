"""What bnmtf_amd.top_entries costs, beside NumPy fp64 computing the same answer on the same host.

    python tools/top_entries_rates.py --out profiles/top_entries_rates.json

Per configuration a fresh child process (this one never touches the GPU): exponential fp64 factors, an exclusion list of about a
tenth of the matrix (the share a 90 %-missing training set has) -- or, for the large case, 600 000 entries of a 200 000 x 150 000
matrix --, and top_entries.from_factors(factors, 10, rows=.., exclude=..), which is what top_entries(model, 10) runs once it has the
model's factors and training entries.  Timed: the wall time of the call -- host clock around it, everything in it included: the
checks, the sort of the exclusion list, the device allocations, the uploads, the kernels, the download -- `--repeats` times after
one untimed call (the median is reported), and of each call the upload and the kernel time from the events on the call's own
stream (bnmtf_top_entries_times).  From the kernel time and the shapes: fmas/s = r J W / t and B bytes/s = r J W 8 / t, the bytes
of B the wave-per-row form reads from the caches (B itself is J W 8 bytes: it is read r times).  The NumPy side: A[rows chunk] @ B.T
in chunks of rows, the excluded entries set to -+inf, argpartition and a sort of the n kept -- the exclusion list is sorted by row
before the clock starts.  Near-ties may come out in another order there (NumPy sums in another order): the file says in how many
rows the columns differ.  The shader clock is read beside a few more calls (bench.py's helper)."""
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
N = 10
# name -> (I, J, K, L, excluded entries (None: a tenth of the matrix), rows asked for (None: all), splits timed)
CONFIGS = {"bnmf_4096_k32": (4096, 4096, 32, 0, None, None, (0,)),
           "bnmf_8192_k64": (8192, 8192, 64, 0, None, None, (0,)),
           "bnmtf_4096_k32_l32": (4096, 4096, 32, 32, None, None, (0,)),
           "entries_200000x150000_k32_4096rows": (200000, 150000, 32, 0, 600000, 4096, (0,)),
           "bnmf_8192_k64_16rows": (8192, 8192, 64, 0, None, 16, (0, 1))}


def problem(I, J, K, L, n_excl, n_rows, seed=0):
    rs = np.random.RandomState(seed)
    A = rs.exponential(1.0, (I, K))
    B = rs.exponential(1.0, (J, L if L else K))
    factors = (A, rs.exponential(1.0, (K, L)), B) if L else (A, B)
    if n_excl is None:
        er, ec = [], []
        for i0 in range(0, I, 1024):
            r, c = np.nonzero(rs.random_sample((min(I, i0 + 1024) - i0, J)) < 0.1)
            er.append((r + i0).astype(np.int32)); ec.append(c.astype(np.int32))
        er, ec = np.concatenate(er), np.concatenate(ec)
        order = rs.permutation(len(er))
        er, ec = np.ascontiguousarray(er[order]), np.ascontiguousarray(ec[order])
    else:
        er, ec = rs.randint(0, I, n_excl).astype(np.int32), rs.randint(0, J, n_excl).astype(np.int32)
    rows = None if n_rows is None else np.sort(rs.permutation(I)[:n_rows]).astype(np.int32)
    return factors, er, ec, rows


def numpy_top(factors, er, ec, rows, n, chunk=256):
    """(cols [r][n], seconds): the clock starts once the exclusion list is sorted by row"""
    A = factors[0] @ factors[1] if len(factors) == 3 else factors[0]
    B = factors[-1]
    sel = np.arange(len(A)) if rows is None else rows
    order = np.argsort(er, kind='stable')
    er, ec = er[order], ec[order]
    ptr = np.searchsorted(er, np.arange(len(A) + 1))
    t0 = time.perf_counter()
    out = np.empty((len(sel), n), dtype=np.int32)
    for q0 in range(0, len(sel), chunk):
        idx = sel[q0:q0 + chunk]
        P = A[idx] @ B.T
        for q, i in enumerate(idx):
            P[q, ec[ptr[i]:ptr[i + 1]]] = -np.inf
        part = np.argpartition(-P, n - 1, axis=1)[:, :n]
        vals = np.take_along_axis(P, part, axis=1)
        keep = np.lexsort((part, -vals), axis=1)
        out[q0:q0 + chunk] = np.take_along_axis(part, keep, axis=1)
    return out, time.perf_counter() - t0


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    import ctypes as C
    from bnmtf_amd import _lib, top_entries
    I, J, K, L, n_excl, n_rows, splits = CONFIGS[a.child]
    factors, er, ec, rows = problem(I, J, K, L, n_excl, n_rows)
    r, W = (I if rows is None else len(rows)), (L if L else K)
    out = {"config": a.child, "I": I, "J": J, "K": K, "L": L, "n": N, "rows": r, "excluded_entries": int(len(er)),
           "multiply_adds": float(r) * J * W, "B_bytes": J * W * 8, "B_bytes_read_by_the_waves": float(r) * J * W * 8, "splits": {}}
    T = None
    for split in splits:
        def call():
            return top_entries.from_factors(factors, N, rows=rows, exclude=(er, ec), split=split)

        call()
        wall, upload, kernel = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            T = call()
            wall.append(time.perf_counter() - t0)
            up, kn = C.c_double(), C.c_double()
            _lib.check(_lib.lib().bnmtf_top_entries_times(C.byref(up), C.byref(kn)))
            upload.append(up.value); kernel.append(kn.value)
        clock = bench._clock_beside(helper, call, lambda: None) if helper is not None else None
        k_s = statistics.median(kernel) * 1e-3
        out["splits"]["library's choice" if split == 0 else str(split)] = {
            "wall_s": [round(t, 4) for t in wall], "wall_s_median": round(statistics.median(wall), 4),
            "upload_ms": [round(t, 3) for t in upload], "kernel_ms": [round(t, 3) for t in kernel],
            "upload_ms_median": round(statistics.median(upload), 3), "kernel_ms_median": round(statistics.median(kernel), 3),
            "fma_per_s": float("%.4g" % (out["multiply_adds"] / k_s)), "B_GB_per_s_read_by_the_waves": round(out["B_bytes_read_by_the_waves"] / k_s / 1e9, 1),
            "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    if not a.no_numpy:
        ref, numpy_s = numpy_top(factors, er, ec, rows, N)
        first = next(iter(out["splits"].values()))
        out.update({"numpy_s": round(numpy_s, 3), "numpy_over_device_wall": round(numpy_s / first["wall_s_median"], 1),
                    "rows_whose_columns_differ_from_numpy": int((ref != T.cols).any(axis=1).sum())})
    print("TOP_ENTRIES_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_entries_rates.json"))
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
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("TOP_ENTRIES_RATES ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit("child failed: %s" % cfg)          # (nothing more is started on the GPU)
        results.append(json.loads(line[0][len("TOP_ENTRIES_RATES "):]))
        print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "bnmtf_amd.top_entries.from_factors(factors, 10, rows, exclude) on exponential fp64 factors: wall time of the call in s "
                               "(host clock, everything included), upload and kernel time in ms from events on the call's stream, fmas/s and the "
                               "bytes/s of B the waves read (r J W 8 bytes over the kernel time: B is read once per row, from the caches), beside "
                               "NumPy fp64 on the same host for the same answer; sclk_mhz: the shader clock (rocm-smi) beside further calls; "
                               "tools/top_entries_rates.py",
                       "configs": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
