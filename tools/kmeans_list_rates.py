"""Where the list forms of the masked K-means pay: the dense KMeans on the parent commit's build against KMeans(layout='observed')
on this build, by the fraction of missing entries.

    python tools/kmeans_list_rates.py --out profiles/kmeans_list_rates.json --parent-lib /path/to/parent/libbnmtf_hip.so

At 4096 x 4096, K = 32, at 50 / 80 / 90 / 99 % missing: the time of one bnmtf_kmeans_assign call and of one bnmtf_kmeans_sums call
(host clock around the call: both end in a device-to-host copy, and the list form's host-side transposition of the centroids is part
of its call), and the wall time of initialise('random', 'kmeans') of bnmtf_gibbs_optimised(layout='observed'), K = L = 32 -- both
clusterings, host code included.  At 16384 x 16384 with about 1.37 M entries (99.49 % missing): the two calls on both forms and the
device bytes of both handles, computed from their allocations (the model-level initialise is left out there: the reference's
tolist() count of the unique points, which an empty cluster asks for, takes minutes and tens of GiB of host memory at that size
on either form).

Every measurement is a fresh child process (this one never touches the GPU); the children of the two builds alternate, so box and
clock are shared.  A child builds the problem, creates the handle, calls each entry point `--warmup` times and then `--repeats`
times, and, where the configuration says so, times one initialise.  On the parent build the model hands KMeans no layout -- what the
parent's classes do.  Reported: every call's time, median and range per build, the iterations the clusterings took and a checksum of
the initial F and G (equal on both builds: the same bits); per measure the observed fraction at which the two medians cross
(log-linear interpolation between the bracketing points; null when they do not cross within the range measured).  The file is
rewritten after every configuration.  Without --parent-lib the dense form runs on this build (the same code path: 'dense' is
unchanged).
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (points = coordinates, K, fraction missing, time the model's initialise)
CONFIGS = {"k32_4096_m%s" % str(f)[2:]: (4096, 32, f, True) for f in (0.5, 0.8, 0.9, 0.99)}
CONFIGS["k32_16384_m9949"] = (16384, 32, 0.9949, False)
MEASURES = ("assign_ms", "sums_ms", "initialise_s")


def problem(I, J, K, frac, seed=0):
    """Positive R = U V^T (0.8 + 0.4 rand) in fp32 and a mask with about (1 - frac) of the entries observed, none of its rows or
    columns empty (drawn block by block)."""
    rs = np.random.RandomState(seed)
    U = rs.exponential(1.0, (I, K)).astype(np.float32); V = rs.exponential(1.0, (J, K)).astype(np.float32)
    R = U @ V.T
    M = np.zeros((I, J), dtype=np.float32)
    for i0 in range(0, I, 1024):
        blk = slice(i0, min(I, i0 + 1024))
        R[blk] *= (0.8 + 0.4 * rs.random_sample((blk.stop - blk.start, J))).astype(np.float32)
        M[blk] = rs.random_sample((blk.stop - blk.start, J)) >= frac
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return R, M


def device_bytes(layout, n, d, K, entries):
    """what the handle allocates on the device (csrc/kernel_kmeans.hip: bnmtf_kmeans_create / bnmtf_kmeans_create_list)"""
    shared = 12 * n + 16 * K * d                             # assign, dist; cnt, tot
    if layout == "dense":
        return 9 * n * d + 9 * K * d + shared                # X fp64 and M bytes; centroids and their masks
    KP = (K + 7) // 8 * 8
    return 28 * entries + 4 * (n + 1) + 4 * (d + 1) + 9 * KP * d + 8 * d + shared     # two lists and the permutation, pointers; transposed centroids; set_row's row


def child(a):
    from bnmtf_amd import _lib, bnmtf_gibbs_optimised
    from bnmtf_amd.kmeans import KMeans
    import ctypes as C
    layout = "dense" if a.parent or a.layout == "dense" else "observed"
    if a.parent:                    # the parent build has no list entry points to bind
        for name in ("bnmtf_kmeans_create_list", "bnmtf_kmeans_build_lists"):
            _lib._SIGS.pop(name)
    if layout == "dense":           # the model classes hand KMeans no layout, as the parent's do
        init = KMeans.__init__
        KMeans.__init__ = lambda self, *args, layout='dense', **kw: init(self, *args, layout='dense', **kw)
    iterations = []
    cluster = KMeans.cluster

    def counted(self):
        cluster(self)
        iterations.append(len(self.assign_hist))
    KMeans.cluster = counted

    n, K, frac, with_model = CONFIGS[a.child]
    R, M = problem(n, n, K, frac)
    entries = int(M.sum())
    lib = _lib.lib()
    km = KMeans(R, M, K, layout=layout)
    random.seed(0)
    km.initialise()
    t0 = time.perf_counter()
    h = km._device_handle()
    create_s = time.perf_counter() - t0
    Cm = np.ascontiguousarray(np.array(km.centroids)); Mc8 = np.ascontiguousarray(km.mask_centroids != 0, dtype=np.uint8)
    new = np.zeros(km.no_points, dtype=np.int32); dist = np.zeros(km.no_points)
    cnt = np.zeros((K, km.no_coordinates)); tot = np.zeros((K, km.no_coordinates))

    def timed(call, *args):
        for _ in range(a.warmup):
            _lib.check(call(h, *args))
        out = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            _lib.check(call(h, *args))
            out.append((time.perf_counter() - t) * 1e3)
        return out

    assign_ms = timed(lib.bnmtf_kmeans_assign, _lib.ptr(Cm), _lib.ptr(Mc8), _lib.ptr(new), _lib.ptr(dist))
    sums_ms = timed(lib.bnmtf_kmeans_sums, _lib.ptr(new), _lib.ptr(cnt), _lib.ptr(tot))
    checks = {"assign_crc": zlib.crc32(new.tobytes()), "dist_crc": zlib.crc32(dist.tobytes()), "cnt_crc": zlib.crc32(cnt.tobytes()),
              "tot_crc": zlib.crc32(tot.tobytes())}
    km.close()
    out = {"config": a.child, "points": n, "coordinates": n, "K": K, "missing": frac, "observed_fraction": entries / (float(n) * n),
           "entries": entries, "layout": layout, "build": "parent" if a.parent else "this", "create_s": round(create_s, 3),
           "assign_ms": [round(t, 3) for t in assign_ms], "sums_ms": [round(t, 3) for t in sums_ms],
           "device_bytes": device_bytes(layout, km.no_points, km.no_coordinates, K, entries), "checks": checks}
    if with_model:
        pri = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
        m = bnmtf_gibbs_optimised(R, M, K, K, pri, seed=1, verbose=False, layout='observed')
        random.seed(0); np.random.seed(0)
        del iterations[:]
        t0 = time.perf_counter()
        m.initialise('random', 'kmeans')
        out["initialise_s"] = [round(time.perf_counter() - t0, 3)]
        out["kmeans_iterations"] = list(iterations)
        out["checks"]["F_crc"] = zlib.crc32(np.ascontiguousarray(m.F).tobytes()); out["checks"]["G_crc"] = zlib.crc32(np.ascontiguousarray(m.G).tobytes())
    print("KMEANS_LIST_RATES " + json.dumps(out), flush=True)


def crossover(points):
    """points: (observed fraction, dense time, list time), any order.  The observed fraction at which the two times are equal,
    interpolated in (log fraction, log ratio) between the two points that bracket it; None if they do not cross in the range."""
    pts = sorted(points)
    for (f0, d0, o0), (f1, d1, o1) in zip(pts, pts[1:]):
        r0, r1 = np.log(o0 / d0), np.log(o1 / d1)
        if r0 == 0:
            return f0
        if r0 * r1 < 0:
            return float(np.exp(np.log(f0) + (np.log(f1) - np.log(f0)) * r0 / (r0 - r1)))
    return None


def summarise(configs, results):
    summary, points = {}, {m: [] for m in MEASURES}
    for cfg in configs:
        rr_all = [r for r in results if r["config"] == cfg]
        if not rr_all:
            continue
        s = {"missing": CONFIGS[cfg][2], "observed_fraction": rr_all[0]["observed_fraction"], "entries": rr_all[0]["entries"]}
        for layout in ("dense", "observed"):
            rr = [r for r in rr_all if r["layout"] == layout]
            if not rr:
                continue
            s[layout] = {"build": rr[0]["build"], "device_bytes": rr[0]["device_bytes"], "runs": len(rr)}
            for m in MEASURES:
                ts = [x for r in rr for x in r.get(m, [])]
                if ts:
                    s[layout][m] = {"median": round(statistics.median(ts), 3), "range": [min(ts), max(ts)]}
            if "kmeans_iterations" in rr[0]:
                s[layout]["kmeans_iterations"] = rr[0]["kmeans_iterations"]
        if "dense" in s and "observed" in s:
            both = [r["checks"] for r in rr_all]
            s["same_results_on_both_builds"] = all(c == both[0] for c in both)
            for m in MEASURES:
                if m in s["dense"] and m in s["observed"]:
                    s["dense_over_list_" + m] = round(s["dense"][m]["median"] / s["observed"][m]["median"], 3)
                    if CONFIGS[cfg][0] == 4096:
                        points[m].append((s["observed_fraction"], s["dense"][m]["median"], s["observed"][m]["median"]))
        summary[cfg] = s
    for m, pts in points.items():
        cross = crossover(pts) if len(pts) > 1 else None
        summary["crossover_observed_fraction_%s_4096" % m] = cross if cross is None else round(cross, 4)
    return summary


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_list_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: the dense form runs on it")
    p.add_argument("--rounds", type=int, default=3, help="children per form and configuration, the forms alternating")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    p.add_argument("--layout", default="observed", choices=("dense", "observed"))
    p.add_argument("--parent", action="store_true", help="(child) the library loaded is the parent build")
    a = p.parse_args()
    if a.child:
        return child(a)
    results, configs = [], a.configs.split(",")
    for cfg in configs:
        for _ in range(a.rounds):
            for layout in ("dense", "observed"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--layout", layout, "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                env = dict(os.environ)
                env.pop("BNMTF_LIB", None)
                if layout == "dense" and a.parent_lib:
                    cmd.append("--parent"); env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = [l for l in r.stdout.splitlines() if l.startswith("KMEANS_LIST_RATES ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit("child failed: %s (%s)" % (cfg, layout))          # (nothing more is started on the GPU)
                results.append(json.loads(line[0][len("KMEANS_LIST_RATES "):]))
                print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "masked K-means: the dense form on the parent build against the list form (layout='observed') on this build, same box, "
                               "fresh child processes alternating; call times in ms (host clock around a synchronous call), initialise('random', "
                               "'kmeans') of bnmtf_gibbs_optimised(layout='observed') in s; tools/kmeans_list_rates.py",
                       "summary": summarise(configs, results), "children": results}, f, indent=1)
            f.write("\n")
    print(json.dumps(summarise(configs, results), indent=1))


if __name__ == "__main__":
    main()
