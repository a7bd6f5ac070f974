#!/usr/bin/env python3
"""What the held-out curves of the non-probabilistic models and of run_many(M_tests=) cost, and that nothing got slower without
them: this build against another build of the library (the parent commit's), same box, processes alternating.

    python tools/heldout_many_rates.py --out profiles/heldout_many_rates.json [--parent-lib /path/to/parent/libbnmtf_hip.so] [--rounds 3]

Every measurement is a fresh child process (this one never touches the GPU); a round runs every job with the parent build, then
with this one.  Jobs:

    nmf_4096      NMF 4096 x 4096, K = 32, 10 % unobserved: device seconds per iteration of run(steps), without a mask and (this build)
                  with the 10 % complement as the mask; the shader clock is read beside the loop (bench.py's rocm-smi helper)
    np_grid       the batched NMTF grid on the GDSC matrix: K, L in {2, 4, 6, 8, 10} x 5 folds = 125 models in one run_many call,
                  without M_tests and (this build) with every model's fold as its mask
    vb_grid       40 bnmf_vb_optimised models of GDSC's shape (10 folds x K in {15, 20, 25, 30}) in one run_many call, likewise
    cv_gdsc_vb    bench.py --workload cv_gdsc_vb --cv-batched (no masks: the cross-validation drivers score a fold with predict())

    python tools/heldout_many_rates.py --child nmf_4096 --mask --no-clock      # one region with the mask, e.g. under rocprofv3
"""
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
JOBS = ("nmf_4096", "np_grid", "vb_grid", "cv_gdsc_vb")


def folds_of(M, n, seed):
    """n disjoint held-out masks that partition the observed entries of M"""
    rs = np.random.RandomState(seed)
    i, j = np.nonzero(M)
    part = rs.permutation(len(i)) % n
    out = []
    for f in range(n):
        Mt = np.zeros(M.shape); Mt[i[part == f], j[part == f]] = 1
        out.append(Mt)
    return out


def trainable(M, Mt):
    """M without the fold, every row and column still observed somewhere"""
    Mf = M * (1 - Mt)
    for ax in (0, 1):
        for e in np.nonzero(Mf.sum(axis=1 - ax) == 0)[0]:
            idx = (e, np.nonzero(M[e])[0][0]) if ax == 0 else (np.nonzero(M[:, e])[0][0], e)
            Mf[idx] = 1
    return Mf


def child_nmf(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    from bnmtf_amd import NMF
    rs = np.random.RandomState(0)
    I = 4096
    R = rs.rand(I, I) * 4 + 0.5
    M = (rs.rand(I, I) < 0.9).astype(float); M[:, 0] = 1; M[0, :] = 1
    np.random.seed(0)
    m = NMF(R, M, 32, verbose=False); m.initialise("random")
    m.run(3)
    out = {"job": "nmf_4096", "steps": a.steps, "held_out_entries": int((1 - M).sum())}
    regions = {"plain": None} if a.parent else ({"mask": 1 - M} if a.mask else {"plain": None, "mask": 1 - M})
    for _ in range(a.repeats):
        for name, Mt in regions.items():
            if Mt is None:
                m.run(a.steps)
            else:
                m.run(a.steps, M_test=Mt)
            out.setdefault(name + "_ms_per_it", []).append(1e3 * m.all_times[-1] / a.steps)
    if helper is not None:
        from bnmtf_amd import _lib
        out["clock"] = bench._clock_beside(helper, lambda: m.run(5), lambda: _lib.check(_lib.lib().bnmtf_sync(m._handle())))
    print(json.dumps(out), flush=True)


def child_grid(a):
    import bnmtf_amd
    from bnmtf_amd import NMTF, bnmf_vb_optimised
    if a.child == "np_grid":
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from np_many_rates import gdsc
        X, M = gdsc()
        nf, settings = 5, [(K, L) for K in (2, 4, 6, 8, 10) for L in (2, 4, 6, 8, 10)]
    else:
        import bench
        X, M = bench._small_problem(bench.WORKLOADS["cv_gdsc_vb"])
        X, M = np.asarray(X, dtype=float), np.asarray(M, dtype=float)
        nf, settings = 10, [(K,) for K in (15, 20, 25, 30)]
    folds = folds_of(M, nf, 1)

    def models():
        np.random.seed(0)
        ms, masks = [], []
        for s in settings:
            for Mt in folds:
                if a.child == "np_grid":
                    b = NMTF(X, trainable(M, Mt), s[0], s[1], verbose=False); b.initialise("random", "random")
                else:
                    b = bnmf_vb_optimised(X, trainable(M, Mt), s[0], dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1), verbose=False); b.initialise("random")
                ms.append(b); masks.append(Mt)
        return ms, masks

    out = {"job": a.child, "steps": a.steps}
    for name in (("plain",) if a.parent else ("plain", "mask")):
        ms, masks = models()
        kw = {"M_tests": masks} if name == "mask" else {}
        bnmtf_amd.run_many(ms, 2, **kw)                               # (library, kernels, the models' handles and states)
        for _ in range(a.repeats):
            t0 = time.perf_counter(); bnmtf_amd.run_many(ms, a.steps, **kw); dt = time.perf_counter() - t0
            out.setdefault(name + "_wall_s", []).append(dt)
            out.setdefault(name + "_device_call_s", []).append(ms[0]._many_info[2])
        out["models"] = len(ms); out["shared"] = ms[0]._many_info[0]
        for b in ms:
            b.close()
    print(json.dumps(out), flush=True)


def run_child(job, lib, parent, a):
    env = dict(os.environ)
    if lib:
        env["BNMTF_LIB"] = lib
    if job == "cv_gdsc_vb":
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cv_gdsc_vb", "--cv-batched", "--no-cpu-baseline", "--no-clock"]
    else:
        steps = {"nmf_4096": 40, "np_grid": 100, "vb_grid": 300}[job]
        cmd = [sys.executable, os.path.abspath(__file__), "--child", job, "--steps", str(steps), "--repeats", "3"] + (["--parent"] if parent else [])
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit("%s (%s) failed with %d:\n%s" % (job, "parent" if parent else "this build", p.returncode, p.stderr[-2000:]))
    d = json.loads(p.stdout.strip().splitlines()[-1])
    if job == "cv_gdsc_vb":
        d = {"job": job, "seconds_by_slots": {s: r["seconds"] for s, r in d["by_slots"].items()}}
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", choices=JOBS[:3])
    ap.add_argument("--parent", action="store_true", help="child: the library is the parent build (no M_test)")
    ap.add_argument("--mask", action="store_true", help="child nmf_4096: regions with the mask only")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-clock", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child_nmf(a) if a.child == "nmf_4096" else child_grid(a)
    rows = []
    for r in range(a.rounds):
        for parent in ([True, False] if a.parent_lib else [False]):
            for job in JOBS:
                d = run_child(job, a.parent_lib if parent else None, parent, a)
                d.update(build="parent" if parent else "this", round=r)
                print(json.dumps(d), flush=True)
                rows.append(d)

    def series(job, build, key):
        v = []
        for d in rows:
            if d["job"] == job and d["build"] == build:
                x = d.get(key)
                v += list(x.values())[-1:] if isinstance(x, dict) else (x or [])
        return v

    summary = {}
    for job, key in (("nmf_4096", "plain_ms_per_it"), ("np_grid", "plain_device_call_s"), ("vb_grid", "plain_device_call_s"), ("cv_gdsc_vb", "seconds_by_slots")):
        s = {}
        for build in ("parent", "this"):
            v = series(job, build, key)
            if v:
                s[build] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
        summary[job] = {"what": key + (" (four slots)" if job == "cv_gdsc_vb" else ""), **s}
    for job, key, per in (("nmf_4096", "ms_per_it", None), ("np_grid", "device_call_s", 125 * 100), ("vb_grid", "device_call_s", 40 * 300)):
        plain, mask = series(job, "this", "plain_" + key), series(job, "this", "mask_" + key)
        if plain and mask:
            d = statistics.median(mask) - statistics.median(plain)
            summary[job]["with_masks"] = {"median": statistics.median(mask), "extra": d,
                                          "extra_us_per_model_iteration" if per else "extra_ms_per_iteration": 1e6 * d / per if per else d}
    out = {"what": "run_many(M_tests=) and NMF/NMTF run(M_test=): this build against the parent build without masks, and the cost of the curves; "
                   "same box, fresh processes alternating parent / this build, %d rounds" % a.rounds,
           "summary": summary, "runs": rows}
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
