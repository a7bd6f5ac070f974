"""Where the observed-entry layout pays for the variational tri-factorisation: iteration rates of bnmtf_vb_optimised (the dense
layout) on the parent commit's build against bnmtf_vb_observed on this build, by the fraction of missing entries.

    python tools/obs_trivb_rates.py --out profiles/obs_trivb_rates.json --parent-lib /path/to/parent/libbnmtf_hip.so

4096 x 4096, K = L = 32 at 50 / 80 / 90 / 95 / 99 % missing, and one size the dense layout cannot hold (16384 x 16384 at 99.5 %
missing: about 1.4 M entries), observed only.  The method is tools/obs_rates.py's: every measurement is a fresh child process
(this one never touches the GPU) that builds the model, warms up, sizes a region from a pilot so that it lasts about `--region`
seconds and times `--repeats` regions of iterations with seeded update orders and null outputs (bnmtf_vb_run / bnmtf_otvb_run);
the children of the two builds alternate, so box and clock are shared.  Reported: every region's it/s, median and range
per build, and the observed fraction at which the two medians cross (log-linear interpolation between the bracketing points), if
they do.  Without --parent-lib the dense class runs on this build (the same code path: bnmtf_vb_optimised is unchanged).
--child CONFIG --layout L --steps N: one child alone, N iterations after the warm-up and nothing else (for a profiler).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from obs_rates import crossover  # noqa: E402

RANK = 32
# name -> (I, J, fraction missing, layouts measured)
CONFIGS = {"4096_m%s" % str(f)[2:]: (4096, 4096, f, ("dense", "observed")) for f in (0.5, 0.8, 0.9, 0.95, 0.99)}
CONFIGS["16384_m995"] = (16384, 16384, 0.995, ("observed",))


def problem(I, J, frac, seed=0):
    """R = F S G^T + noise in fp32 (4 x 4 generating ranks) and a mask with about (1 - frac) of the entries observed, none of its
    rows or columns empty (drawn block by block, as tools/obs_rates.py does)."""
    rs = np.random.RandomState(seed)
    F = rs.exponential(1.0, (I, 4)).astype(np.float32); S = rs.exponential(1.0, (4, 4)).astype(np.float32); G = rs.exponential(1.0, (J, 4)).astype(np.float32)
    R = (F @ S) @ G.T
    M = np.zeros((I, J), dtype=np.float32)
    for i0 in range(0, I, 1024):
        blk = slice(i0, min(I, i0 + 1024))
        R[blk] += rs.standard_normal((blk.stop - blk.start, J)).astype(np.float32)
        M[blk] = rs.random_sample((blk.stop - blk.start, J)) >= frac
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return R, M


def child(a):
    from bnmtf_amd import _lib, bnmtf_vb_observed, bnmtf_vb_optimised
    if a.parent:                    # the parent build has no otvb entry points to bind
        for name in [n for n in _lib._SIGS if "_otvb_" in n]:
            _lib._SIGS.pop(name)
    I, J, frac, _ = CONFIGS[a.child]
    R, M = problem(I, J, frac)
    pri = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
    np.random.seed(0)
    t0 = time.perf_counter()
    model = (bnmtf_vb_observed if a.layout == "observed" else bnmtf_vb_optimised)(R, M, RANK, RANK, pri, verbose=False)
    rs = np.random.RandomState(1)          # (a start of moderate size: the exponential prior's draws at K = L = 32 predict values of 10^5)
    for name, shape in (("F", (I, RANK)), ("S", (RANK, RANK)), ("G", (J, RANK))):
        e = rs.exponential(0.3, shape) + 0.05
        setattr(model, "exp" + name, e); setattr(model, "mu" + name, e.copy())
        setattr(model, "tau" + name, np.ones(shape)); setattr(model, "var" + name, np.full(shape, 0.05))
    model.exptau = 1.0
    model._push()
    create_s = time.perf_counter() - t0
    h, L = model._handle(), _lib.lib()

    ors = np.random.RandomState(2)

    def timed(n):
        od = np.array([np.concatenate([ors.permutation(RANK * RANK), ors.permutation(RANK), ors.permutation(RANK)]) for _ in range(n)], dtype=np.int32)
        t = time.perf_counter()             # (the orders are drawn ahead of the clock: the host's shuffles are not the device's iteration)
        _lib.check((L.bnmtf_otvb_run if a.layout == "observed" else L.bnmtf_vb_run)(h, n, _lib.ptr(od), None, None, None, None))
        _lib.check(L.bnmtf_sync(h))
        return time.perf_counter() - t

    timed(a.warmup)
    if a.steps:                     # (a profiler's run: the iterations and nothing else)
        timed(a.steps)
        print("OBS_TRIVB_STEPS %d" % a.steps, flush=True)
        return
    pilot = timed(10) / 10
    steps = int(min(max(a.region / pilot, 10), 2000))
    rates = []
    for _ in range(a.repeats):
        rates.append(steps / timed(steps))
    n = int(M.sum())
    out = {"config": a.child, "I": I, "J": J, "K": RANK, "L": RANK, "missing": frac, "observed_fraction": n / (float(I) * J), "entries": n,
           "layout": a.layout, "build": "parent" if a.parent else "this", "steps": steps, "create_and_upload_s": round(create_s, 2),
           "it_per_s": [round(r, 2) for r in rates], "median_it_per_s": round(statistics.median(rates), 2), "describe": model.describe()}
    print("OBS_TRIVB_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_trivb_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: the dense class runs on it")
    p.add_argument("--rounds", type=int, default=2, help="children per layout and configuration, the layouts alternating")
    p.add_argument("--region", type=float, default=0.5, help="seconds per timed region")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    p.add_argument("--layout", default="observed", choices=("dense", "observed"))
    p.add_argument("--parent", action="store_true", help="(child) the library loaded is the parent build")
    p.add_argument("--steps", type=int, default=0, help="(child) run this many iterations after the warm-up and stop")
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in a.configs.split(","):
        for _ in range(a.rounds):
            for layout in CONFIGS[cfg][3]:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--layout", layout, "--region", str(a.region),
                       "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                env = dict(os.environ)
                env.pop("BNMTF_LIB", None)
                if layout == "dense" and a.parent_lib:
                    cmd.append("--parent"); env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = [l for l in r.stdout.splitlines() if l.startswith("OBS_TRIVB_RATES ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit("child failed: %s (%s)" % (cfg, layout))          # (nothing more is started on the GPU)
                results.append(json.loads(line[0][len("OBS_TRIVB_RATES "):]))
                print(line[0], flush=True)
    summary, points = {}, []
    for cfg in a.configs.split(","):
        s = {"missing": CONFIGS[cfg][2]}
        for layout in CONFIGS[cfg][3]:
            rs = [x for r in results if r["config"] == cfg and r["layout"] == layout for x in r["it_per_s"]]
            rr = [r for r in results if r["config"] == cfg and r["layout"] == layout]
            s[layout] = {"build": rr[0]["build"], "median_it_per_s": round(statistics.median(rs), 2), "range_it_per_s": [min(rs), max(rs)]}
            s["observed_fraction"] = rr[0]["observed_fraction"]; s["entries"] = rr[0]["entries"]
        if "dense" in s and "observed" in s:
            s["observed_over_dense"] = round(s["observed"]["median_it_per_s"] / s["dense"]["median_it_per_s"], 3)
            if CONFIGS[cfg][0] == 4096:
                points.append((s["observed_fraction"], s["dense"]["median_it_per_s"], s["observed"]["median_it_per_s"]))
        summary[cfg] = s
    cross = crossover(points) if len(points) > 1 else None
    summary["crossover_observed_fraction_4096_k32_l32"] = cross if cross is None else round(cross, 4)
    with open(a.out, "w") as f:
        json.dump({"what": "BNMTF VB iteration rates (seeded update orders, null outputs), K = L = 32: bnmtf_vb_optimised (dense) on the parent "
                           "build against bnmtf_vb_observed on this build, same box, fresh child processes alternating; tools/obs_trivb_rates.py",
                   "summary": summary, "children": results}, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
