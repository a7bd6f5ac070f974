"""Where the observed-entry layout pays for the non-probabilistic models: iteration rates of nmf_np.NMF and nmtf_np.NMTF with
layout='dense' on the parent commit's build against layout='observed' on this build, by the fraction of missing entries.

    python tools/obs_np_rates.py --out profiles/obs_np_rates.json --parent-lib /path/to/parent/libbnmtf_hip.so

NMF at 4096 x 4096, K = 32, at 50 / 80 / 90 / 99 % missing; NMTF at 4096 x 4096, K = L = 32, at 90 / 99 % missing; and both at
16384 x 16384 with about 1.37 M entries (99.49 % missing), observed only: the dense layout caps rows and columns at 16 384 entries
and would hold R twice, the mask and NMTF's P at 1 GiB each.  Every measurement is a fresh child process (this one never touches
the GPU): it builds the model, warms up, sizes a region from a pilot so that it lasts about `--region` seconds and times
`--repeats` regions of iterations through the C entry point with null outputs (bnmf_np_run / bnmtf_np_run / bnmtf_onp_run), then
reads the shader clock beside one more region (bench.py's helper).  The children of the two builds alternate, so box and clock are
shared.  Reported: every region's it/s, median and range per build, the shader clock; the observed fraction at which the two
medians cross (log-linear interpolation between the bracketing points; null when they do not cross within the range measured); and
for the observed NMF the bytes its gathers ask for per iteration over the measured time, as tools/obs_rates.py reports them.  The
file is rewritten after every configuration.  Without --parent-lib the dense layout runs on this build (the same code path: 'dense'
is unchanged).
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
# name -> (I, J, K, L (0: NMF), fraction missing, layouts measured)
CONFIGS = {"nmf_4096_m%s" % str(f)[2:]: (4096, 4096, 32, 0, f, ("dense", "observed")) for f in (0.5, 0.8, 0.9, 0.99)}
CONFIGS.update({"nmtf_4096_m%s" % str(f)[2:]: (4096, 4096, 32, 32, f, ("dense", "observed")) for f in (0.9, 0.99)})
CONFIGS["nmf_16384_m9949"] = (16384, 16384, 32, 0, 0.9949, ("observed",))
CONFIGS["nmtf_16384_m9949"] = (16384, 16384, 32, 32, 0.9949, ("observed",))


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


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    from bnmtf_amd import NMF, NMTF, _lib
    if a.parent:                    # the parent build has no onp entry points to bind
        for name in [n for n in _lib._SIGS if "_onp_" in n]:
            _lib._SIGS.pop(name)
    I, J, K, L, frac, _ = CONFIGS[a.child]
    R, M = problem(I, J, K, frac)
    kw = {} if a.parent else {"layout": a.layout}
    np.random.seed(0)
    t0 = time.perf_counter()
    if L:
        model = NMTF(R, M, K, L, verbose=False, **kw)
        model.initialise("random", "random")
    else:
        model = NMF(R, M, K, verbose=False, **kw)
        model.initialise("random")
    model._push()
    create_s = time.perf_counter() - t0
    h, lib = model._handle(), _lib.lib()
    fn = lib.bnmtf_onp_run if a.layout == "observed" else (lib.bnmtf_np_run if L else lib.bnmf_np_run)

    def run(n):
        _lib.check(fn(h, n, None, None, None))

    def sync():
        _lib.check(lib.bnmtf_sync(h))

    def timed(n):
        t = time.perf_counter()
        run(n); sync()
        return time.perf_counter() - t

    timed(a.warmup)
    pilot = timed(5) / 5
    steps = int(min(max(a.region / pilot, 5), 2000))
    rates = [steps / timed(steps) for _ in range(a.repeats)]
    clock = bench._clock_beside(helper, lambda: run(steps), sync) if helper is not None else None
    n = int(M.sum())
    out = {"config": a.child, "model": "nmtf" if L else "nmf", "I": I, "J": J, "K": K, "L": L, "missing": frac,
           "observed_fraction": n / (float(I) * J), "entries": n, "layout": a.layout, "build": "parent" if a.parent else "this",
           "steps": steps, "create_and_upload_s": round(create_s, 2), "it_per_s": [round(r, 2) for r in rates],
           "median_it_per_s": round(statistics.median(rates), 2), "sclk_mhz": clock["sclk_mhz_median"] if clock else None}
    if a.layout == "observed":
        out["describe"] = model.describe() if hasattr(model, "describe") else None
        if not L:
            KP = (K + 3) // 4 * 4
            gathered = 2.0 * n * (KP * 4 + K * 4 + 8)        # per iteration: both half sweeps; the other factor's row, one element per column, index and value
            out["gather_bytes_per_iteration"] = gathered
            out["gathered_TB_per_s"] = round(gathered * statistics.median(rates) / 1e12, 3)
    print("OBS_NP_RATES " + json.dumps(out), flush=True)


def crossover(points):
    """points: (observed fraction, dense it/s, observed it/s), any order.  The observed fraction at which the two rates are equal,
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
    summary, points = {}, {"nmf": [], "nmtf": []}
    for cfg in configs:
        rr_all = [r for r in results if r["config"] == cfg]
        if not rr_all:
            continue
        s = {"missing": CONFIGS[cfg][4], "observed_fraction": rr_all[0]["observed_fraction"], "entries": rr_all[0]["entries"]}
        for layout in CONFIGS[cfg][5]:
            rr = [r for r in rr_all if r["layout"] == layout]
            if not rr:
                continue
            rs = [x for r in rr for x in r["it_per_s"]]
            clocks = [r["sclk_mhz"] for r in rr if r["sclk_mhz"] is not None]
            s[layout] = {"build": rr[0]["build"], "median_it_per_s": round(statistics.median(rs), 2), "range_it_per_s": [min(rs), max(rs)],
                         "sclk_mhz": statistics.median(clocks) if clocks else None}
            if "gather_bytes_per_iteration" in rr[0]:
                s[layout]["gathered_TB_per_s"] = round(rr[0]["gather_bytes_per_iteration"] * s[layout]["median_it_per_s"] / 1e12, 3)
        if "dense" in s and "observed" in s:
            s["observed_over_dense"] = round(s["observed"]["median_it_per_s"] / s["dense"]["median_it_per_s"], 3)
            if CONFIGS[cfg][0] == 4096:
                points[rr_all[0]["model"]].append((s["observed_fraction"], s["dense"]["median_it_per_s"], s["observed"]["median_it_per_s"]))
        summary[cfg] = s
    for model, pts in points.items():
        cross = crossover(pts) if len(pts) > 1 else None
        summary["crossover_observed_fraction_%s_4096" % model] = cross if cross is None else round(cross, 4)
    return summary


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_np_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: the dense layout runs on it")
    p.add_argument("--rounds", type=int, default=2, help="children per layout and configuration, the layouts alternating")
    p.add_argument("--region", type=float, default=0.5, help="seconds per timed region")
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    p.add_argument("--layout", default="observed", choices=("dense", "observed"))
    p.add_argument("--parent", action="store_true", help="(child) the library loaded is the parent build")
    p.add_argument("--no-clock", action="store_true")
    a = p.parse_args()
    if a.child:
        return child(a)
    results, configs = [], a.configs.split(",")
    for cfg in configs:
        for _ in range(a.rounds):
            for layout in CONFIGS[cfg][5]:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--layout", layout, "--region", str(a.region),
                       "--warmup", str(a.warmup), "--repeats", str(a.repeats)] + (["--no-clock"] if a.no_clock else [])
                env = dict(os.environ)
                env.pop("BNMTF_LIB", None)
                if layout == "dense" and a.parent_lib:
                    cmd.append("--parent"); env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                line = [l for l in r.stdout.splitlines() if l.startswith("OBS_NP_RATES ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit("child failed: %s (%s)" % (cfg, layout))          # (nothing more is started on the GPU)
                results.append(json.loads(line[0][len("OBS_NP_RATES "):]))
                print(line[0], flush=True)
        with open(a.out, "w") as f:
            json.dump({"what": "NMF / NMTF iteration rates (multiplicative updates, null outputs): layout='dense' on the parent build against "
                               "layout='observed' on this build, same box, fresh child processes alternating; tools/obs_np_rates.py",
                       "summary": summarise(configs, results), "children": results}, f, indent=1)
            f.write("\n")
    print(json.dumps(summarise(configs, results), indent=1))


if __name__ == "__main__":
    main()
