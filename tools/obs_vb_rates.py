"""Where the observed-entry layout pays for the variational model: iteration rates of bnmf_vb_optimised on the parent commit's
build against bnmf_vb_observed on this build, by the fraction of missing entries.

    python tools/obs_vb_rates.py --out profiles/obs_vb_rates.json --parent-lib /path/to/parent/libbnmtf_hip.so

4096 x 4096, K = 32 at 50 / 80 / 90 / 95 / 99 % missing, and 16384 x 16384 at 99.5 % missing (1.3 M entries; the dense class would
hold several 1 GiB copies of the matrix), observed only.  tools/obs_rates.py's method and its problems: every measurement is a
fresh child process (this one never touches the GPU) that builds the model, initialises it ('random', NumPy seed 0), warms up,
sizes a region from a pilot so that it lasts about `--region` seconds and times `--repeats` regions of iterations through the C
entry point with null outputs (bnmf_vb_run / bnmf_vbo_run).  The children of the two builds alternate, so box and clock are
shared.  Reported: every region's it/s, median and range per class, and the observed fraction at which the two medians cross
(None: they do not cross in the measured range).  Without --parent-lib the dense class runs on this build (its kernels are
unchanged)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from obs_rates import crossover, problem  # noqa: E402

# name -> (I, J, K, fraction missing, classes measured)
CONFIGS = {"4096_m%s" % str(f)[2:]: (4096, 4096, 32, f, ("dense", "observed")) for f in (0.5, 0.8, 0.9, 0.95, 0.99)}
CONFIGS["16384_m995"] = (16384, 16384, 32, 0.995, ("observed",))


def child(a):
    from bnmtf_amd import _lib
    if a.parent:                    # the parent build has no bnmf_vbo_* entry points to bind
        for name in [n for n in _lib._SIGS if "_vbo_" in n]:
            _lib._SIGS.pop(name)
    from bnmtf_amd import bnmf_vb_observed, bnmf_vb_optimised
    I, J, K, frac, _ = CONFIGS[a.child]
    R, M = problem(I, J, K, frac)
    pri = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
    np.random.seed(0)
    t0 = time.perf_counter()
    model = (bnmf_vb_observed if a.layout == "observed" else bnmf_vb_optimised)(R, M, K, pri, verbose=False)
    model.initialise("random")
    model._push()
    create_s = time.perf_counter() - t0
    h, L = model._handle(), _lib.lib()
    entry = L.bnmf_vbo_run if a.layout == "observed" else L.bnmf_vb_run

    def timed(n):
        t = time.perf_counter()
        _lib.check(entry(h, n, None, None, None, None)); _lib.check(L.bnmtf_sync(h))
        return time.perf_counter() - t

    timed(a.warmup)
    pilot = timed(10) / 10
    steps = int(min(max(a.region / pilot, 10), 2000))
    rates = []
    for _ in range(a.repeats):
        rates.append(steps / timed(steps))
    n = int(M.sum())
    out = {"config": a.child, "I": I, "J": J, "K": K, "missing": frac, "observed_fraction": n / (float(I) * J), "entries": n,
           "layout": a.layout, "build": "parent" if a.parent else "this", "steps": steps, "create_and_upload_s": round(create_s, 2),
           "it_per_s": [round(r, 2) for r in rates], "median_it_per_s": round(statistics.median(rates), 2), "describe": model.describe()}
    print("OBS_VB_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_vb_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: the dense class runs on it")
    p.add_argument("--rounds", type=int, default=2, help="children per class and configuration, the classes alternating")
    p.add_argument("--region", type=float, default=0.5, help="seconds per timed region")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    p.add_argument("--layout", default="observed", choices=("dense", "observed"))
    p.add_argument("--parent", action="store_true", help="(child) the library loaded is the parent build")
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in a.configs.split(","):
        for _ in range(a.rounds):
            for layout in CONFIGS[cfg][4]:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--layout", layout, "--region", str(a.region),
                       "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                env = dict(os.environ)
                env.pop("BNMTF_LIB", None)
                if layout == "dense" and a.parent_lib:
                    cmd.append("--parent"); env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                line = [l for l in r.stdout.splitlines() if l.startswith("OBS_VB_RATES ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit("child failed: %s (%s)" % (cfg, layout))          # (nothing more is started on the GPU)
                results.append(json.loads(line[0][len("OBS_VB_RATES "):]))
                print(line[0], flush=True)
    summary, points = {}, []
    for cfg in a.configs.split(","):
        s = {"missing": CONFIGS[cfg][3]}
        for layout in CONFIGS[cfg][4]:
            rs = [x for r in results if r["config"] == cfg and r["layout"] == layout for x in r["it_per_s"]]
            rr = [r for r in results if r["config"] == cfg and r["layout"] == layout]
            s[layout] = {"build": rr[0]["build"], "median_it_per_s": round(statistics.median(rs), 2), "range_it_per_s": [min(rs), max(rs)]}
            s["observed_fraction"] = rr[0]["observed_fraction"]; s["entries"] = rr[0]["entries"]
        if "dense" in s and "observed" in s:
            s["observed_over_dense"] = round(s["observed"]["median_it_per_s"] / s["dense"]["median_it_per_s"], 3)
            points.append((s["observed_fraction"], s["dense"]["median_it_per_s"], s["observed"]["median_it_per_s"]))
        summary[cfg] = s
    cross = crossover(points) if len(points) > 1 else None
    summary["crossover_observed_fraction_4096_k32"] = cross if cross is None else round(cross, 4)
    with open(a.out, "w") as f:
        json.dump({"what": "variational iteration rates: bnmf_vb_optimised on the parent build against bnmf_vb_observed on this build, "
                           "same box, fresh child processes alternating; tools/obs_vb_rates.py", "summary": summary, "children": results}, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
