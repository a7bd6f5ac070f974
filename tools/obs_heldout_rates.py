"""What a held-out curve costs on the observed-entry layout, and what list input saves on the host.

    python tools/obs_heldout_rates.py --out profiles/obs_heldout_rates.json --parent-lib /path/to/parent/libbnmtf_hip.so

Rates: iterations per second of bnmf_gibbs_optimised(layout='observed') -- Gibbs draws without the sample hand-off, bnmf_obs_run
with null outputs -- without a held-out list on the parent commit's build and on this build (no launch is added: expected equal
within box noise), and with a held-out list of 1.68 M entries on this build; at 4096 x 4096, K = 32, 90 % missing (the size behind
the dense layout's "about 42 us per iteration") and at K = 256, 99 % missing.  The models are built from
Entries.  Every measurement is a fresh child process (this one never touches the GPU): it builds the model, warms up, sizes a
region from a pilot so that it lasts about `--region` seconds and times `--repeats` regions; the children of the three kinds
alternate, so box and clock are shared.  Reported: every region's it/s, median and range per kind, and the curve's cost per
iteration, 1 / with - 1 / without on this build, beside the time of an iteration without it (two half sweeps and the finish).

Construction (tools/create_overheads.py's method: one fresh process per measurement, wall time around constructor + handle, the
process's peak resident set): the 16 384 x 16 384 model with about 1.4 M entries from dense fp64 arrays against from an Entries.
"""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (I, J, K, fraction missing, held-out entries)
CONFIGS = {"4096_k32_m90": (4096, 4096, 32, 0.90, 1680000), "4096_k256_m99": (4096, 4096, 256, 0.99, 1680000)}
KINDS = ("parent_without", "without", "with")
CREATE = (16384, 16384, 32, 1400000)


def entries(I, J, n, seed):
    """About n entries of an I x J matrix, a cyclic diagonal among them (no empty row or column), with non-negative values."""
    from bnmtf_amd import Entries
    rs = np.random.RandomState(seed)
    d = np.arange(max(I, J), dtype=np.int64)
    flat = np.unique(np.concatenate([(d % I) * J + d % J, rs.randint(0, I, n).astype(np.int64) * J + rs.randint(0, J, n)]))
    return Entries((I, J), flat // J, flat % J, rs.exponential(1.0, len(flat)))


def child_rate(a):
    from bnmtf_amd import _lib, bnmf_gibbs_optimised
    if a.kind == "parent_without":           # the parent build has no such entry point to bind
        _lib._SIGS.pop("bnmtf_set_heldout_entries")
    I, J, K, frac, n_held = CONFIGS[a.child]
    E = entries(I, J, int((1.0 - frac) * I * J), 0)
    np.random.seed(0)
    model = bnmf_gibbs_optimised(E, None, K, dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1), seed=123, verbose=False, layout='observed')
    model.initialise("random")
    model._push()
    held = 0
    if a.kind == "with":
        Et = entries(I, J, n_held, 1)
        model._set_heldout(Et)
        held = len(Et)
    h, L = model._handle(), _lib.lib()

    def timed(n):
        t = time.perf_counter()
        _lib.check(L.bnmf_obs_run(h, n, _lib.UPDATE_DRAW, None, None, None, None, None)); _lib.check(L.bnmtf_sync(h))
        return time.perf_counter() - t

    timed(a.warmup)
    pilot = timed(10) / 10
    steps = int(min(max(a.region / pilot, 10), 5000))
    rates = [steps / timed(steps) for _ in range(a.repeats)]
    print("OBS_HELDOUT " + json.dumps({"config": a.child, "kind": a.kind, "I": I, "J": J, "K": K, "missing": frac, "entries": len(E), "heldout_entries": held,
                                       "steps": steps, "it_per_s": [round(r, 2) for r in rates], "median_it_per_s": round(statistics.median(rates), 2)}), flush=True)


def child_create(a):
    from bnmtf_amd import bnmf_gibbs_optimised
    I, J, K, n = CREATE
    E = entries(I, J, n, 0)
    args = (E, None)
    if a.create == "dense":
        args = E.to_dense()
        del E
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    t0 = time.perf_counter()
    model = bnmf_gibbs_optimised(*args, K, dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1), seed=123, verbose=False, layout='observed')
    model._handle()
    dt = time.perf_counter() - t0
    print("OBS_HELDOUT " + json.dumps({"create": a.create, "I": I, "J": J, "K": K, "entries": int(model.size_Omega), "constructor_and_handle_s": round(dt, 3),
                                       "peak_rss_MB_before": round(rss0 / 1024.0, 1), "peak_rss_MB": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)}), flush=True)


def spawn(args, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("OBS_HELDOUT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit("child failed: %s" % " ".join(args))          # (nothing more is started on the GPU)
    print(line[0], flush=True)
    return json.loads(line[0][len("OBS_HELDOUT "):])


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_heldout_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library; without it the parent kind is left out")
    p.add_argument("--rounds", type=int, default=2, help="children per kind and configuration, the kinds alternating")
    p.add_argument("--region", type=float, default=0.5, help="seconds per timed region")
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--configs", default=",".join(CONFIGS))
    p.add_argument("--child", default=None, choices=sorted(CONFIGS))
    p.add_argument("--kind", default="without", choices=KINDS)
    p.add_argument("--create", default=None, choices=("dense", "entries"), help="(child) the construction measurement")
    p.add_argument("--no-create", action="store_true", help="leave the construction measurement out")
    a = p.parse_args()
    if a.create:
        return child_create(a)
    if a.child:
        return child_rate(a)
    base = dict(os.environ)
    base.pop("BNMTF_LIB", None)
    kinds = [k for k in KINDS if k != "parent_without" or a.parent_lib]
    children, summary = [], {}
    for cfg in a.configs.split(","):
        for _ in range(a.rounds):
            for kind in kinds:
                env = dict(base)
                if kind == "parent_without":
                    env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                children.append(spawn(["--child", cfg, "--kind", kind, "--region", str(a.region), "--warmup", str(a.warmup), "--repeats", str(a.repeats)], env))
        s = {}
        for kind in kinds:
            rs = [x for c in children if c["config"] == cfg and c["kind"] == kind for x in c["it_per_s"]]
            s[kind] = {"median_it_per_s": round(statistics.median(rs), 2), "range_it_per_s": [min(rs), max(rs)]}
        one = [c for c in children if c["config"] == cfg and c["kind"] == "with"][0]
        s["entries"], s["heldout_entries"] = one["entries"], one["heldout_entries"]
        s["iteration_without_us"] = round(1e6 / s["without"]["median_it_per_s"], 2)
        s["curve_us_per_iteration"] = round(1e6 / s["with"]["median_it_per_s"] - 1e6 / s["without"]["median_it_per_s"], 2)
        summary[cfg] = s
    created = [] if a.no_create else [spawn(["--create", how], base) for how in ("dense", "entries", "dense", "entries")]
    with open(a.out, "w") as f:
        json.dump({"what": "bnmf_gibbs_optimised(layout='observed'), Gibbs draws, no sample hand-off: it/s without a held-out list on the parent build and "
                           "on this build, and with one on this build; same box, fresh child processes alternating; and the construction of the "
                           "16384 x 16384 model from dense arrays against from an Entries; tools/obs_heldout_rates.py",
                   "summary": summary, "construction": created, "children": children}, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": summary, "construction": created}, indent=1))


if __name__ == "__main__":
    main()
