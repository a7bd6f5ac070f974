"""What run(..., M_test=) costs: iteration rates with and without a held-out mask, and against another build of the library.

    python tools/heldout_rates.py --out profiles/heldout_rates.json [--parent-lib /path/to/parent/libbnmtf_hip.so]

Two configurations: BNMF Gibbs 4096 x 4096, K = 32 and BNMTF VB 4096 x 4096, K = L = 32, 10 % of the
entries unobserved; the held-out mask is exactly those 10 %.  Every measurement is a fresh child process (this one never touches
the GPU): it builds the model, warms up, then times `--repeats` regions of `--steps` iterations each -- for this build alternating
without / with the mask on ONE handle (the mask is set once per region, outside the timed part), for the parent build without
(it has no such entry point).  The children of the two builds alternate, so box and clock are shared; the shader clock is read
beside the loop (bench.py's rocm-smi helper) and the iteration is also given in shader cycles.

    python tools/heldout_rates.py --child bnmf_4096_k32 --mask --steps 50 --no-clock      # one region, e.g. under rocprofv3
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
CONFIGS = ("bnmf_4096_k32", "bnmtf_vb_4096_k32")


def child(a):
    import bench
    helper = None if a.no_clock else bench._clock_helper_start()         # (before anything here touches the GPU)
    from bnmtf_amd import _lib
    from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf
    has_entry = not a.parent
    if a.parent:                    # the parent build has no held-out entry points to bind
        for name in ("bnmtf_set_heldout", "bnmtf_get_heldout"):
            _lib._SIGS.pop(name)
    w = bench.WORKLOADS[a.child]
    if w["kind"] == "trivb":
        R, M, _, _, _ = generate_bnmtf(w["I"], w["J"], w["K"], w["L"], 0.1, seed_data=0, seed_mask=1)
    else:
        R, M, _, _ = generate_bnmf(w["I"], w["J"], w["K"], 0.1, tau=1.0, seed_data=0, seed_mask=1)
    model = bench.build_model(w, R, M, 0, 1, 0, None)
    h, L = model._handle(), _lib.lib()
    Mt = None if a.parent else model._check_heldout(1 - M)
    orders = None
    if w["kind"] == "trivb":
        import random
        random.seed(1)
        orders = np.ascontiguousarray(model._draw_orders(max(a.steps, a.warmup)))

    def run(n):
        if w["kind"] == "trivb":
            _lib.check(L.bnmtf_vb_run(h, n, _lib.ptr(orders[:n]), None, None, None, None))
        else:
            _lib.check(L.bnmf_gibbs_run(h, n, _lib.UPDATE_DRAW, None, None, None, None, None))

    def sync():
        _lib.check(L.bnmtf_sync(h))

    run(a.warmup); sync()
    modes = ["mask"] if a.mask else (["no_mask", "mask"] if has_entry and not a.no_mask_only else ["no_mask"])
    rates = {m: [] for m in modes}
    for _ in range(a.repeats):
        for mode in modes:
            if has_entry:
                model._set_heldout(Mt if mode == "mask" else None)
            run(20); sync()
            t0 = time.perf_counter()
            run(a.steps); sync()
            rates[mode].append(a.steps / (time.perf_counter() - t0))
    clock = None
    if helper is not None:
        if has_entry:
            model._set_heldout(None)
        clock = bench._clock_beside(helper, lambda: run(a.steps), sync)
    sclk = clock["sclk_mhz_median"] if clock else None
    out = {"config": a.child, "build": "parent" if a.parent else "this", "steps": a.steps, "heldout_entries": None if Mt is None else int(Mt.sum()),
           "sclk_mhz": sclk, "describe": model.describe()}
    for m in modes:
        med = statistics.median(rates[m])
        out[m] = {"it_per_s": [round(r, 1) for r in rates[m]], "median_it_per_s": round(med, 1), "us_per_iteration": round(1e6 / med, 2),
                  "kcycles_per_iteration": None if sclk is None else round(sclk * 1e3 / med, 1)}
    print("HELDOUT_RATES " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout_rates.json"))
    p.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for the same-box A/B without a mask")
    p.add_argument("--rounds", type=int, default=2, help="children per build and configuration, the builds alternating")
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--warmup", type=int, default=100)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--child", default=None, choices=CONFIGS)
    p.add_argument("--parent", action="store_true", help="(child) the library loaded is the parent build")
    p.add_argument("--mask", action="store_true", help="(child) only regions with the mask")
    p.add_argument("--no-mask-only", action="store_true", help="(child) only regions without the mask")
    p.add_argument("--no-clock", action="store_true")
    a = p.parse_args()
    if a.child:
        return child(a)
    results = []
    for cfg in CONFIGS:
        for _ in range(a.rounds):
            for build in (["parent"] if a.parent_lib else []) + ["this"]:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                env = dict(os.environ)
                if build == "parent":
                    cmd.append("--parent"); env["BNMTF_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("BNMTF_LIB", None)
                if a.no_clock:
                    cmd.append("--no-clock")
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                line = [l for l in r.stdout.splitlines() if l.startswith("HELDOUT_RATES ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
                    raise SystemExit("child failed: %s (%s)" % (cfg, build))          # (nothing more is started on the GPU)
                results.append(json.loads(line[0][len("HELDOUT_RATES "):]))
                print(line[0], flush=True)
    summary = {}
    for cfg in CONFIGS:
        s = {}
        for build, mode in (("parent", "no_mask"), ("this", "no_mask"), ("this", "mask")):
            rs = [r[mode]["median_it_per_s"] for r in results if r["config"] == cfg and r["build"] == build and mode in r]
            kc = [r[mode]["kcycles_per_iteration"] for r in results if r["config"] == cfg and r["build"] == build and mode in r and r[mode]["kcycles_per_iteration"]]
            if rs:
                s["%s_%s" % (build, mode)] = {"it_per_s": rs, "kcycles_per_iteration": kc}
        if "this_mask" in s:
            a_, b_ = statistics.median(s["this_no_mask"]["it_per_s"]), statistics.median(s["this_mask"]["it_per_s"])
            s["mask_cost_us_per_iteration"] = round(1e6 / b_ - 1e6 / a_, 2)
        summary[cfg] = s
    with open(a.out, "w") as f:
        json.dump({"what": "iteration rates with / without a 10 % held-out mask (run(M_test=)) and against the parent build, same box, "
                           "children alternating; tools/heldout_rates.py", "summary": summary, "children": results}, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
