#!/usr/bin/env python3
"""Headline benchmark: Gibbs iterations/sec of BNMF on a synthetic I=J=8192, K=64 matrix
with a 10 % missing mask (BASELINE.json metric / configs[2]; it fits one GPU).

    python bench.py --gpus N --steps K --warmup W [--workload NAME] [--repeats R] [--dump-outputs DIR]

One process per GPU.  For N > 1 the ranks are either started by a launcher that sets RANK / WORLD_SIZE /
LOCAL_RANK / MASTER_ADDR / MASTER_PORT (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`: used
as a process launcher only) or, when bench.py is called directly, by bench.py itself (N child processes, started
before anything touches a GPU).  Rows of R are split over the ranks for the U sweep, columns for the V sweep; the
factor blocks are exchanged with RCCL inside libbnmtf_hip.so; the control plane (RCCL id, barrier, max of the
times) is plain TCP (bnmtf_amd/comm.py) -- no PyTorch anywhere.

A step is one full iteration exactly as the reference's run() defines it (bnmf_gibbs_optimised.py:133-155): K column
updates of U, K of V, the tau draw, the sample hand-off (all_U[it], all_V[it]) and the three training-mask metrics.
Inputs (R, M) are resident in HBM when the timed region starts; `value` is the rate of that whole iteration, samples
handed to page-locked host arrays included; `device_resident` is the same loop with the samples left
on the device.  `mse_trajectory` holds the masked MSE of the first iterations of this very run (up to 200), and
`cpu_baseline.mse_vs_iter_small` the same chain (same Philox seed) run by the CPU oracle and by the device at a size
the oracle finishes.  Rank 0 prints ONE JSON line.

--steps K is the number of timed iterations, and `ms_per_step` the time one of them took (the timed seconds over K).
--dump-outputs DIR writes what the timed path computed in its last iteration -- the state a caller of run() holds after it
and that iteration's metrics -- as DIR/<name>.npy; the inputs and the initial state are seeded, so that two builds can be
compared output for output.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_VECTOR_TFLOPS = 157.3    # MI355X_MICROARCH.md: fp32 vector peak = f32 MFMA peak
PEAK_BF16_MFMA_TFLOPS = 2500.0    # dense bf16 MFMA peak (the contraction takes 6 bf16 products per fp32 product)
PEAK_HBM_GBS = 8000.0

WORKLOADS = {
    "bnmf_8192_k64": dict(kind="bnmf", I=8192, J=8192, K=64),          # BASELINE.json metric config (headline)
    "bnmf_4096_k32": dict(kind="bnmf", I=4096, J=4096, K=32),          # configs[1]
    "bnmf_1024_k16": dict(kind="bnmf", I=1024, J=1024, K=16),
    "bnmf_8192_k32": dict(kind="bnmf", I=8192, J=8192, K=32),          # the 16-wave sweep with one register of columns per lane
    "bnmtf_4096_k32": dict(kind="bnmtf", I=4096, J=4096, K=32, L=32),  # configs[3]
    "vb_8192_k64": dict(kind="vb", I=8192, J=8192, K=64),              # configs[4]
    "bnmtf_vb_4096_k32": dict(kind="trivb", I=4096, J=4096, K=32, L=32),   # bnmtf_vb_optimised (round 6: the first measurement of it)
    "vb_4096_k32": dict(kind="vb", I=4096, J=4096, K=32),
    "vb_8192_k32": dict(kind="vb", I=8192, J=8192, K=32),
    # the shapes the reference itself publishes numbers for: one small model / a model-selection job
    "bnmf_toy_100x80_k10": dict(kind="bnmf", small=True, I=100, J=80, K=10, missing=0.0, steps=1000, published=29.3,
                                source="plots/time_toy/nmf_gibbs_times.txt (1000 it in 34.16 s; experiments_toy/time/nmf_gibbs_time.py:23-51, M = ones)"),
    "bnmf_gdsc_622x138_k25": dict(kind="bnmf", small=True, I=622, J=138, K=25, missing=0.19, steps=500, published=2.49,
                                  source="plots/time_Sanger/nmf_gibbs_times.txt (500 it in 201.0 s; experiments_gdsc/time/nmf_gibbs_time.py:22-47, 81 % observed)"),
    "bnmtf_toy_100x80_k5": dict(kind="bnmtf", small=True, I=100, J=80, K=5, L=5, missing=0.0, steps=1000, published=45.1,
                                source="plots/time_toy/nmtf_gibbs_times.txt (2000 it in 44.37 s; experiments_toy/time/nmtf_gibbs_time.py:25-53)"),
    "bnmtf_gdsc_622x138_k5": dict(kind="bnmtf", small=True, I=622, J=138, K=5, L=5, missing=0.19, steps=1000, published=9.02,
                                  source="plots/time_Sanger/nmtf_gibbs_times.txt (1000 it in 110.8 s; experiments_gdsc/time/nmtf_gibbs_time.py, K = L = 5, 81 % observed)"),
    "cv_gdsc": dict(kind="cv", small=True, I=622, J=138, K=25, missing=0.19, values_K=[15, 20, 25, 30], folds=10, iterations=1000, burn_in=900, thinning=2,
                    source="experiments_gdsc/cross_validation/gibbs_nmf/linesearch_xval_gibbs.py:17-62 (10 folds x K in {15,20,25,30} x 1000 it, AIC, then 10 final models)"),
    "cv_gdsc_vb": dict(kind="cv", classifier="vb", small=True, I=622, J=138, K=25, missing=0.19, values_K=[15, 20, 25, 30], folds=10, iterations=1000, burn_in=0, thinning=1,
                       published={"MSE": 2.2822, "R^2": 0.8056},
                       source="experiments_gdsc/cross_validation/vb_nmf/linesearch_xval_vb.py:17-52 (10 folds x K in {15,20,25,30} x 1000 VB iterations, AIC, then 10 final models; "
                              "the file's own results on the real GDSC data: MSE 2.282, R^2 0.806)"),
    "cv_gdsc_bnmtf": dict(kind="cv3", small=True, I=622, J=138, K=8, L=8, missing=0.19, values_K=[5, 6, 7, 8, 9, 10], values_L=[5, 6, 7, 8, 9, 10], folds=10,
                          iterations=1000, burn_in=900, thinning=2, published={"MSE": 2.402, "R^2": 0.795},
                          source="experiments_gdsc/cross_validation/gibbs_nmtf/greedysearch_xval_gibbs.py:17-60 (10 folds, greedy search over K, L in 5..10 by AIC, "
                                 "init S random / F, G k-means, 1000 it, burn-in 900, thinning 2; the file's own results on the real GDSC data: MSE 2.402, R^2 0.795)"),
}
PRI2 = dict(alpha=1.0, beta=1.0, lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
REGION_SAMPLE_BYTES = 512 << 20     # page-locked sample arrays of one timed region, at most (they are re-used by every region)
DUMP_LIMIT_BYTES = 64 * 10 ** 6
STATE = {"bnmf": ("U", "V", "tau"), "bnmtf": ("F", "S", "G", "tau")}     # (the variational models: their _NAMES)


def _regions(steps, repeats, sample_bytes_per_step=0):
    """The --steps timed iterations as consecutive timed regions: --repeats of them, more when one region's samples would not
    fit REGION_SAMPLE_BYTES; sizes differ by at most one, the first is the largest."""
    cap = max(1, REGION_SAMPLE_BYTES // sample_bytes_per_step) if sample_bytes_per_step else steps
    r = max(min(max(1, repeats), steps), -(-steps // cap))
    return [steps // r + (i < steps % r) for i in range(r)]


def model_outputs(model, kind, metrics):
    """What run() leaves a caller after the last timed iteration: the model's state (the last sample of the Gibbs samplers,
    the q-parameters of the variational ones) and that iteration's MSE, R^2, Rp."""
    model._pull()
    out = {n: getattr(model, n) for n in STATE.get(kind, getattr(model, "_NAMES", ()))}
    out["metrics"] = metrics
    return out


def dump_outputs(d, arrays):
    """--dump-outputs: d/<name>.npy in float64 (64 MB in all at most: every workload's outputs fit whole)."""
    arrays = {n: np.asarray(a, dtype=np.float64) for n, a in arrays.items()}
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_LIMIT_BYTES, {n: a.shape for n, a in arrays.items()}
    os.makedirs(d, exist_ok=True)
    for n, a in arrays.items():
        np.save(os.path.join(d, n + ".npy"), a)


def _blas_cores():
    try:
        import threadpoolctl
        return int(max(i["num_threads"] for i in threadpoolctl.threadpool_info() if i.get("user_api") == "blas"))
    except Exception:
        return int(os.cpu_count() or 1)


def cpu_baseline(w, R, M, whole=False):
    """The oracle (NumPy restatement of the reference, fp64, as written) on a bounded sample of the same workload, at
    full size: a few column / entry updates of each kind timed and scaled to the iteration's count, plus the tail
    (tau + metrics).  ~10-30 s of CPU work; the figure is then EXTRAPOLATED and says so (`extrapolated`).  whole=True
    (BNMF Gibbs): every column of one iteration is timed -- a measurement, minutes at the headline size
    (profiles/bench/r06_cpu_whole_iteration_*.json holds the round's)."""
    from oracle import bnmtf_oracle as O
    from oracle import rng as orng
    K, kind = w["K"], w["kind"]
    R = R.astype(np.float64); M = M.astype(np.float64)
    rs = np.random.RandomState(0)
    tic = time.perf_counter
    fair, kind_note = None, "port"
    if kind == "bnmf":
        o = O.BNMFGibbsOracle(R, M, K, PRI2, seed=0)
        o.U = rs.exponential(10.0, (o.I, K)); o.V = rs.exponential(10.0, (o.J, K)); o.tau = 1.0
        n = K if whole else min(K, 10 if o.I * o.J <= 4096 * 4096 else 4)
        t0 = tic()
        for k in range(n):
            t = o.tauU(k); m = o.muU(t, k); o.U[:, k] = orng.tn_draw(m, t, np.arange(o.I), k, 0, orng.STREAM_ROWS, 0)
        t1 = tic()
        for k in range(n):
            t = o.tauV(k); m = o.muV(t, k); o.V[:, k] = orng.tn_draw(m, t, np.arange(o.J), k, 0, orng.STREAM_COLS, 0)
        t2 = tic()
        o.tau = orng.gamma_draw(o.alpha_s(), o.beta_s(), 0, 0)
        o.predict_while_running()
        t3 = tic()
        sec = K * (t2 - t0) / n + (t3 - t2)
        sample = "%d of %d U-column updates %.2fs, %d of %d V-column updates %.2fs, tau+metrics %.2fs" % (n, K, t1 - t0, n, K, t2 - t1, t3 - t2)
        kind_note = "every column of one iteration timed" if n == K else "extrapolated from %d of %d column updates of each factor" % (n, K)
        # the "fair CPU" variant: same conditionals on the masked residual kept current by rank-one
        # updates (O(I J) per column instead of a full U V^T product), vectorised sampler -- so that the ratio is not only
        # the as-written algorithm's redundant dgemms.  Same sampling: n columns of each factor, scaled.
        t4 = tic()
        E = o.M * (o.R - o.U @ o.V.T)
        t5 = tic()
        for k in range(n):
            a_ = o.M @ (o.V[:, k] ** 2); t = o.tau * a_
            m = (-o.lambdaU[:, k] + o.tau * (E @ o.V[:, k] + o.U[:, k] * a_)) / t
            new = orng.tn_draw(m, t, np.arange(o.I), k, 1, orng.STREAM_ROWS, 0)
            E -= o.M * np.outer(new - o.U[:, k], o.V[:, k]); o.U[:, k] = new
        for k in range(n):
            a_ = o.M.T @ (o.U[:, k] ** 2); t = o.tau * a_
            m = (-o.lambdaV[:, k] + o.tau * (E.T @ o.U[:, k] + o.V[:, k] * a_)) / t
            new = orng.tn_draw(m, t, np.arange(o.J), k, 1, orng.STREAM_COLS, 0)
            E -= o.M * np.outer(o.U[:, k], new - o.V[:, k]); o.V[:, k] = new
        t6 = tic()
        (E ** 2).sum(); o.predict_while_running()
        t7 = tic()
        fair_sec = (t5 - t4) + K * (t6 - t5) / n + (t7 - t6)
        fair = {"value": 1.0 / fair_sec, "unit": "iterations/s", "kind": "port", "form": "residual form, vectorised sampler", "extrapolated": None if n == K else kind_note,
                "sample": "oracle.BNMFGibbsFairCPU arithmetic at full size: residual %.2fs, %d of %d column updates of each factor %.2fs, tau+metrics %.2fs; iteration = %.1fs" % (
                    t5 - t4, n, K, t6 - t5, t7 - t6, fair_sec)}
    elif kind == "bnmtf":
        L = w["L"]
        o = O.BNMTFGibbsOracle(R, M, K, L, PRI3, seed=0)
        o.F = rs.exponential(1.0, (o.I, K)); o.S = rs.exponential(1.0, (K, L)); o.G = rs.exponential(1.0, (o.J, L)); o.tau = 1.0
        nf, ns = 2, 6
        t0 = tic()
        for k in range(nf):
            t = o.tauF(k); m = o.muF(t, k); o.F[:, k] = orng.tn_draw(m, t, np.arange(o.I), k, 0, orng.STREAM_ROWS, 0)
        t1 = tic()
        for l in range(ns):
            t = o.tauS(0, l); m = o.muS(t, 0, l); o.S[0, l] = float(orng.tn_draw(m, t, 0, l, 0, orng.STREAM_S, 0))
        t2 = tic()
        for l in range(nf):
            t = o.tauG(l); m = o.muG(t, l); o.G[:, l] = orng.tn_draw(m, t, np.arange(o.J), l, 0, orng.STREAM_COLS, 0)
        t3 = tic()
        o.tau = orng.gamma_draw(o.alpha_s(), o.beta_s(), 0, 0)
        o.predict_while_running()
        t4 = tic()
        sec = K * (t1 - t0) / nf + K * L * (t2 - t1) / ns + L * (t3 - t2) / nf + (t4 - t3)
        sample = "%d of %d F columns %.2fs, %d of %d S entries %.2fs, %d of %d G columns %.2fs, tau+metrics %.2fs" % (
            nf, K, t1 - t0, ns, K * L, t2 - t1, nf, L, t3 - t2, t4 - t3)
        kind_note = "extrapolated from %d of %d F columns, %d of %d S entries, %d of %d G columns" % (nf, K, ns, K * L, nf, L)
    elif kind == "trivb":
        import random as _random
        L = w["L"]
        o = O.BNMTFVBOracle(R, M, K, L, PRI3)
        np.random.seed(0); _random.seed(0)
        o.initialise("random", "random")          # (host TN moments of every entry + one exp_square_diff: not timed)
        nf, ns = 2, 6
        t0 = tic()
        for kk, ll in [(0, l) for l in range(ns)]:
            o.update_S(kk, ll); o.update_exp_S(kk, ll)
        t1 = tic()
        for k in range(nf):
            o.update_F(k); o.update_exp_F(k)
        t2 = tic()
        for l in range(nf):
            o.update_G(l); o.update_exp_G(l)
        t3 = tic()
        o.update_tau(); o.update_exp_tau(); o.predict(o.M)
        t4 = tic()
        sec = K * L * (t1 - t0) / ns + K * (t2 - t1) / nf + L * (t3 - t2) / nf + (t4 - t3)
        sample = "%d of %d S entries %.2fs, %d of %d F columns %.2fs, %d of %d G columns %.2fs, tau+metrics %.2fs" % (
            ns, K * L, t1 - t0, nf, K, t2 - t1, nf, L, t3 - t2, t4 - t3)
        kind_note = "extrapolated from %d of %d S entries, %d of %d F columns, %d of %d G columns" % (ns, K * L, nf, K, nf, L)
    else:
        o = O.BNMFVBOracle(R, M, K, PRI2)
        o.muU = rs.exponential(1.0, (o.I, K)); o.muV = rs.exponential(1.0, (o.J, K))
        o.tauU = np.ones((o.I, K)); o.tauV = np.ones((o.J, K))
        o.expU, o.varU = o.muU.copy(), np.ones((o.I, K)); o.expV, o.varV = o.muV.copy(), np.ones((o.J, K))
        o.exptau = 1.0
        n = min(K, 8 if o.I * o.J <= 4096 * 4096 else 3)
        t0 = tic()
        for k in range(n):
            o.update_U(k); o.update_exp_U(k)
        for k in range(n):
            o.update_V(k); o.update_exp_V(k)
        t1 = tic()
        o.update_tau(); o.update_exp_tau(); o.predict(o.M); o.elbo()
        t2 = tic()
        sec = K * (t1 - t0) / n + (t2 - t1)
        sample = "%d of %d update_U+update_exp_U and as many for V %.2fs, tau+metrics+ELBO %.2fs" % (n, K, t1 - t0, t2 - t1)
        kind_note = "extrapolated from %d of %d column updates of each factor" % (n, K)
    out = {"value": 1.0 / sec, "unit": "iterations/s", "cores": _blas_cores(), "kind": "port",
           "extrapolated": None if kind_note.startswith("every") else kind_note,
           "sample": "oracle/bnmtf_oracle.py (NumPy fp64, as written) at full size: %s; iteration = %.1fs" % (sample, sec)}
    if fair is not None:
        out["fair_cpu"] = fair
    return out


def small_trajectories(n_iter=25):
    """Masked MSE vs iteration of ONE chain run twice: by the CPU oracle and by the device, same data, same initial state,
    same Philox seed (BNMF Gibbs, 1024 x 1024, K = 16, 10 % missing: a size the oracle finishes in seconds)."""
    import bnmtf_amd
    from bnmtf_amd.synthetic import generate_bnmf
    from oracle import bnmtf_oracle as O
    I = J = 1024; K = 16
    R, M, _, _ = generate_bnmf(I, J, K, 0.1, tau=1.0, seed_data=0, seed_mask=1)
    np.random.seed(0)
    b = bnmtf_amd.bnmf_gibbs_optimised(R, M, K, PRI2, seed=0, verbose=False)
    b.initialise("random")
    o = O.BNMFGibbsOracle(R.astype(np.float64), M.astype(np.float64), K, PRI2, seed=0)
    o.U, o.V, o.tau = b.U.copy(), b.V.copy(), b.tau
    t0 = time.perf_counter(); o.run(n_iter); t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter(); b.run(n_iter); t_gpu = time.perf_counter() - t0
    b.close()
    return {"config": "BNMF Gibbs %dx%d K=%d, 10%% missing, seed 0, %d iterations" % (I, J, K, n_iter),
            "cpu_oracle_mse": [float(x) for x in o.all_performances["MSE"]], "device_mse": [float(x) for x in b.all_performances["MSE"]],
            "cpu_oracle_s_per_iteration": t_cpu / n_iter, "device_s_per_iteration": t_gpu / n_iter}


def build_model(w, R, M, rank, world, local_rank, comm_id):
    import bnmtf_amd
    kw = dict(seed=0, device=local_rank, verbose=False, rank=rank, world=world, comm_id=comm_id)
    np.random.seed(0)
    if w["kind"] == "bnmf":
        m = bnmtf_amd.bnmf_gibbs_optimised(R, M, w["K"], PRI2, **kw)
        m.initialise("random")
    elif w["kind"] == "bnmtf":
        m = bnmtf_amd.bnmtf_gibbs_optimised(R, M, w["K"], w["L"], PRI3, **kw)
        m.initialise("random", "random")
    elif w["kind"] == "trivb":
        import random as _random
        assert world == 1, "bnmtf_vb runs on one GPU"
        m = bnmtf_amd.bnmtf_vb_optimised(R, M, w["K"], w["L"], PRI3, device=local_rank, verbose=False)
        _random.seed(0)
        m.initialise("random", "random")
    else:
        kw.pop("seed")
        m = bnmtf_amd.bnmf_vb_optimised(R, M, w["K"], PRI2, **kw)
        m.initialise("exp")
    m._push()
    return m


def _small_problem(w, seed=0):
    from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf
    if w["kind"] in ("bnmtf", "cv3"):
        R, M, _, _, _ = generate_bnmtf(w["I"], w["J"], w["K"], w["L"], w["missing"], seed_data=seed, seed_mask=seed + 1)
    else:
        R, M, _, _ = generate_bnmf(w["I"], w["J"], w["K"], w["missing"], tau=1.0, seed_data=seed, seed_mask=seed + 1)
    return R, M


def _small_model(w, R, M, seed):
    import bnmtf_amd
    np.random.seed(seed)
    if w["kind"] == "bnmtf":
        m = bnmtf_amd.bnmtf_gibbs_optimised(R, M, w["K"], w["L"], PRI3, seed=seed, verbose=False)
        m.initialise("random", "random")
    else:
        m = bnmtf_amd.bnmf_gibbs_optimised(R, M, w["K"], PRI2, seed=seed, verbose=False)
        m.initialise("random")
    m._push()
    return m


_CLOCK_HELPER = r"""
import json, re, shutil, subprocess, sys, threading
rows, stop = [], threading.Event()
def sampler():
    while not stop.is_set():
        try:
            card = json.loads(subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=10).stdout)
            card = card[sorted(card)[0]]
            sclk = next((float(re.sub(r"[^0-9.]", "", str(v))) for k, v in card.items() if k.lower().startswith("sclk") and "mhz" in str(v).lower()), None)
            power = next((float(v) for k, v in card.items() if "power" in k.lower() and re.fullmatch(r"[0-9.]+", str(v))), None)
            if sclk is not None:
                rows.append((sclk, power))
        except Exception:
            return
        stop.wait(0.05)
th = None
for line in sys.stdin:
    cmd = line.strip()
    if cmd == "begin":
        rows.clear(); stop.clear()
        th = threading.Thread(target=sampler, daemon=True); th.start()
    elif cmd == "end":
        stop.set()
        if th is not None: th.join(timeout=15)
        print(json.dumps(rows)); sys.stdout.flush()
    elif cmd == "quit":
        break
"""


def _clock_helper_start():
    """The rocm-smi sampler as a helper PROCESS, started before this process has touched the GPU: rocm-smi is a `#!/usr/bin/env
    python3` script, and on this pool a process that has initialised the GPU (or a fork of one) must not exec another program
    (round 6: the boxes refuse it; under rocprofv3 every reading was refused).  The helper never touches the GPU; it samples
    between "begin" and "end" on its stdin."""
    import shutil, subprocess
    if shutil.which("rocm-smi") is None:
        return None
    try:
        return subprocess.Popen([sys.executable, "-c", _CLOCK_HELPER], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    except Exception:      # noqa: BLE001 -- a reading is optional
        return None


def _clock_beside(helper, work, sync, seconds=2.0):
    """Median shader clock (MHz) and socket power (W) by rocm-smi (the helper process) while `work()` is repeated for ~`seconds` (untimed)."""
    import statistics
    if helper is None:
        return None
    try:
        work(); sync()
        helper.stdin.write("begin\n"); helper.stdin.flush()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            work()
            sync()
        helper.stdin.write("end\n"); helper.stdin.flush()
        rows = json.loads(helper.stdout.readline() or "[]")
        helper.stdin.write("quit\n"); helper.stdin.flush()
    except Exception:      # noqa: BLE001
        return None
    rows = [r for r in rows if r[0] > 500.0]          # (a reading taken after the loop ended shows the idle clock)
    if not rows:
        return None
    pw = [r[1] for r in rows if r[1] is not None]
    return {"sclk_mhz_median": statistics.median(r[0] for r in rows), "power_w_median": statistics.median(pw) if pw else None, "readings": len(rows),
            "what": "rocm-smi (a helper process started before the GPU was touched) beside ~%.0f s of the device-resident loop, after the timed regions (untimed)" % seconds}


def main_small(a, w):
    """The shapes the reference publishes numbers for: ONE small model through the class API (what its timing scripts do), a batch
    of independent models in one launch (folds / ranks / restarts of a model search), and the cost of building a model."""
    import bnmtf_amd
    from bnmtf_amd import _lib
    steps = a.steps if a.steps_given else w["steps"]
    R, M = _small_problem(w)
    # construction: class + initialise + handle (bnmtf_create), a fresh model each time
    t_build = []
    for s in range(6):
        t0 = time.perf_counter(); m = _small_model(w, R, M, s); _lib.check(_lib.lib().bnmtf_sync(m._handle())); t_build.append(time.perf_counter() - t0)
        if s < 5:
            m.close()
    m.run(max(a.warmup, 1))
    # one model, the reference's call: run(iterations) with every sample handed to the host and the three metrics per iteration
    sizes = _regions(steps, a.repeats)
    dts = []
    for n in sizes:
        t0 = time.perf_counter(); m.run(n); dts.append(time.perf_counter() - t0)
    mse = list(m.all_performances["MSE"])
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, model_outputs(m, w["kind"], [m.all_performances[q][-1] for q in ("MSE", "R^2", "Rp")]))
    dt = float(sum(dts))
    dev_s = float(m.all_times[-1])           # the device's own clock over the last call (HIP events around the iterations)
    t0 = time.perf_counter(); m.run(steps, store_samples=False); t_nos = time.perf_counter() - t0
    desc = m.describe()
    m.close()
    # a batch of independent models (different masks / seeds, same shape) in ONE call: what a model search runs
    batch = None
    if w["kind"] in ("bnmf", "bnmtf"):       # (run_many: the models of the one-launch path share a launch, a block each)
        batch = {}
        for nb in a.batch:
            ms = []
            for s in range(nb):
                Rb, Mb = _small_problem(w, seed=100 + s) if nb <= 64 else (R, M)
                ms.append(_small_model(w, Rb, Mb, 1000 + s))
            bnmtf_amd.run_many(ms, max(a.warmup, 1), store_samples=False)
            t0 = time.perf_counter(); bnmtf_amd.run_many(ms, steps, store_samples=False); tb = time.perf_counter() - t0
            t0 = time.perf_counter(); bnmtf_amd.run_many(ms, steps, store_samples=True); tbs = time.perf_counter() - t0
            fin = [float(x.all_performances["MSE"][-1]) for x in ms]
            batch[str(nb)] = {"models": nb, "model_iterations_per_s": nb * steps / tb, "per_model_it_s": steps / tb, "with_samples_model_iterations_per_s": nb * steps / tbs,
                              "final_mse_min_max": [min(fin), max(fin)]}
            for x in ms:
                x.close()
    kind = w["kind"]
    out = {"metric": ("Gibbs iterations/sec (BNMF, %dx%d, K=%d)" if kind == "bnmf" else "Gibbs iterations/sec (BNMTF, %dx%d, K=L=%d)") % (w["I"], w["J"], w["K"]),
           "value": steps / dt, "unit": "Gibbs iterations/s", "n_gpus": 1, "steps": steps, "warmup": a.warmup, "ms_per_step": 1e3 * dt / steps,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": (steps / dt) / w["published"], "dtype": "f32", "data": "synthetic",
           "config": {"workload": "%s Gibbs, synthetic R %dx%d K=%d%s, %.0f %% missing, priors alpha=beta=1 lambda=0.1, init random; one model through the class API: run(%d) incl. the sample hand-off and the per-iteration metrics" % (
               "BNMF" if kind == "bnmf" else "BNMTF", w["I"], w["J"], w["K"], " L=%d" % w["L"] if "L" in w else "", 100 * w["missing"], steps)},
           "published": {"value": w["published"], "unit": "iterations/s", "hardware": "unstated CPU, Python 2.7 (BASELINE.md section 1)", "source": w["source"]},
           "repeats": {"n": len(dts), "values": [n / d for n, d in zip(sizes, dts)]},
           "device_clock_it_s": sizes[-1] / dev_s if dev_s > 0 else None, "no_samples_it_s": steps / t_nos,
           "create_ms_per_model": {"median": 1e3 * float(np.median(t_build[1:])), "first": 1e3 * t_build[0], "what": "class constructor + initialise + bnmtf_create + state upload"},
           "batch": batch, "mse_first_last": [mse[0], mse[-1]], "describe": desc, "roofline": None, "cpu_baseline": None}
    print(json.dumps(out)); sys.stdout.flush()


def heldout_outputs(cv):
    """The model-selection jobs' result (of the last slot setting): every fold's held-out performance, per measure."""
    return {"heldout_" + q.replace("^", ""): v for q, v in cv.performances.items()}


def main_cv(a, w):
    """The reference's model-selection job (linesearch_xval_gibbs.py): 10 folds x K in {15, 20, 25, 30} x 1000 iterations through
    LineSearchCrossValidation, then 10 final models -- 50 model fits -- on one GPU with s replica slots."""
    import tempfile
    import bnmtf_amd
    from bnmtf_amd.cross_validation.line_search_cross_validation import LineSearchCrossValidation
    from bnmtf_amd.cross_validation.replicas import ReplicaPool
    import random
    R, M = _small_problem(w)
    its = a.steps if a.steps_given else w["iterations"]
    burn, thin = (w["burn_in"], w["thinning"]) if its == w["iterations"] else (its // 2, 2)
    res = {}
    vb = w.get("classifier") == "vb"             # (the variational line search, linesearch_xval_vb.py: no one-launch kernel; --cv-batched: the models of a slot share every launch, csrc/api_many.inc)
    for s in a.slots:
        random.seed(0); np.random.seed(0)
        pool = ReplicaPool(devices=[0] * s, shared={"R": np.asarray(R, dtype=float)}, **({"batched": True} if a.cv_batched else {}))
        with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
            cv = LineSearchCrossValidation(classifier=bnmtf_amd.bnmf_vb_optimised if vb else bnmtf_amd.bnmf_gibbs_optimised, R=R, M=M, values_K=w["values_K"], folds=w["folds"], priors=PRI2,
                                           init_UV="random", iterations=its, restarts=1, quality_metric="AIC", file_performance=f.name, pool=pool, seed=1)
            pool.map(_warm, [{} for _ in range(s)])            # workers up, library loaded, GPU context made: not the job
            t0 = time.perf_counter(); cv.run(**({} if vb else dict(burn_in=burn, thinning=thin))); dt = time.perf_counter() - t0
        pool.close()
        nmodels = w["folds"] * len(w["values_K"]) + w["folds"]
        res[str(s)] = {"slots": s, "seconds": dt, "models": nmodels, "model_iterations_per_s": nmodels * its / dt,
                       "heldout_MSE": cv.average_performance["MSE"], "heldout_R2": cv.average_performance["R^2"]}
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, heldout_outputs(cv))
    best = max(res.values(), key=lambda r: r["model_iterations_per_s"])
    out = {"metric": "model-iterations/sec of the GDSC-shaped 10-fold line-search cross-validation (BNMF %s 622x138, K in {15,20,25,30}, %d iterations)" % ("VB" if vb else "Gibbs", its),
           "value": best["model_iterations_per_s"], "unit": "model-iterations/s", "n_gpus": 1, "steps": its, "warmup": 0, "ms_per_step": 1e3 * best["seconds"] / its,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic (GDSC's shape and observed fraction)",
           "config": {"workload": "LineSearchCrossValidation, %d folds x K in %s x %d iterations (burn-in %d, thinning %d) + %d final models; ReplicaPool slots on one GPU: %s%s" % (
               w["folds"], w["values_K"], its, burn, thin, w["folds"], a.slots, ", batched launches" if a.cv_batched else ""), "source": w["source"]},
           "by_slots": res, "roofline": None, "cpu_baseline": None}
    if "published" in w:
        out["published_on_the_real_data"] = w["published"]
    print(json.dumps(out)); sys.stdout.flush()


def main_cv3(a, w):
    """The reference's model-selection job for the tri-factorisation (greedysearch_xval_gibbs.py): per fold a greedy walk over
    (K, L) by AIC -- every step fits the one to three neighbouring models --, then the folds' final models, through
    GreedySearchCrossValidation on one GPU: with s replica slots (processes; each model a call of its own), and with one batched
    slot ("1b": the steps the ten folds have open at the same time are ONE device call, a block per model -- kernel_small.hip)."""
    import tempfile
    import bnmtf_amd
    from bnmtf_amd.cross_validation.greedy_search_cross_validation import GreedySearchCrossValidation
    from bnmtf_amd.cross_validation.replicas import ReplicaPool
    import random
    R, M = _small_problem(w)
    its = a.steps if a.steps_given else w["iterations"]
    burn, thin = (w["burn_in"], w["thinning"]) if its == w["iterations"] else (its // 2, 2)
    res = {}
    for s, batched in [(s, False) for s in a.slots] + [(1, True)] + [(s, True) for s in a.slots if s > 1]:
        random.seed(0); np.random.seed(0)
        pool = ReplicaPool(devices=[0] * s, shared={"R": np.asarray(R, dtype=float)}, batched=batched)
        fits = [0]
        pmap = pool.map

        def counted(fn, jobs, *aa, **kk):
            jobs = list(jobs); fits[0] += len(jobs)
            return pmap(fn, jobs, *aa, **kk)
        pool.map = counted
        with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
            cv = GreedySearchCrossValidation(classifier=bnmtf_amd.bnmtf_gibbs_optimised, R=R, M=M, values_K=w["values_K"], values_L=w["values_L"], folds=w["folds"],
                                             priors=PRI3, init_S="random", init_FG="kmeans", iterations=its, restarts=1, quality_metric="AIC",
                                             file_performance=f.name, pool=pool, seed=1)
            pmap(_warm, [{} for _ in range(s)])
            t0 = time.perf_counter(); cv.run(burn_in=burn, thinning=thin); dt = time.perf_counter() - t0
        pool.close()
        res[str(s) + ("b" if batched else "")] = {"slots": s, "batched": batched, "seconds": dt, "models": fits[0], "model_iterations_per_s": fits[0] * its / dt,
                                                  "heldout_MSE": cv.average_performance["MSE"], "heldout_R2": cv.average_performance["R^2"]}
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, heldout_outputs(cv))
    best = max(res.values(), key=lambda r: r["model_iterations_per_s"])
    out = {"metric": "model-iterations/sec of the GDSC-shaped 10-fold greedy-search cross-validation (BNMTF Gibbs 622x138, K, L in 5..10, %d iterations)" % its,
           "value": best["model_iterations_per_s"], "unit": "model-iterations/s", "n_gpus": 1, "steps": its, "warmup": 0, "ms_per_step": 1e3 * best["seconds"] / its,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic (GDSC's shape and observed fraction, planted K = L = %d)" % w["K"],
           "config": {"workload": "GreedySearchCrossValidation, %d folds x greedy walk over K in %s, L in %s x %d iterations (burn-in %d, thinning %d, k-means initialisation of F and G) + %d final models; ReplicaPool slots on one GPU: %s, and one batched slot (\"1b\")" % (
               w["folds"], w["values_K"], w["values_L"], its, burn, thin, w["folds"], a.slots), "source": w["source"]},
           "published_on_the_real_data": w["published"], "by_slots": res, "roofline": None, "cpu_baseline": None}
    print(json.dumps(out)); sys.stdout.flush()


def _warm(job, shared):
    import bnmtf_amd
    R, M = _small_problem(dict(kind="bnmf", I=40, J=30, K=3, missing=0.1))
    m = bnmtf_amd.bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False, device=job.get("device", 0))
    m.initialise("random"); m.run(2, store_samples=False); m.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed iterations (default 100; the small workloads: their own count)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=1, help="timed regions the --steps iterations are split into; value = steps / timed seconds")
    ap.add_argument("--workload", default="bnmf_8192_k64", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-whole-iteration", action="store_true",
                    help="CPU baseline: time ONE WHOLE iteration of the as-written oracle (and of the residual-form 'fair' CPU variant) instead of a sample "
                         "of its column updates scaled to the iteration (minutes at the headline size: not the default)")
    ap.add_argument("--no-clock", action="store_true", help="skip the rocm-smi reading of shader clock / socket power behind the timed regions")
    ap.add_argument("--no-samples", action="store_true", help="leave the samples on the device in the timed loop too (then `value` is NOT the reference's iteration)")
    ap.add_argument("--batch", type=int, nargs="*", default=[16, 256], help="small workloads: models per batched call")
    ap.add_argument("--slots", type=int, nargs="*", default=[1, 4], help="cv_gdsc: replica slots on the GPU")
    ap.add_argument("--cv-batched", action="store_true", help="cv_gdsc: the pool fits its jobs in batched launches")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed path computed in its last iteration as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps is not None and a.steps < 1:
        ap.error("--steps must be at least 1")
    a.steps_given = a.steps is not None
    if a.steps is None:
        a.steps = 100
    if WORKLOADS[a.workload].get("small"):
        return {"cv": main_cv, "cv3": main_cv3}.get(WORKLOADS[a.workload]["kind"], main_small)(a, WORKLOADS[a.workload])

    from bnmtf_amd import comm
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # called directly: start one process per GPU ourselves (nothing here has touched the GPU)
        sys.exit(comm.spawn_local(a.gpus, [os.path.abspath(__file__)] + sys.argv[1:]))

    rank, world, local_rank, comm_id, cp = comm.init_from_env()
    a.gpus = world
    clock_helper = _clock_helper_start() if (world == 1 and not a.no_clock) else None      # (before anything here touches the GPU)

    from bnmtf_amd import _lib
    from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf

    w = WORKLOADS[a.workload]
    I, J, K, kind = w["I"], w["J"], w["K"], w["kind"]
    if kind in ("bnmtf", "trivb"):
        R, M, _, _, _ = generate_bnmtf(I, J, K, w["L"], 0.1, seed_data=0, seed_mask=1)
    else:
        R, M, _, _ = generate_bnmf(I, J, K, 0.1, tau=1.0, seed_data=0, seed_mask=1)

    t_create = time.perf_counter()
    model = build_model(w, R, M, rank, world, local_rank, comm_id)
    t_create = time.perf_counter() - t_create
    h = model._handle()
    L = _lib.lib()

    def sync():
        _lib.check(L.bnmtf_sync(h))
        cp.barrier()

    def run(n, perf=None, samples=None):
        s = samples or (None, None, None)
        if kind == "bnmf":
            _lib.check(L.bnmf_gibbs_run(h, n, _lib.UPDATE_DRAW, _lib.ptr(s[0]), _lib.ptr(s[1]), None, _lib.ptr(perf), None))
        elif kind == "bnmtf":
            _lib.check(L.bnmtf_gibbs_run(h, n, _lib.UPDATE_DRAW, _lib.ptr(s[0]), _lib.ptr(s[2]), _lib.ptr(s[1]), None, _lib.ptr(perf), None))
        elif kind == "trivb":
            _lib.check(L.bnmtf_vb_run(h, n, _lib.ptr(tri_orders[:n]), None, _lib.ptr(perf), None, None))
        else:
            _lib.check(L.bnmf_vb_run(h, n, None, _lib.ptr(perf), None, None))

    # the reference's run() hands every sample to the host (all_U[it], all_V[it]): the timed loop does too -- page-locked
    # arrays of one region's samples (re-used by every timed region), asynchronous copies behind the compute stream
    with_samples = kind not in ("vb", "trivb") and not a.no_samples
    sizes = _regions(a.steps, a.repeats, 4 * (I * K + J * w.get("L", K) + (K * w["L"] if kind == "bnmtf" else 0)) if with_samples else 0)
    tri_orders = None
    if kind == "trivb":           # the three shuffles of every iteration, drawn the reference's way (bnmtf_vb_optimised.py:171-186): reused by every region
        import random as _random
        _random.seed(1)
        tri_orders = np.ascontiguousarray(model._draw_orders(max(sizes[0], a.warmup, 50)))
    bufs = None
    if with_samples:
        if kind == "bnmf":
            bufs = (_lib.sample_buffer((sizes[0], I, K)), _lib.sample_buffer((sizes[0], J, K)), None)
        else:
            bufs = (_lib.sample_buffer((sizes[0], I, K)), _lib.sample_buffer((sizes[0], J, w["L"])), _lib.sample_buffer((sizes[0], K, w["L"])))
    trajectory = []
    perf_w = np.zeros((max(a.warmup, 1), 3))
    if a.warmup > 0:
        run(a.warmup, perf_w)
        trajectory += [float(x) for x in perf_w[:a.warmup, 0]]
    # one untimed pass over the page-locked sample arrays: the device's first write to a fresh pinned page is slow (the first
    # timed region ran at 600-1 700 instead of 2 400 it/s), and the arrays are re-used by every timed region
    if with_samples:
        perf_t = np.zeros((sizes[0], 3))
        run(sizes[0], perf_t, samples=bufs)
        trajectory += [float(x) for x in perf_t[:, 0]]
    # timed regions: HIP events bracket the roofline kernel only, on its own stream, in every fourth iteration (an event
    # record drains the queue for ~4 us: two per iteration were 2 % of the headline iteration)
    # (BNMTF: the cols direction's contraction is no pass over R~ any more -- (R~^T F) S from the S step's slabs -- so the
    # roofline kernel there is the rows direction's, R~ . (G S^T))
    # (bnmtf_vb: its rows-side pass over R~ runs on a second stream beside the S pass since round 6 -- the timed one is R~^T E[F])
    ROOF = _lib.KERNEL_GEMM_ROWS if kind == "bnmtf" else _lib.KERNEL_GEMM_COLS
    model.set_profiling(True, kernel=ROOF, every=4)
    perf_first = None
    dts = []
    # (the regions together are EXACTLY --steps iterations, each between two barriers; a region's time is the max over the ranks)
    for n in sizes:
        perf = np.zeros((n, 3))
        sync()
        t0 = time.perf_counter()
        run(n, perf, samples=bufs)
        sync()
        dts.append(cp.allreduce_max(time.perf_counter() - t0))
        if len(trajectory) < 400:
            trajectory += [float(x) for x in perf[:, 0]]
        if perf_first is None:
            perf_first = perf
    dt = float(sum(dts))
    if with_samples:
        assert np.isfinite(bufs[0][sizes[-1] - 1]).all() and float(np.abs(bufs[0][sizes[-1] - 1]).max()) > 0.0
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, model_outputs(model, kind, perf[-1]))

    names = {_lib.KERNEL_GEMM_ROWS: "gemm_rows(R~.V)", _lib.KERNEL_GEMM_COLS: "gemm_cols((R~^T.F).S from the S step's slabs)" if kind == "bnmtf" else "gemm_cols(R~^T.U)",
             _lib.KERNEL_SWEEP_ROWS: "sweep_rows", _lib.KERNEL_SWEEP_COLS: "sweep_cols"}
    if kind == "bnmtf":
        names[_lib.KERNEL_SWEEP_S] = "sweep_S"
    stats = {}
    ms, n = model.kernel_stats(ROOF)
    stats[names[ROOF]] = {"avg_us": 1e3 * ms / max(n, 1), "launches": n}
    # the other kernels of the iteration: a short untimed run with every timer on
    model.set_profiling(True)
    run(min(a.steps, 10))
    sync()
    for kid, nm in names.items():
        if kid == ROOF:
            continue
        ms, n = model.kernel_stats(kid)
        stats[nm] = {"avg_us": 1e3 * ms / max(n, 1), "launches": n}
    model.set_profiling(False)

    # the same loop with the samples left on the device (what round 1 and 2 reported as `value`)
    resident = None
    if with_samples:
        run(2)
        sync(); t1 = time.perf_counter()
        run(sizes[0])
        sync(); resident = sizes[0] / cp.allreduce_max(time.perf_counter() - t1)

    # what the box sustains under this loop: the pool's boxes differ by +-5 % in rate, and that spread is the shader clock
    # (~861 k cycles per iteration of the headline on either kind) -- rocm-smi read a few times beside ~2 s of the
    # device-resident loop, after everything that is timed; None when rocm-smi is not there or says nothing
    clock = _clock_beside(clock_helper, lambda: run(max(sizes[0], 50) if kind != "trivb" else min(max(sizes[0], 50), len(tri_orders))), sync) if clock_helper is not None else None

    import ctypes as C_
    ck, cr = C_.c_int(), C_.c_int()
    _lib.check(L.bnmtf_comm_info(h, C_.byref(ck), C_.byref(cr)))
    # the CPU leg LAST (round 5's review: an observer's busy trace should show the GPU legs first): the oracle on the host cores,
    # rank 0 of a single-GPU run only, a bounded sample of the same workload (or, --cpu-whole-iteration, one whole iteration)
    cpu = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        cpu = cpu_baseline(w, R, M, whole=a.cpu_whole_iteration)
        if kind == "bnmf":
            cpu["mse_vs_iter_small"] = small_trajectories()
    if rank == 0:
        Wc = w.get("L", K)                 # width of the cols-direction contraction's factor operand is K (F or U)
        ms_step = 1e3 * dt / a.steps
        rates = [n / d for n, d in zip(sizes, dts)]
        # dominant HBM kernel, "the U^T.R step" (SURVEY.md 8(d)): algorithmic 4*I*J bytes (R~ read once) and 2*I*J*K flop
        # per launch (per rank: its column shard); fp32-exact products on the bf16 matrix cores (3-term splits), so a
        # stream of R~ from HBM
        g = stats[names[ROOF]]
        flops = 2.0 * I * (J / world) * K
        bytes_alg = 4.0 * I * (J / world)
        f32_gemm = os.environ.get("BNMTF_GEMM") == "f32"
        t_mfma = (4.0 * I * J * K / (PEAK_F32_VECTOR_TFLOPS * 1e12) if f32_gemm else 6 * 4.0 * I * J * K / (PEAK_BF16_MFMA_TFLOPS * 1e12)) / world
        t_hbm = (2.0 * I * J * 4.125 + 8.0 * (I + J) * K) / (PEAK_HBM_GBS * 1e9) / world
        traffic, traffic_note = None, None
        try:     # HBM bytes per launch of this kernel from the committed rocprofv3 PMC passes (profiles/traffic.json);
            tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))   # only for the build they were measured on
            lib_md5 = hashlib.md5(open(_lib.LIB_PATH, "rb").read()).hexdigest()
            e = tj.get(a.workload)
            if e and world == 1:
                if e.get("lib_md5") == lib_md5:
                    traffic = e["hbm_bytes_per_launch"]
                traffic_note = {"kernel": e.get("kernel"), "measured_lib_md5": e.get("lib_md5"), "this_lib_md5": lib_md5}
        except Exception:
            pass
        if f32_gemm:
            ach = flops / (g["avg_us"] * 1e-6) / 1e12 if g["avg_us"] > 0 else 0.0
            roof = {"bound": "mfma", "kernel": "gemm_cols: Pv = R~^T.U (f32 MFMA 32x32x2)", "achieved": ach, "peak": PEAK_F32_VECTOR_TFLOPS,
                    "unit": "TFLOP/s", "frac": ach / PEAK_F32_VECTOR_TFLOPS, "traffic": None}
        else:
            ach = bytes_alg / (g["avg_us"] * 1e-6) / 1e9 if g["avg_us"] > 0 else 0.0
            roof = {"bound": "hbm", "kernel": ("gemm_rows: P = R~.(G S^T)" if kind == "bnmtf" else ("gemm_cols: Pv = R~^T.E[F]" if kind == "trivb" else "gemm_cols: Pv = R~^T.U")) + " (bf16x3 MFMA 32x32x16, fp32-exact products)", "achieved": ach,
                    "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": ach / PEAK_HBM_GBS, "traffic": traffic}
        roof.update({"algorithmic_per_launch": {"flop": flops, "bytes": bytes_alg,
                                                "bytes_note": "4 B per element: the operand is the PRE-MASKED R~ = M.R (fp32, built once at create), so a launch reads no mask; "
                                                              "SURVEY 8(d)'s 4.125 B (fp32 R + 1-bit mask) would credit bytes this kernel does not move: x 1.031 for that convention"},
                     "avg_launch_us": g["avg_us"], "traffic_source": traffic_note})
        # what makes a rate comparable between the boxes of a pool (their sustained shader clock differs by +-5 %, and the iteration
        # follows it): the clock read beside the loop, the iteration in shader cycles, and the times of the other kernels of the
        # iteration -- inside `roofline`, the object a reader of the bench record keeps
        sclk = clock["sclk_mhz_median"] if clock else None
        roof.update({"sclk_mhz": sclk, "power_w": clock["power_w_median"] if clock else None,
                     "cycles_per_iteration": None if sclk is None else sclk * ms_step * 1e3,
                     "cycles_per_iteration_device_resident": None if (sclk is None or resident is None) else sclk * 1e6 / resident,
                     "timed_seconds": float(sum(dts)), "timed_regions": len(dts),
                     "kernels_us": {nm: round(v["avg_us"], 2) for nm, v in stats.items()},
                     "iteration_frac_of_bound": max(t_mfma, t_hbm) / (dt / a.steps)})
        # the sweep kernels (K sequential conditional updates per unit) are bound by vector issue + LDS gathers, not by HBM
        # or the matrix cores: algorithmic fp32 work per launch = 8 flop per (missing entry, column) -- the q rebuild
        # (1 FMA), sum q.v, sum v^2 and the q update (3 FMAs) -- against the fp32 vector peak
        nmiss = float(I) * J - float(np.count_nonzero(M))
        sw = stats.get("sweep_cols", {"avg_us": 0.0})
        sweep_flop = 8.0 * nmiss * Wc / world
        sweep_ach = sweep_flop / (sw["avg_us"] * 1e-6) / 1e12 if sw["avg_us"] > 0 else 0.0
        out = {
            "metric": {"bnmf": "Gibbs iterations/sec (BNMF, I=J=%d, K=%d)", "bnmtf": "Gibbs iterations/sec (BNMTF, I=J=%d, K=L=%d)",
                       "vb": "VB iterations/sec (BNMF VB, I=J=%d, K=%d)", "trivb": "VB iterations/sec (BNMTF VB, I=J=%d, K=L=%d)"}[kind] % (I, K),
            "value": a.steps / dt, "unit": "iterations/s" if kind in ("vb", "trivb") else "Gibbs iterations/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": ms_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s, synthetic R %dx%d K=%d%s, 10%% missing mask, priors alpha=beta=1 lambda=0.1, init %s" % (
                           {"bnmf": "BNMF Gibbs", "bnmtf": "BNMTF Gibbs", "vb": "BNMF VB", "trivb": "BNMTF VB (bnmtf_vb_optimised, shuffled update orders)"}[kind], I, J, K, " L=%d" % w["L"] if "L" in w else "",
                           "exp" if kind == "vb" else "random"),
                       "parallelism": "rows/cols split x%d, RCCL all-gather of factor blocks" % world if world > 1 else "single GPU",
                       "rccl_ranks": int(cr.value) if ck.value == 1 else 0,
                       "communicator": {0: "none", 1: "rccl", 2: "in-process"}[int(ck.value)] + " (%d ranks by its own count, world %d)" % (cr.value, world),
                       "samples": ("handed to the host every iteration (all_U/all_V: %.1f MiB per iteration, page-locked arrays, copy stream)" % (
                                       4.0 * (I * K + J * Wc + (K * Wc if kind == "bnmtf" else 0)) / 2 ** 20)) if with_samples else
                                  ("none (the variational run() stores no samples)" if kind in ("vb", "trivb") else "device-resident (--no-samples)")},
            "repeats": {"n": len(dts), "timed_seconds": dt, "values": [n / d for n, d in zip(sizes[:40], dts)], "min": min(rates), "median": float(np.median(rates)), "max": max(rates)},
            "device_resident": None if resident is None else {"value": resident, "unit": "iterations/s", "what": "same loop, samples left on the device"},
            "clock": clock,
            "roofline": roof,
            "roofline_sweep": {"bound": "valu", "kernel": "sweep_cols: K sequential conditional updates per unit (LDS gathers + fp32 vector FMAs)",
                               "achieved": sweep_ach, "peak": PEAK_F32_VECTOR_TFLOPS, "unit": "TFLOP/s", "frac": sweep_ach / PEAK_F32_VECTOR_TFLOPS,
                               "algorithmic_per_launch": {"flop": sweep_flop, "lds_gather_bytes": 8.0 * nmiss * Wc / world}, "avg_launch_us": sw["avg_us"]},
            "iteration_bound": {"t_mfma_us": 1e6 * t_mfma, "t_hbm_us": 1e6 * t_hbm, "frac_of_bound": max(t_mfma, t_hbm) / (dt / a.steps)},
            "kernels": stats,
            "create_s": t_create,
            "mse_first_last": [float(perf_first[0, 0]), float(perf[-1, 0])],
            "mse_trajectory": {"what": "masked MSE on the training mask after each iteration of this run, from iteration 1 (warm-up and the untimed sample pass included), first %d" % min(len(trajectory), 200),
                               "values": trajectory[:200]},
            "cpu_baseline": cpu,
        }
        print(json.dumps(out))
        sys.stdout.flush()
    cp.barrier()
    model.close()
    cp.close()


if __name__ == "__main__":
    main()
