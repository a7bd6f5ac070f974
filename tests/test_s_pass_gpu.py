"""The variational S pass (csrc/kernel_trivb.hip: ssys_chain_vb_kernel, ssys_chain_vb_blocked_kernel; device_rng.h:
tn_moments_f32, tn_mean_f32_regime; tn_mean_table.h) checked step by step in every regime and at every launch shape.

run(1, orders=...) on a pushed state: the S pass is the first thing of an iteration (api_trivb.inc: enqueue_trivb_iteration;
api_obs_trivb.inc on the observed-entry layout), so muS, tauS, expS, varS afterwards are the pass's results.  The system is exact
and every step's regime is steered through lambdaS (tests/_s_pass_cases.py, where the checks and their bounds are derived; the CPU
side, test_s_pass_cases_cpu.py, shows that a NumPy fp32 restatement of the kernels passes them and that one skipped fold, dropped
tail step, wrong row, stale LDS region, wrong segment, wrong threshold or missing fall-back fails them).  Every entry of every case:
 (a) expS, varS against the fp64 moments of the returned (muS, tauS): rtol 2e-6 / 5e-6;
 (b) tauS bit for bit and muS explained, within a running rounding bound, by the device's own E of the earlier steps.
Each test prints its largest difference / bound ratio."""
import os

import numpy as np
import pytest

import _s_pass_cases as SP
from bnmtf_amd import bnmtf_vb_observed, bnmtf_vb_optimised
from _s_pass_cases import CASES, HOOK_SHAPE, HOOK_TAUS, OBSERVED_CASES

pytestmark = pytest.mark.gpu

LAM_FG = 0.5


@pytest.fixture(scope="module", autouse=True)
def conditions_over_all_shapes():
    assert "BNMTF_VB_CHAIN" not in os.environ          # (=steps would send every pass to the barrier-per-step kernel)
    SP.global_coverage()


def _model(K, L, lam, layout="dense"):
    p, st, s = SP.system(K, L)
    assert s.ok.all()
    pri = dict(alpha=1., beta=1., lambdaF=LAM_FG, lambdaS=np.asarray(lam, np.float64), lambdaG=LAM_FG)
    cls = bnmtf_vb_observed if layout == "observed" else bnmtf_vb_optimised
    return cls(p.R, p.M, K, L, pri, verbose=False), p, st


def _set_state(model, p, st, tau):
    I, J = p.R.shape
    K, L = st.S.shape
    model.expF, model.varF = st.F.astype(np.float64), st.varF.astype(np.float64)
    model.expG, model.varG = st.G.astype(np.float64), st.varG.astype(np.float64)
    model.expS, model.varS = st.S.astype(np.float64), np.ones((K, L))
    for n, shape in (("muF", (I, K)), ("tauF", (I, K)), ("muG", (J, L)), ("tauG", (J, L)), ("muS", (K, L)), ("tauS", (K, L))):
        setattr(model, n, np.ones(shape))
    model.exptau = float(tau)


def _run_pass(case):
    steer = SP.case_conditions(case)
    model, p, st = _model(case.K, case.L, steer.lam, case.layout)
    try:
        _set_state(model, p, st, case.tau)
        model.run(1, orders=SP.orders_row(case))
        got = [np.array(getattr(model, n)) for n in ("muS", "tauS", "expS", "varS")]
    finally:
        model.close()
    (ra_e, ra_v, rb), fails = SP.check_all(case, steer.lam, *got)
    print("%s (%s kernel): largest difference / bound  (a) mean %.3f variance %.3f  (b) %.3f" % (case.id, case.kernel, ra_e, ra_v, rb))
    assert not fails, fails


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pass_step_by_step(case):
    _run_pass(case)


@pytest.mark.parametrize("case", OBSERVED_CASES, ids=[c.id for c in OBSERVED_CASES])
def test_pass_step_by_step_observed_layout(case):
    """api_obs_trivb.inc's own permute and chain enqueue (the system built from the entry lists)"""
    _run_pass(case)


@pytest.mark.parametrize("tau", HOOK_TAUS, ids=["tau2^%d" % int(np.log2(t)) for t in HOOK_TAUS])
def test_single_step_hook_over_a_grid_of_x(tau):
    """update_S(k, l) with update_exp_S(k, l) on the device: bnmtf_vb_update(which = 1, moments = 1) -- the barrier-per-step kernel
    with one step, its x <= -6 shortcut and tn_moments_f32 -- each entry from the same pushed state, steered to
    x in {-40, -12, -6 -+ 1e-3, -1e-3, 0, 1e-3, 3, 12, 25.9, 26.1, 29.9, 30.1, 35}, tauS from below 2^-10 to above 2^20 over the
    exptau's.  Check (a).  (The class's update_exp_S forms the moments with the fp64 routine on what update_S returned; the
    one-call form is the model's own _update.)"""
    K, L = HOOK_SHAPE
    lam, x, tauS = SP.hook_lambda(tau)
    model, p, st = _model(K, L, lam)
    mu, tq, E, V = (np.zeros(K * L) for _ in range(4))
    try:
        for k in range(K):
            for l in range(L):
                _set_state(model, p, st, tau)
                model._update(1, k, l, 1)
                a = k * L + l
                mu[a], tq[a], E[a], V[a] = model.muS[k, l], model.tauS[k, l], model.expS[k, l], model.varS[k, l]
    finally:
        model.close()
    assert np.array_equal(tq, tauS.astype(np.float32).astype(np.float64))
    ra_e, ra_v, bad = SP.check_moments(mu, tq, E, V)
    xd = -mu * np.sqrt(tq)
    print("exptau 2^%d: tauS %.3g .. %.3g, x %s: largest difference / bound  (a) mean %.3f variance %.3f" % (
        int(np.log2(tau)), tq.min(), tq.max(), np.round(xd, 4).tolist(), ra_e, ra_v))
    assert bad.size == 0, "entries %s: x %s, E %s, Var %s" % (bad.tolist(), xd[bad].tolist(), E[bad].tolist(), V[bad].tolist())
