"""layout='observed' of bnmf_gibbs_optimised / nmf_icm (csrc/kernel_obs.hip) on the device: the residual kept
on the observed entries, against the fp64 oracle, the reference's golden vectors and the dense layout.

Tolerances are the project's own: tau* rel 2e-6; mu* abs 2e-5 x the size of the cancelling terms; masked
SSE / MSE rel 2e-5; mode-update trajectories rel 5e-4 (factors: of their scale, at least 1); with draws and the same seed, more
than 99 % of the first sweep's elements within 1e-3; fp64 device sums against NumPy: RTOL of tests/test_heldout_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import bnmf_gibbs_optimised, nmf_icm
from bnmtf_amd._base import metrics_from_sums
from bnmtf_amd.synthetic import generate_bnmf
from oracle import bnmtf_oracle as O

from _obs_cases import PRI, SHAPES, _mode_iteration

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9                      # tests/test_heldout_gpu.py
SEED_DATA, SEED_MASK = 3, 0      # generate_bnmf(97, 83, 5) at 90 % missing: the mask of seed 0 leaves no row or column empty


def _pri(c):
    return dict(alpha=float(c["alpha"]), beta=float(c["beta"]), lambdaU=c["lambdaU"], lambdaV=c["lambdaV"])


def _mu_scale(M, R, U, V, tau, k, rows=True):
    """magnitude of the terms that cancel inside the numerator of mu (tests/test_bnmf_gibbs_gpu.py)"""
    if rows:
        return tau * ((M * np.abs(R)) @ np.abs(V[:, k]) + np.abs(U) @ np.abs(V.T @ V[:, k]))
    return tau * ((M * np.abs(R)).T @ np.abs(U[:, k]) + np.abs(V) @ np.abs(U.T @ U[:, k]))


def _sparse_problem():
    R, M, _, _ = generate_bnmf(97, 83, 5, 0.9, seed_data=SEED_DATA, seed_mask=SEED_MASK)
    M = M.astype(float)
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0 and M.sum() == 97 * 83 - int(0.9 * 97 * 83)
    rs = np.random.RandomState(17)
    return R.astype(np.float64), M, rs.exponential(0.5, (97, 5)), rs.exponential(0.5, (83, 5))


# ---------------------------------------------------------------- 1. known answers
def test_known_answers_of_the_reference_on_its_5x3_matrix(golden):
    """tests/code/test_bnmf_gibbs_optimised.py:144-203 on the observed-entry kernel, and the golden case of the same shape."""
    I, J, K = 5, 3, 2
    R = np.ones((I, J)); M = np.ones((I, J)); M[0, 0] = M[2, 2] = M[3, 1] = 0
    pri = dict(alpha=3, beta=1, lambdaU=2 * np.ones((I, K)), lambdaV=3 * np.ones((J, K)))
    b = bnmf_gibbs_optimised(R, M, K, pri, verbose=False, layout='observed')
    b.initialise('exp')
    assert (b.U == 0.5).all() and (b.V == 1. / 3.).all() and b.tau >= 0.0
    assert b.alpha_s() == 3 + 6.
    assert abs(b.beta_s() - (1 + .5 * (12 * (2. / 3.) ** 2))) < 1e-6
    b.tau = 3.
    tauU = 3. * np.array([[2. / 9.] * 2, [1. / 3.] * 2, [2. / 9.] * 2, [2. / 9.] * 2, [1. / 3.] * 2])
    muU = 1. / tauU * (3. * np.array([[2. * (5. / 6.) * (1. / 3.), 10. / 18.], [15. / 18.] * 2, [10. / 18.] * 2, [10. / 18.] * 2, [15. / 18.] * 2]) - 2.)
    for k in range(K):
        assert np.abs(b.tauU(k) - tauU[:, k]).max() < 1e-6
        assert np.abs(b.muU(tauU[:, k], k) - muU[:, k]).max() < 1e-5
        assert np.abs(b.tauV(k) - 3.).max() < 1e-6
        assert np.abs(b.muV(3. * np.ones(J), k) - (1. / 3.) * (3. * 4. * (5. / 6.) * .5 - 3.)).max() < 1e-5
    b.close()
    c = golden("bnmf_gibbs_cond.npz").case("t5x3")
    assert c["R"].shape == (5, 3)
    b = bnmf_gibbs_optimised(c["R"], c["M"], int(c["K"]), _pri(c), verbose=False, layout='observed')
    b.U, b.V, b.tau = c["U"].copy(), c["V"].copy(), float(c["tau"])
    assert b.alpha_s() == float(c["alpha_s"])
    assert abs(b.beta_s() - float(c["beta_s"])) <= 2e-6 * abs(float(c["beta_s"]))
    for k in range(b.K):
        np.testing.assert_allclose(b.tauU(k), c["tauU"][k], rtol=2e-6)
        sc = _mu_scale(c["M"], c["R"], c["U"], c["V"], float(c["tau"]), k, True) / c["tauU"][k]
        assert (np.abs(b.muU(c["tauU"][k], k) - c["muU"][k]) <= 2e-5 * sc + 1e-6).all()
        np.testing.assert_allclose(b.tauV(k), c["tauV"][k], rtol=2e-6)
        sc = _mu_scale(c["M"], c["R"], c["U"], c["V"], float(c["tau"]), k, False) / c["tauV"][k]
        assert (np.abs(b.muV(c["tauV"][k], k) - c["muV"][k]) <= 2e-5 * sc + 1e-6).all()
    assert np.array_equal(b.U, c["U"]) and np.array_equal(b.V, c["V"])       # the hooks change nothing
    b.close()


@pytest.mark.parametrize("name", ["toy", "r37x29", "r40x33"])
def test_conditional_parameters_match_reference(golden, name):
    c = golden("bnmf_gibbs_cond.npz").case(name)
    b = bnmf_gibbs_optimised(c["R"], c["M"], int(c["K"]), _pri(c), verbose=False, layout='observed')
    b.U, b.V, b.tau = c["U"].copy(), c["V"].copy(), float(c["tau"])
    tot, row, col = b.omega_counts()
    assert tot == int(c["size_Omega"]) and np.array_equal(row, c["row_counts"]) and np.array_equal(col, c["col_counts"])
    assert abs(b.beta_s() - float(c["beta_s"])) <= 2e-6 * abs(float(c["beta_s"]))
    for k in range(b.K):
        np.testing.assert_allclose(b.tauU(k), c["tauU"][k], rtol=2e-6)
        sc = _mu_scale(c["M"], c["R"], c["U"], c["V"], float(c["tau"]), k, True) / c["tauU"][k]
        assert (np.abs(b.muU(c["tauU"][k], k) - c["muU"][k]) <= 2e-5 * sc + 1e-6).all()
        np.testing.assert_allclose(b.tauV(k), c["tauV"][k], rtol=2e-6)
        sc = _mu_scale(c["M"], c["R"], c["U"], c["V"], float(c["tau"]), k, False) / c["tauV"][k]
        assert (np.abs(b.muV(c["tauV"][k], k) - c["muV"][k]) <= 2e-5 * sc + 1e-6).all()
    b.close()


# ---------------------------------------------------------------- 2. mode trajectory
def test_mode_trajectory_follows_the_oracle_at_90_percent_missing():
    R, M, U0, V0 = _sparse_problem()
    o = O.BNMFGibbsOracle(R, M, 5, PRI)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(8, draw=False)
    b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, layout='observed')
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(8, update='mode')
    assert "layout=observed" in b.describe() and "entries=%d" % int(M.sum()) in b.describe()
    assert b.all_U.shape == (8, 97, 5) and b.all_V.shape == (8, 83, 5)
    for t in range(8):
        sU, sV = max(1.0, np.abs(o.all_U[t]).max()), max(1.0, np.abs(o.all_V[t]).max())
        assert np.abs(b.all_U[t] - o.all_U[t]).max() < 5e-4 * sU and np.abs(b.all_V[t] - o.all_V[t]).max() < 5e-4 * sV, t
    np.testing.assert_allclose(b.all_tau, o.all_tau, rtol=5e-4)
    for m in ("MSE", "R^2", "Rp"):
        np.testing.assert_allclose(b.all_performances[m], o.all_performances[m], rtol=5e-4, err_msg=m)
    assert np.allclose(b.U, b.all_U[-1]) and np.allclose(b.V, b.all_V[-1]) and abs(b.tau - b.all_tau[-1]) < 1e-12
    assert len(b.all_times) == 8 and all(np.diff(b.all_times) > 0)
    b.close()


def test_icm_follows_the_oracle_at_90_percent_missing():
    R, M, U0, V0 = _sparse_problem()
    o = O.NMFICMOracle(R, M, 5, PRI)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(6, minimum_TN=0.05)
    b = nmf_icm(R, M, 5, PRI, verbose=False, layout='observed')
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    assert b.run(6, minimum_TN=0.05) is None
    np.testing.assert_allclose(b.all_tau, o.all_tau, rtol=5e-4)
    np.testing.assert_allclose(b.all_performances["MSE"], o.all_performances["MSE"], rtol=5e-4)
    assert np.abs(b.U - o.U).max() < 5e-4 * max(1.0, np.abs(o.U).max()) and np.abs(b.V - o.V).max() < 5e-4 * max(1.0, np.abs(o.V).max())
    assert (b.U >= 0.05 * (1 - 1e-6)).all() and (b.V >= 0.05 * (1 - 1e-6)).all()
    b.close()


@pytest.mark.parametrize("name", ["nmf_conv", "nmf_min", "nmf_collapse"])
def test_nmf_icm_trajectory_matches_reference(golden, name):
    """tests/test_icm_gpu.py's comparison with the reference's own trajectories (tests/golden/icm.npz), same bounds."""
    c = golden("icm.npz").case(name)
    t = golden("toy_data.npz").case("bnmf")
    K, lam, mtn, iters = int(c["cfg"][0]), float(c["cfg"][1]), float(c["cfg"][2]), int(c["cfg"][3])
    b = nmf_icm(t["R"], t["M"], K, dict(alpha=1.0, beta=1.0, lambdaU=lam, lambdaV=lam), verbose=False, layout='observed')
    b.initialise("exp")
    b.U, b.V = c["U0"].copy(), c["V0"].copy()
    b.tau = (b.alpha_s() - 1) / b.beta_s()
    assert b.tau == pytest.approx(float(c["tau0"]), rel=2e-5)
    assert b.run(iters, minimum_TN=mtn) is None
    np.testing.assert_allclose(b.all_tau, c["all_tau"], rtol=5e-4)
    np.testing.assert_allclose(b.all_performances["MSE"], c["mse"], rtol=5e-4)
    np.testing.assert_allclose(b.all_performances["R^2"], c["r2"], rtol=5e-4, atol=1e-4)
    sU, sV = max(np.abs(c["U"]).max(), 1e-3), max(np.abs(c["V"]).max(), 1e-3)
    assert np.abs(b.U - c["U"]).max() <= 2e-3 * sU and np.abs(b.V - c["V"]).max() <= 2e-3 * sV
    if mtn > 0:
        assert b.U.min() >= mtn * (1 - 1e-6) and b.V.min() >= mtn * (1 - 1e-6)
    q = [b.quality(m) for m in ["loglikelihood", "BIC", "AIC", "MSE", "ELBO"]]
    np.testing.assert_allclose(q, c["quality"], rtol=1e-3)
    p = b.predict(c["Mpred"])
    np.testing.assert_allclose([p["MSE"], p["R^2"]], c["pred"][:2], rtol=1e-3, atol=1e-4)
    b.close()


# ---------------------------------------------------------------- 3. draws
def test_first_drawn_sweep_follows_the_oracle_and_the_dense_layout():
    R, M, U0, V0 = _sparse_problem()
    o = O.BNMFGibbsOracle(R, M, 5, PRI, seed=77)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(1)
    runs = {}
    for layout in ('observed', 'dense'):
        b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, seed=77, layout=layout)
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
        b.run(2)
        runs[layout] = (b.all_U.copy(), b.all_V.copy(), b.all_tau.copy(), list(b.all_performances['MSE']))
        b.close()
    got = runs['observed']
    for dev, ora in ((got[0][0], o.all_U[0]), (got[1][0], o.all_V[0]), (got[0][0], runs['dense'][0][0]), (got[1][0], runs['dense'][1][0])):
        d = np.abs(dev - ora) / (1e-3 + np.abs(ora))
        print("first sweep: share within 1e-3 = %.4f" % np.mean(d < 1e-3))
        assert np.mean(d < 1e-3) > 0.99
    print("MSE[0]: observed %.9g dense %.9g oracle %.9g" % (got[3][0], runs['dense'][3][0], o.all_performances['MSE'][0]))
    assert abs(got[3][0] / o.all_performances['MSE'][0] - 1) < 1e-5
    assert abs(got[3][0] / runs['dense'][3][0] - 1) < 1e-5
    assert abs(got[2][0] / o.all_tau[0] - 1) < 1e-3
    assert (got[0] >= 0).all() and (got[1] >= 0).all() and (got[2] > 0).all()


# ---------------------------------------------------------------- 4. launch shapes
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_launch_shapes_match_the_oracle(shape):
    M, K = SHAPES[shape]()
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0
    R, U0, V0, (U1, V1, tau1, perf, desc) = _mode_iteration(M, K)
    o = O.BNMFGibbsOracle(R, M, K, PRI)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(1, draw=False)
    if shape in ("row_counts", "col_counts", "full_matrix_long"):
        assert "long_form_units=%s" % {"row_counts": "3/0", "col_counts": "0/3", "full_matrix_long": "3/0"}[shape] in desc, desc
    else:
        assert "long_form_units=0/0" in desc, desc
    eU = np.abs(U1 - o.all_U[0]).max() / max(1.0, np.abs(o.all_U[0]).max()); eV = np.abs(V1 - o.all_V[0]).max() / max(1.0, np.abs(o.all_V[0]).max())
    print("%s: U %.2e V %.2e tau %.2e MSE %.2e" % (shape, eU, eV, abs(tau1 / o.all_tau[0] - 1), abs(perf[0] / o.all_performances["MSE"][0] - 1)))
    assert eU < 5e-4 and eV < 5e-4
    assert abs(tau1 / o.all_tau[0] - 1) < 5e-4
    assert abs(perf[0] / o.all_performances["MSE"][0] - 1) < 5e-4
    # the record's metrics are those of the stored sample (fp64 NumPy on the fp32 factors): masked SSE / MSE rel 2e-5
    want = metrics_from_sums(O.metric_sums(M, R, U1.astype(np.float64) @ V1.astype(np.float64).T))
    assert abs(perf[0] / want["MSE"] - 1) < 2e-5


# ---------------------------------------------------------------- 5. one form, one result
_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
from _obs_cases import SHAPES, _mode_iteration, _draw_iterations
out = {}
for shape in ("row_counts", "col_counts"):         # long units in the U half sweep, then in the V half sweep (and its end-of-iteration sums)
    M, K = SHAPES[shape]()
    _, _, _, (U1, V1, tau1, perf, desc) = _mode_iteration(M, K)
    d = _draw_iterations(M, K)
    assert ("force_long=1" in desc) == (%r == "1"), desc
    assert ("long_form_units=3/0" if shape == "row_counts" else "long_form_units=0/3") in desc, desc
    out.update({shape + "_" + k: v for k, v in dict(U1=U1, V1=V1, tau1=tau1, perf=np.array(perf), dU=d[0], dV=d[1], dtau=d[2], dperf=d[3]).items()})
np.savez(sys.argv[1], **out)
"""


def _child_run(tmp_path, force_long, tag):
    env = dict(os.environ)
    env.pop("BNMTF_OBS_LONG", None)
    if force_long:
        env["BNMTF_OBS_LONG"] = "1"
    out = str(tmp_path / ("run_%s.npz" % tag))
    subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), "1" if force_long else "0"), out], check=True, env=env, cwd=ROOT, timeout=300)
    return np.load(out)


def test_long_form_and_register_form_give_the_same_bits(tmp_path):
    """BNMTF_OBS_LONG=1 (every unit down the long form) in a fresh child process against two default runs, on the matrices of the
    row-count and column-count shapes (long units in the U and in the V half sweep): one mode iteration and three drawn ones each."""
    a = _child_run(tmp_path, False, "a")
    b = _child_run(tmp_path, False, "b")
    c = _child_run(tmp_path, True, "long")
    for key in a.files:
        assert np.array_equal(a[key], b[key]), "two default runs differ in %s" % key
        assert np.array_equal(a[key], c[key]), "the long form differs from the default in %s" % key
    assert len(a.files) == 16 and len(set(a["row_counts_dperf"][0])) == 3 and len(set(a["col_counts_dperf"][0])) == 3


# ---------------------------------------------------------------- 6. per-iteration metrics
@pytest.mark.parametrize("update", ["draw", "mode"])
def test_every_iterations_metrics_are_those_of_its_sample(update):
    R, M, U0, V0 = _sparse_problem()
    b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, layout='observed', seed=9)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(6, update=update)
    for t in range(6):
        want = metrics_from_sums(O.metric_sums(M, R, b.all_U[t].astype(np.float64) @ b.all_V[t].astype(np.float64).T))
        assert abs(b.all_performances["MSE"][t] / want["MSE"] - 1) < 2e-5, t
        assert abs(b.all_performances["R^2"][t] - want["R^2"]) < 2e-5 and abs(b.all_performances["Rp"][t] - want["Rp"]) < 2e-5, t
    assert len(set(b.all_performances["MSE"])) == 6
    b.close()


# ---------------------------------------------------------------- 7. post-run API
def _mpred_cases(M):
    I, J = M.shape
    one = np.zeros((I, J)); one[3, 4] = 1
    row = np.zeros((I, J)); row[5, :] = 1
    rs = np.random.RandomState(4)
    over = ((rs.rand(I, J) < 0.1) | ((M != 0) & (rs.rand(I, J) < 0.3))).astype(float)        # missing and observed entries
    return {"one_entry": one, "full_row": row, "overlapping_M": over}


def test_postrun_api_equals_the_dense_layouts():
    R, M, _, _ = _sparse_problem()
    rs = np.random.RandomState(8)
    all_U = [rs.exponential(0.6, (97, 5)) for _ in range(10)]
    all_V = [rs.exponential(0.6, (83, 5)) for _ in range(10)]
    all_tau = list(rs.uniform(0.5, 2.0, 10))
    models = {}
    for layout in ('observed', 'dense'):
        b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, layout=layout)
        b.all_U, b.all_V, b.all_tau = list(all_U), list(all_V), list(all_tau)
        models[layout] = b
    o, d = models['observed'], models['dense']
    for got, want in zip(o.approx_expectation(2, 3), d.approx_expectation(2, 3)):
        assert np.array_equal(got, want)
    for name, Mp in _mpred_cases(M).items():
        po, pd = o.predict(Mp, 2, 3), d.predict(Mp, 2, 3)
        # (one entry: R^2 and Rp are 0 / 0 up to the rounding of the sums, in either layout -- only the MSE is a number to compare)
        for m in (("MSE",) if name == "one_entry" else ("MSE", "R^2", "Rp")):
            assert np.isfinite(pd[m]), (name, m)
            np.testing.assert_allclose(po[m], pd[m], rtol=RTOL, err_msg="%s %s" % (name, m))
    for metric in ("loglikelihood", "BIC", "AIC", "MSE", "ELBO"):
        np.testing.assert_allclose(o.quality(metric, 2, 3), d.quality(metric, 2, 3), rtol=RTOL, err_msg=metric)
    # against NumPy in fp64 too: the list-metric kernel's six sums
    eU, eV, _ = o.approx_expectation(2, 3)
    Mp = _mpred_cases(M)["overlapping_M"]
    np.testing.assert_allclose(o._metric_sums(Mp, eU, None, eV), O.metric_sums(Mp, R.astype(np.float32).astype(np.float64), eU @ eV.T), rtol=RTOL)
    with pytest.raises(AssertionError) as e:
        o.predict(2 * np.ones_like(M), 2, 3)
    assert str(e.value) == "The indicator matrix M_pred must contain only 0 and 1."
    o.close(); d.close()


# ---------------------------------------------------------------- 8. continuation and isolation
@pytest.mark.parametrize("update", ["draw", "mode"])
def test_run_3_then_4_equals_run_7(update):
    R, M, U0, V0 = _sparse_problem()
    res = []
    for parts in ((7,), (3, 4)):
        b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, layout='observed', seed=31)
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
        Us, Vs, taus, mse = [], [], [], []
        for n in parts:
            b.run(n, update=update)
            Us.append(b.all_U.copy()); Vs.append(b.all_V.copy()); taus.append(b.all_tau.copy()); mse += list(b.all_performances["MSE"])
        res.append((np.concatenate(Us), np.concatenate(Vs), np.concatenate(taus), np.array(mse), b.U.copy(), b.V.copy(), b.tau))
        assert "layout=observed" in b.describe()
        b.close()
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)


def test_a_dense_model_is_untouched_by_an_observed_one_in_the_same_process():
    R, M, U0, V0 = _sparse_problem()

    def dense():
        b = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, seed=13)
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
        b.run(4)
        out = (b.all_U.copy(), b.all_V.copy(), b.all_tau.copy(), np.array(b.all_performances["MSE"]))
        assert "layout=observed" not in b.describe()
        b.close()
        return out

    before = dense()
    ob = bnmf_gibbs_optimised(R, M, 5, PRI, verbose=False, seed=13, layout='observed')
    ob.U, ob.V, ob.tau = U0.copy(), V0.copy(), 1.3
    ob.run(4)
    during = dense()                      # (the observed model is still alive)
    ob.run(2)
    ob.close()
    after = dense()
    for x, y, z in zip(before, during, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)
