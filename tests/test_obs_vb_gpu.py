"""bnmf_vb_observed (csrc/kernel_obs_vb.hip) on the device: the variational two-factor model with the
residual kept on the observed entries, against the fp64 oracle on every launch shape of the observed-entry sweep, the
reference's golden trajectories and known answers, the dense class, and itself (one result whatever the form or the split).

Tolerances are the project's own.  One iteration on the launch shapes: 5e-4 (tests/test_obs_gpu.py::
test_launch_shapes_match_the_oracle), factors scaled by max(1, max|ref|); masked SSE / MSE against fp64 NumPy on the returned
expectations rel 2e-5; the ELBO of the first iterations rel 2e-5, of a trajectory 2e-4; MSE and exptau of a trajectory 1e-3
(tests/test_bnmf_vb_gpu.py); tau of a hook rel 2e-6; exp_square_diff of a set state rel 2e-6."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from bnmtf_amd import bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised
from bnmtf_amd._base import metrics_from_sums
from oracle import bnmtf_oracle as O

from _obs_cases import PRI, SHAPES, _problem
from _obs_vb_cases import EXPTAU0, NAMES, seed_state, vb_model, vb_problem, vb_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_UNITS = {"row_counts": "3/0", "col_counts": "0/3", "full_matrix_long": "3/0"}
# after one sweep the oracle's ELBO is -inf exactly on these: the fp64 erfc underflows at mu sqrt(tau) of -7 .. -13
UNDERFLOW = ("K63", "K64", "K65", "K130")


def _scaled(got, ref):
    return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())


def _oracle(R, M, K, state, exptau=EXPTAU0):
    o = O.BNMFVBOracle(R, M, K, PRI)
    seed_state(o, state, exptau)
    return o


# ---------------------------------------------------------------- 1. launch shapes
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_launch_shapes_match_the_oracle(shape):
    M, K = SHAPES[shape]()
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0
    R, state = vb_problem(M, K)
    o = _oracle(R, M, K, state)
    o.sweep()
    o_elbo, o_mse, o_esd = o.elbo(), o.predict(M)["MSE"], o.exp_square_diff()
    under = shape in UNDERFLOW
    (g, g3), desc = vb_run(shape, (1, 2))
    assert "layout=observed" in desc and "long_form_units=%s" % LONG_UNITS.get(shape, "0/0") in desc, desc
    err = {}
    for n in NAMES:
        ref = getattr(o, n)
        err[n] = abs(g[n] / ref - 1).max() if n.startswith("tau") else _scaled(g[n], ref)
    err["exptau"] = abs(g["exptau"][0] / o.exptau - 1)
    err["MSE"] = abs(g["mse"][0] / o_mse - 1)
    err["esd"] = abs(g["terms"][0, 0] / o_esd - 1)
    print("%s: %s" % (shape, " ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    for n, e in err.items():
        assert e < 5e-4, (n, e)
    print("%s: ELBO device %.12g oracle %.12g" % (shape, g["elbo"][0], o_elbo))
    if under:
        assert not np.isfinite(o_elbo) and not np.isfinite(g["elbo"][0])
        o.sweep(); o.sweep()
        o3 = o.elbo()
        print("%s: ELBO of the third iteration: device %.12g oracle %.12g (rel %.2e)" % (shape, g3["elbo"][-1], o3, abs(g3["elbo"][-1] / o3 - 1)))
        assert np.isfinite(o3)
        np.testing.assert_allclose(g3["elbo"][-1], o3, rtol=2e-4)
    else:
        assert np.isfinite(o_elbo)
        np.testing.assert_allclose(g["elbo"][0], o_elbo, rtol=2e-5)
    # the record's metrics are those of the returned expectations (fp64 NumPy on the fp32 values): masked SSE / MSE rel 2e-5
    want = metrics_from_sums(O.metric_sums(M, R, g["expU"] @ g["expV"].T))
    assert abs(g["mse"][0] / want["MSE"] - 1) < 2e-5


# ---------------------------------------------------------------- 2. the reference's trajectories and known answers
def test_toy_trajectory_matches_reference(golden):
    g = golden("bnmf_vb.npz").case("toy")
    t = golden("toy_data.npz").case("bnmf")
    I, J = t["R"].shape; K = 10
    b = bnmf_vb_observed(t["R"], t["M"], K, dict(alpha=1., beta=1., lambdaU=0.1 * np.ones((I, K)), lambdaV=0.1 * np.ones((J, K))), verbose=False)
    b.initialise('exp')
    assert abs(b.exptau - float(g["init_exptau"])) < 2e-6 * b.exptau
    np.testing.assert_allclose(b.expU, g["init_expU"], rtol=1e-9)
    assert abs(b.exp_square_diff() - float(g["init_esd"])) < 2e-6 * float(g["init_esd"])
    b.run(20)
    np.testing.assert_allclose(b.all_performances['MSE'], g["mse"], rtol=1e-3)
    np.testing.assert_allclose(b.all_performances['MSE'][:5], g["mse"][:5], rtol=2e-5)
    np.testing.assert_allclose(b.all_exp_tau, g["exptau"], rtol=1e-3)
    np.testing.assert_allclose(b.all_elbo, g["elbo"], rtol=2e-4)
    np.testing.assert_allclose(b.all_elbo[:6], g["elbo"][:6], rtol=2e-5)
    for nm in ["expU", "expV", "muU", "muV", "tauU", "tauV"]:
        ref = g["it20/" + nm]
        assert np.abs(getattr(b, nm) - ref).max() < 2e-3 * np.abs(ref).max(), nm
    assert abs(b.elbo() - g["elbo"][-1]) < 2e-4 * abs(g["elbo"][-1])
    q = [b.quality(m) for m in ["loglikelihood", "BIC", "AIC", "MSE", "ELBO"]]
    np.testing.assert_allclose(q, g["quality"], rtol=1e-3)
    p = b.predict(t["M"])
    np.testing.assert_allclose([p["MSE"], p["R^2"], p["Rp"]], g["final_perf"], rtol=1e-3)
    assert len(b.all_times) == 20 and not hasattr(b, "all_performances_test")
    b.close()


def test_ragged_case_matches_reference(golden):
    g = golden("bnmf_vb.npz").case("r31x23")
    K = 4
    b = bnmf_vb_observed(g["R"], g["M"], K, dict(alpha=2., beta=.5, lambdaU=g["lambdaU"], lambdaV=g["lambdaV"]), verbose=False)
    b.initialise('exp', {"tauU": g["tauU0"], "tauV": g["tauV0"]})
    b.run(10)
    assert "layout=observed" in b.describe()
    np.testing.assert_allclose(b.all_performances['MSE'], g["mse"], rtol=1e-3)
    np.testing.assert_allclose(b.all_elbo, g["elbo"], rtol=1e-4)
    assert np.abs(b.expU - g["it10/expU"]).max() < 2e-3 * np.abs(g["it10/expU"]).max()
    b.close()


def test_known_answers_of_reference_tests():
    """tests/code/test_bnmf_vb_optimised.py:218-311 (tests/test_bnmf_vb_gpu.py::test_known_answers_of_reference_tests on this class)."""
    I, J, K = 5, 3, 2
    R = np.ones((I, J)); M = np.ones((I, J)); M[0, 0] = M[2, 2] = M[3, 1] = 0
    lambdaU = 2 * np.ones((I, K)); lambdaV = 3 * np.ones((J, K))
    pri = dict(alpha=3, beta=1, lambdaU=lambdaU, lambdaV=lambdaV)
    b = bnmf_vb_observed(R, M, K, pri, verbose=False)
    b.expU = 1. / lambdaU; b.expV = 1. / lambdaV; b.varU = 2 * np.ones((I, K)); b.varV = 3 * np.ones((J, K))
    assert abs(b.exp_square_diff() - 172.66666666666666) < 2e-5      # expV = 1/3 is rounded to fp32 on the device
    b.update_tau()
    assert b.alpha_s == 3 + 12. / 2. and abs(b.beta_s - (1 + 172.66666666666666 / 2.)) < 2e-5
    for k in range(K):
        b = bnmf_vb_observed(R, M, K, pri, verbose=False)
        b.muU = np.zeros((I, K)); b.tauU = np.zeros((I, K)); b.muV = np.zeros((J, K)); b.tauV = np.zeros((J, K))
        b.expU = 1. / lambdaU; b.expV = 1. / lambdaV; b.varU = 2 * np.ones((I, K)); b.varV = 3 * np.ones((J, K))
        b.exptau = 3.
        b.update_U(k)
        for i in range(I):
            w = (M[i] * (b.expV[:, k] ** 2 + b.varV[:, k])).sum()
            assert abs(b.tauU[i, k] - 3. * w) < 1e-5 * 3. * w
            ref = (1. / (3. * w)) * (-2. + 3. * (M[i] * ((R[i] - b.expU[i] @ b.expV.T + b.expU[i, k] * b.expV[:, k]) * b.expV[:, k])).sum())
            assert abs(b.muU[i, k] - ref) < 1e-5
        b.update_V(k)
        for j in range(J):
            w = (M[:, j] * (b.expU[:, k] ** 2 + b.varU[:, k])).sum()
            assert abs(b.tauV[j, k] - 3. * w) < 1e-5 * 3. * w
    b = bnmf_vb_observed(R, M, K, pri, verbose=False)
    b.initialise()
    assert abs(b.exptau - (3 + 12. / 2.) / (1 + 35.4113198623 / 2.)) < 1e-6
    assert abs(b.explogtau - (2.1406414779556 - math.log(1 + 35.4113198623 / 2.))) < 1e-6
    b.tauU = 4 * np.ones((I, K)); b.update_exp_U(0)
    assert np.abs(b.expU[:, 0] - (0.5 + 0.5 * 0.2876155949126352)).max() < 1e-5
    assert np.abs(b.varU[:, 0] - 0.25 * (1. - 0.37033832534958433)).max() < 1e-5
    with pytest.raises(AssertionError) as e:
        b.quality('FAIL')
    assert str(e.value) == "Unrecognised metric for model quality: FAIL."


# ---------------------------------------------------------------- 3. against the dense class
def test_five_iterations_follow_the_dense_class():
    I, J, K = 40, 37, 5
    rs = np.random.RandomState(41)
    M = (rs.rand(I, J) < 0.5).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    M_pred = ((M == 0) & (rs.rand(I, J) < 0.5)).astype(float)          # disjoint from the training mask
    assert M_pred.sum() > 100 and (M * M_pred).sum() == 0
    R, _, _ = _problem(M, K, 5)
    res = {}
    for cls in (bnmf_vb_observed, bnmf_vb_optimised):
        b = cls(R, M, K, PRI, verbose=False)
        b.initialise('exp')
        b.run(5)
        p = b.predict(M_pred)
        res[cls] = (np.array(b.all_performances["MSE"]), np.array(b.all_exp_tau), np.array(b.all_elbo),
                    np.array([p["MSE"], p["R^2"], p["Rp"]]), np.array([b.quality(m) for m in ["loglikelihood", "BIC", "AIC", "MSE", "ELBO"]]))
        b.close()
    got, want = res[bnmf_vb_observed], res[bnmf_vb_optimised]
    for name, g, w, tol in zip(("MSE", "exptau", "ELBO", "predict", "quality"), got, want, (1e-3, 1e-3, 2e-4, 1e-3, 1e-3)):
        print("%s: largest relative difference %.2e" % (name, np.abs(g / w - 1).max()))
        np.testing.assert_allclose(g, w, rtol=tol, err_msg=name)


# ---------------------------------------------------------------- 4. hooks
@pytest.mark.parametrize("shape,which", [("row_counts", 0), ("col_counts", 1)])        # (the long units in the hook's direction)
def test_a_column_update_changes_mu_and_tau_of_its_column_only(shape, which):
    M, K = SHAPES[shape]()
    for k in (0, K - 1):
        R, state, b = vb_model(M, K)
        o = _oracle(R, M, K, state)
        if which == 0:
            b.update_U(k); o.update_U(k)
        else:
            b.update_V(k); o.update_V(k)
        mu, tau = ("muU", "tauU") if which == 0 else ("muV", "tauV")
        for n in NAMES:
            held = state[n].astype(np.float32).astype(np.float64)               # what the device holds of the state
            if n in (mu, tau):
                rest = np.arange(K) != k
                assert np.array_equal(getattr(b, n)[:, rest], held[:, rest]), n
            else:
                assert np.array_equal(getattr(b, n), held), n
        e_tau = abs(getattr(b, tau)[:, k] / getattr(o, tau)[:, k] - 1).max(); e_mu = _scaled(getattr(b, mu)[:, k], getattr(o, mu)[:, k])
        print("%s k=%d: tau %.2e mu %.2e" % (shape, k, e_tau, e_mu))
        np.testing.assert_allclose(getattr(b, tau)[:, k], getattr(o, tau)[:, k], rtol=2e-6)
        assert e_mu < 5e-4
        b.close()


@pytest.mark.parametrize("shape", ["row_counts", "K33"])
def test_exp_square_diff_of_a_set_state(shape):
    M, K = SHAPES[shape]()
    R, state, b = vb_model(M, K)
    want = _oracle(R, M, K, state).exp_square_diff()
    got = b.exp_square_diff()
    print("%s: exp_square_diff %.12g oracle %.12g (rel %.2e)" % (shape, got, want, abs(got / want - 1)))
    assert abs(got - want) < 2e-6 * want
    b.update_tau(); b.update_exp_tau()
    assert b.beta_s == PRI["beta"] + 0.5 * got and np.isfinite(b.elbo())
    b.close()


# ---------------------------------------------------------------- 5. one result
def test_run_3_then_4_equals_run_7():
    (one,), _ = vb_run("row_counts", (7,))
    (_, two), _ = vb_run("row_counts", (3, 4))
    assert np.array_equal(two["exptau"], one["exptau"][3:]) and np.array_equal(two["terms"], one["terms"][3:])
    assert np.array_equal(two["expU"], one["expU"]) and np.array_equal(two["tauV"], one["tauV"])
    assert len(set(one["exptau"])) == 7


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
from _obs_vb_cases import vb_run
out = {}
for shape in ("row_counts", "col_counts"):         # long units in the U half sweep, then in the V half sweep (and its end-of-iteration sums)
    (g,), desc = vb_run(shape, (3,))
    assert ("force_long=1" in desc) == (%r == "1"), desc
    assert ("long_form_units=3/0" if shape == "row_counts" else "long_form_units=0/3") in desc, desc
    out.update({shape + "_" + k: v for k, v in g.items()})
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
    row-count and column-count shapes: three iterations each, all eight state arrays and the record."""
    a = _child_run(tmp_path, False, "a")
    b = _child_run(tmp_path, False, "b")
    c = _child_run(tmp_path, True, "long")
    assert len(a.files) == 2 * (len(NAMES) + 6)
    for key in a.files:
        assert np.array_equal(a[key], b[key], equal_nan=True), "two default runs differ in %s" % key
        assert np.array_equal(a[key], c[key], equal_nan=True), "the long form differs from the default in %s" % key
    assert len(set(a["row_counts_mse"])) == 3 and len(set(a["col_counts_mse"])) == 3


# ---------------------------------------------------------------- 6. neighbours untouched
def test_the_gibbs_layout_and_the_dense_class_are_untouched_in_the_same_process():
    M, K = SHAPES["row_counts"]()
    R, U0, V0 = _problem(M, K, 5)

    def gibbs():
        b = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, seed=13, layout='observed')
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
        b.run(3)
        out = (b.all_U.copy(), b.all_V.copy(), b.all_tau.copy(), np.array(b.all_performances["MSE"]))
        b.close()
        return out

    def dense():
        b = bnmf_vb_optimised(R, M, K, PRI, verbose=False)
        b.initialise('exp')
        b.run(3)
        out = (b.expU.copy(), b.varV.copy(), np.array(b.all_exp_tau), np.array(b.all_elbo_terms))
        assert "layout=observed" not in b.describe()
        b.close()
        return out

    before = gibbs() + dense()
    _, _, ob = vb_model(M, K)
    ob.run(2)
    during = gibbs() + dense()            # (the variational observed model is still alive)
    ob.run(1)
    ob.close()
    after = gibbs() + dense()
    for x, y, z in zip(before, during, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)
