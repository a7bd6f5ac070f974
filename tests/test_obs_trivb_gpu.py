"""bnmtf_vb_observed (csrc/kernel_obs_trivb.hip, obs_trivb_sweep_kernel) on the
device: the variational tri-factorisation with the residual kept on the observed entries, against the fp64 oracle on every launch
shape, the reference's golden vectors and known answers, the dense class, the exact diagonal of the S system, and itself (one
result whatever the form or the split).

Tolerances are the project's own.  The launch shapes: 5e-4 (tests/test_obs_vb_gpu.py::test_launch_shapes_match_the_oracle), factors
scaled by max(1, max|ref|), tau relative; the ELBO rel 2e-5 where the oracle's is finite; the record's MSE against fp64 NumPy on
the returned expectations rel 2e-5.  The golden vectors: those of tests/test_bnmtf_vb_gpu.py.  The dense class: those of
tests/test_obs_vb_gpu.py::test_five_iterations_follow_the_dense_class.  exp_square_diff of a set state: rel 2e-6."""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from bnmtf_amd import bnmtf_gibbs_optimised, bnmtf_vb_observed, bnmtf_vb_optimised
from bnmtf_amd._base import metrics_from_sums
from oracle import bnmtf_oracle as O

import _obs_trivb_cases as TC
from _obs_cases import SHAPES
from _obs_tri_cases import COL_COUNTS, Case, _mask
from _obs_vb_cases import vb_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(TC.NAMES)


def _scaled(got, ref):
    return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())


def _oracle(R, M, K, L, state, exptau=TC.EXPTAU0, pri=TC.PRI):
    o = O.BNMTFVBOracle(R, M, K, L, pri)
    TC.seed_state(o, state, exptau)
    return o


# ---------------------------------------------------------------- 1. launch shapes
@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_launch_shapes_match_the_oracle(name, permuted):
    M, K, L = TC.CASES[name]()
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0
    R, state = TC.problem(M, K, L)
    od = TC.orders(K, L, 3, permuted)
    (g1, g3), desc = TC.run(name, (1, 2), permuted)
    assert "layout=observed" in desc and "long_form_units=%s" % TC.LONG_UNITS.get(name, "0/0") in desc, desc
    o = _oracle(R, M, K, L, state)
    for its, g in ((1, g1), (3, g3)):
        for it in range(0 if its == 1 else 1, its):
            o.sweep(*TC.oracle_orders(od[it], K, L))
        o_mse, o_esd = o.predict(M)["MSE"], o.exp_square_diff()
        with np.errstate(all="ignore"):
            o_elbo = o.elbo()
        err = {}
        for n in NAMES:
            ref = getattr(o, n)
            err[n] = abs(g[n] / ref - 1).max() if n.startswith("tau") else _scaled(g[n], ref)
        err["exptau"] = abs(g["exptau"][-1] / o.exptau - 1)
        err["MSE"] = abs(g["mse"][-1] / o_mse - 1)
        err["esd"] = abs(g["terms"][-1, 0] / o_esd - 1)
        print("%s %s it %d: %s" % (name, "permuted" if permuted else "identity", its, " ".join("%s %.2e" % kv for kv in sorted(err.items()))))
        for n, e in err.items():
            assert e < 5e-4, (its, n, e)
        print("%s it %d: ELBO device %.12g oracle %.12g" % (name, its, float(g["elbo"]), o_elbo))
        if np.isfinite(o_elbo):
            np.testing.assert_allclose(float(g["elbo"]), o_elbo, rtol=2e-5)
        # the record's metrics are those of the returned expectations (fp64 NumPy on the fp32 values)
        want = metrics_from_sums(O.metric_sums(M, R, g["expF"] @ g["expS"] @ g["expG"].T))
        assert abs(g["mse"][-1] / want["MSE"] - 1) < 2e-5


# ---------------------------------------------------------------- 2. the reference's golden vectors and known answers
def _t5x3():
    I, J, K, L = 5, 3, 2, 4
    R = np.ones((I, J)); M = np.ones((I, J)); M[0, 0] = M[2, 2] = M[3, 1] = 0
    pri = dict(alpha=3, beta=1, lambdaF=2 * np.ones((I, K)), lambdaS=3 * np.ones((K, L)), lambdaG=4 * np.ones((J, L)))
    return R, M, K, L, pri


def _case(golden, tag):
    g = golden("bnmtf_vb.npz").case(tag)
    if tag == "t5x3":
        R, M, K, L, pri = _t5x3()
    else:
        R, M = g["R"], g["M"]
        K, L = g["lambdaS"].shape
        pri = dict(alpha=2.0, beta=0.5, lambdaF=g["lambdaF"], lambdaS=g["lambdaS"], lambdaG=g["lambdaG"])
    return g, R, M, K, L, pri


def test_known_answers_of_the_reference_tests():
    """test_bnmtf_vb_optimised.py:281-300 (tests/test_bnmtf_vb_gpu.py::test_known_answers_of_the_reference_tests on this class)."""
    R, M, K, L, pri = _t5x3()
    I, J = R.shape
    b = bnmtf_vb_observed(R, M, K, L, pri, verbose=False)
    b.expF = 1. / pri["lambdaF"]; b.expS = 1. / pri["lambdaS"]; b.expG = 1. / pri["lambdaG"]
    b.varF = np.ones((I, K)) * 2; b.varS = np.ones((K, L)) * 3; b.varG = np.ones((J, L)) * 4
    assert abs(b.exp_square_diff() - (2749 + 5. / 6.)) < 2e-6 * 2749           # 1/3 is rounded to fp32 on the device
    b.update_tau()
    assert b.alpha_s == 3 + 12. / 2. and abs(b.beta_s - (1 + (2749 + 5. / 6.) / 2.)) < 2e-6 * 1375
    with pytest.raises(AssertionError) as e:
        b.quality('FAIL')
    assert str(e.value) == "Unrecognised metric for model quality: FAIL."
    b.close()


@pytest.mark.parametrize("tag", ["t5x3", "r33x27"])
def test_single_updates_match_the_reference(golden, tag):
    """update_F(k), update_S(k,l), update_G(l) (bnmtf_vb_optimised.py:241-273), each from the same hand-set state."""
    g, R, M, K, L, pri = _case(golden, tag)
    b = bnmtf_vb_observed(R, M, K, L, pri, verbose=False)

    def fresh():
        for n in NAMES:
            setattr(b, n, g["state/" + n].copy())
        b.exptau = float(g["state/exptau"])
        return b

    assert abs(fresh().exp_square_diff() - float(g["esd"])) < 5e-6 * float(g["esd"])
    for k in range(K):
        fresh().update_F(k)
        np.testing.assert_allclose(b.tauF[:, k], g["upd/tauF"][:, k], rtol=5e-6)
        scale = np.abs(g["upd/muF"][:, k]).max() + 1.0
        assert np.abs(b.muF[:, k] - g["upd/muF"][:, k]).max() < 2e-5 * scale
    for l in range(L):
        fresh().update_G(l)
        np.testing.assert_allclose(b.tauG[:, l], g["upd/tauG"][:, l], rtol=5e-6)
        scale = np.abs(g["upd/muG"][:, l]).max() + 1.0
        assert np.abs(b.muG[:, l] - g["upd/muG"][:, l]).max() < 2e-5 * scale
    for k, l in itertools.product(range(K), range(L)):
        fresh().update_S(k, l)
        assert abs(b.tauS[k, l] - g["upd/tauS"][k, l]) < 5e-6 * g["upd/tauS"][k, l]
        assert abs(b.muS[k, l] - g["upd/muS"][k, l]) < 2e-5 * (np.abs(g["upd/muS"]).max() + 1.0)
        others = np.ones((K, L), dtype=bool); others[k, l] = False
        assert np.array_equal(b.muS[others], g["state/muS"][others].astype(np.float32).astype(np.float64))
    b.close()


def test_ragged_run_matches_the_reference(golden):
    """Ten iterations with the reference's shuffles: once handed over, once re-drawn from Python's random stream."""
    g, R, M, K, L, pri = _case(golden, "r33x27")
    orders = np.concatenate([g["order_S"], g["order_F"], g["order_G"]], axis=1)
    for mode in ("stored", "stream"):
        b = bnmtf_vb_observed(R, M, K, L, pri, verbose=False)
        b.initialise("exp", "exp", {"tauF": g["init/tauF"], "tauS": g["init/tauS"], "tauG": g["init/tauG"]})
        assert abs(b.exptau - float(g["init_exptau"])) < 5e-6 * b.exptau
        if mode == "stored":
            b.run(10, orders=orders)
        else:
            random.seed(int(g["seed"]))
            b.run(10)
        np.testing.assert_allclose(b.all_performances["MSE"], g["mse"], rtol=1e-3)
        np.testing.assert_allclose(b.all_performances["MSE"][:3], g["mse"][:3], rtol=5e-5)
        np.testing.assert_allclose(b.all_exp_tau, g["exptau"], rtol=1e-3)
        assert abs(b.elbo() - g["elbo"][-1]) < 2e-4 * abs(g["elbo"][-1])
        for n in ("expF", "expS", "expG", "muF", "tauG"):
            ref = g["final/" + n]
            assert np.abs(getattr(b, n) - ref).max() < 3e-3 * np.abs(ref).max(), n
        np.testing.assert_allclose([b.quality(m) for m in ["loglikelihood", "BIC", "AIC", "MSE", "ELBO"]], g["quality"], rtol=1e-3)
        assert len(b.all_times) == 10 and "layout=observed" in b.describe()
        b.close()


def test_toy_run_matches_the_reference(golden):
    """data_toy/bnmtf, K = L = 5, init random / random under numpy.random.seed(5), 20 iterations under random.seed(3)."""
    t = golden("toy_data.npz").case("bnmtf")
    g = golden("bnmtf_vb.npz").case("toy")
    I, J = t["R"].shape; K = L = 5
    pri = dict(alpha=1.0, beta=1.0, lambdaF=0.1 * np.ones((I, K)), lambdaS=0.1 * np.ones((K, L)), lambdaG=0.1 * np.ones((J, L)))
    b = bnmtf_vb_observed(t["R"], t["M"], K, L, pri, verbose=False)
    np.random.seed(5)
    b.initialise("random", "random")
    for n in ("muF", "muS", "muG"):                      # same NumPy stream as the reference's scalar draws
        np.testing.assert_allclose(getattr(b, n), g["init/" + n], rtol=1e-12)
    assert abs(b.exptau - float(g["init_exptau"])) < 5e-6 * b.exptau
    assert abs(b.exp_square_diff() - float(g["init_esd"])) < 5e-6 * float(g["init_esd"])
    assert abs(b.elbo() - float(g["init_elbo"])) < 2e-5 * abs(float(g["init_elbo"]))
    random.seed(int(g["seed"]))
    b.run(20)
    np.testing.assert_allclose(b.all_performances["MSE"], g["mse"], rtol=2e-3)
    np.testing.assert_allclose(b.all_performances["MSE"][:5], g["mse"][:5], rtol=1e-4)
    np.testing.assert_allclose(b.all_exp_tau, g["exptau"], rtol=2e-3)
    assert abs(b.elbo() - g["elbo"][-1]) < 5e-4 * abs(g["elbo"][-1])
    p = b.predict(t["M"])
    np.testing.assert_allclose([p["MSE"], p["R^2"], p["Rp"]], g["final_perf"], rtol=2e-3)
    b.close()


# ---------------------------------------------------------------- 3. against the dense class
def test_ten_iterations_follow_the_dense_class():
    I, J, K, L = 120, 90, 5, 4
    rs = np.random.RandomState(41)
    M = (rs.rand(I, J) < 0.08).astype(float)           # (with an entry added per empty row and column: 90 % missing)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    M_pred = ((M == 0) & (rs.rand(I, J) < 0.1)).astype(float)          # disjoint from the training mask
    assert 0.89 < 1 - M.mean() < 0.91 and M_pred.sum() > 100 and (M * M_pred).sum() == 0
    R, state = TC.problem(M, K, L, seed=7)
    od = TC.orders(K, L, 10, True)
    res = {}
    for cls in (bnmtf_vb_observed, bnmtf_vb_optimised):
        b = cls(R, M, K, L, TC.PRI, verbose=False)
        np.random.seed(3)
        b.initialise('random', 'random')
        b.run(10, orders=od)
        p = b.predict(M_pred)
        res[cls] = (np.array(b.all_performances["MSE"]), np.array(b.all_exp_tau), np.array([b.elbo()]),
                    np.array([p["MSE"], p["R^2"], p["Rp"]]), np.array([b.quality(m) for m in ["loglikelihood", "BIC", "AIC", "MSE", "ELBO"]]))
        b.close()
    got, want = res[bnmtf_vb_observed], res[bnmtf_vb_optimised]
    for name, g, w, tol in zip(("MSE", "exptau", "ELBO", "predict", "quality"), got, want, (1e-3, 1e-3, 2e-4, 1e-3, 1e-3)):
        print("%s: largest relative difference %.2e" % (name, np.abs(g / w - 1).max()))
    for name, g, w, tol in zip(("MSE", "exptau", "ELBO", "predict", "quality"), got, want, (1e-3, 1e-3, 2e-4, 1e-3, 1e-3)):
        np.testing.assert_allclose(g, w, rtol=tol, err_msg=name)


# ---------------------------------------------------------------- 4. hooks
@pytest.mark.parametrize("name", ["rows", "cols", "KL5x13"])        # (long units in either direction; a K L beside the 64-lane step)
def test_a_hook_changes_mu_and_tau_of_its_target_only(name):
    R, M, K, L, state, b = TC.model(name)
    held = {n: state[n].astype(np.float32).astype(np.float64) for n in NAMES}               # what the device holds of the state

    def check(mu, tau, target, o):
        for n in NAMES:
            got = getattr(b, n)
            if n in (mu, tau):
                rest = np.ones(got.shape, dtype=bool); rest[target] = False
                assert np.array_equal(got[rest], held[n][rest]), n
            else:
                assert np.array_equal(got, held[n]), n
        e_tau = abs(getattr(b, tau)[target] / getattr(o, tau)[target] - 1).max(); e_mu = _scaled(getattr(b, mu)[target], getattr(o, mu)[target])
        print("%s %s%s: tau %.2e mu %.2e" % (name, mu, target, e_tau, e_mu))
        assert e_tau < 5e-6 and e_mu < 5e-4

    for k in (0, K - 1):
        TC.seed_state(b, state); o = _oracle(R, M, K, L, state)
        b.update_F(k); o.update_F(k)
        check("muF", "tauF", (slice(None), k), o)
    for l in (0, L - 1):
        TC.seed_state(b, state); o = _oracle(R, M, K, L, state)
        b.update_G(l); o.update_G(l)
        check("muG", "tauG", (slice(None), l), o)
    for k, l in ((0, 0), (K - 1, L - 1)):
        TC.seed_state(b, state); o = _oracle(R, M, K, L, state)
        b.update_S(k, l); o.update_S(k, l)
        check("muS", "tauS", (slice(k, k + 1), slice(l, l + 1)), o)
    b.close()


@pytest.mark.parametrize("name", ["rows", "cols", "KL31x32"])
def test_exp_square_diff_of_a_set_state(name):
    R, M, K, L, state, b = TC.model(name)
    want = _oracle(R, M, K, L, state).exp_square_diff()
    got = b.exp_square_diff()
    print("%s: exp_square_diff %.12g oracle %.12g (rel %.2e)" % (name, got, want, abs(got / want - 1)))
    assert abs(got - want) < 2e-6 * want
    b.update_tau(); b.update_exp_tau()
    assert b.beta_s == TC.PRI["beta"] + 0.5 * got and np.isfinite(b.elbo())
    b.close()


# ---------------------------------------------------------------- 5. the S system's new diagonal, exactly
@pytest.mark.parametrize("case", [Case("counts_small", 520, 17, 2, 3, COL_COUNTS), Case("counts", 520, 130, 32, 32, COL_COUNTS)], ids=lambda c: c.id)
def test_the_second_moment_diagonal_of_the_S_system_is_exact(case):
    """tauS of update_S(k, l) = exptau sum_j W~_j,kk Gamma~_j,ll with W~_j,kk = sum_{i in Omega_j} (F_ik^2 + varF_ik) (obs_tri_gram_vb_kernel's
    diagonal) and Gamma~_j,ll = G_jl^2 + varG_jl.  On integer grids (F 0/1, varF, varG in {0, 1, 2}, G in {0, 1, 2}, exptau = 1) every
    W~_j,kk is below 2^16 and every Gamma~_j,ll at most 6, so the packed bf16x3 GEMM drops nothing, and wherever the sum of |terms|
    is below 2^24 the only correct fp32 value is the exact one."""
    I, J, K, L = case.I, case.J, case.K, case.L
    M = _mask(case)
    cols = (M != 0).sum(axis=0).astype(int)
    assert set(COL_COUNTS) <= set(cols.tolist()) and I in cols
    rs = np.random.RandomState(I + 31 * J + K)
    F = (rs.rand(I, K) < 0.4).astype(float); G = rs.randint(0, 3, (J, L)).astype(float)
    G[G.sum(axis=1) == 0, 0] = 1
    vF = rs.randint(0, 3, (I, K)).astype(float); vG = rs.randint(0, 3, (J, L)).astype(float)
    S = rs.randint(1, 4, (K, L)).astype(float); vS = rs.randint(0, 3, (K, L)).astype(float)
    R = rs.randint(0, 8, (I, J)).astype(float)
    state = dict(muF=F.copy(), tauF=np.ones((I, K)), expF=F, varF=vF, muS=S.copy(), tauS=np.ones((K, L)), expS=S, varS=vS,
                 muG=G.copy(), tauG=np.ones((J, L)), expG=G, varG=vG)
    Wd = M.T @ (F ** 2 + vF)                      # [J][K]
    Gd = G ** 2 + vG                              # [J][L]
    want = Wd.T @ Gd                              # [K][L]: every term a non-negative integer
    assert Wd.max() < 2 ** 16 and Gd.max() <= 6
    exact = want < 2 ** 24
    assert exact.any()
    pri = dict(alpha=1., beta=1., lambdaF=0.5, lambdaS=0.5, lambdaG=0.5)
    b = bnmtf_vb_observed(R, M, K, L, pri, verbose=False)
    o = _oracle(R, M, K, L, state, exptau=1.0, pri=pri)
    picks = [(0, 0), (K - 1, L - 1), (K // 2, L // 2), (K - 1, 0)]
    n_exact = 0
    for k, l in picks:
        TC.seed_state(b, state, 1.0)
        b.update_S(k, l); o.update_S(k, l)
        assert abs(o.tauS[k, l] - want[k, l]) < 1e-9 * want[k, l]
        if exact[k, l]:
            assert b.tauS[k, l] == want[k, l], (k, l, b.tauS[k, l], want[k, l])
            n_exact += 1
        else:
            assert abs(b.tauS[k, l] / want[k, l] - 1) < 5e-6
        scale = max(1.0, abs(o.muS[k, l]))
        print("%s (%d,%d): tauS %.0f exact=%s muS device %.9g oracle %.9g" % (case.id, k, l, want[k, l], bool(exact[k, l]), b.muS[k, l], o.muS[k, l]))
        assert abs(b.muS[k, l] - o.muS[k, l]) < 2e-5 * scale
    assert n_exact > 0
    b.close()


# ---------------------------------------------------------------- 6. one result
def test_two_runs_and_a_split_run_give_the_same_bits():
    for name in ("rows", "KL8x8"):
        (one,), _ = TC.run(name, (7,), True)
        (again,), _ = TC.run(name, (7,), True)
        (_, two), _ = TC.run(name, (3, 4), True)
        for n in NAMES:
            assert np.array_equal(one[n], again[n]), (name, n)
            assert np.array_equal(one[n], two[n]), (name, n)
        assert np.array_equal(one["exptau"], again["exptau"]) and np.array_equal(one["terms"], again["terms"])
        assert np.array_equal(two["exptau"], one["exptau"][3:]) and np.array_equal(two["terms"], one["terms"][3:])
        assert np.array_equal(two["mse"], one["mse"][3:])
        assert len(set(one["exptau"])) == 7


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [%r, %r]
import _obs_trivb_cases as TC
out = {}
for name in ("rows", "cols"):         # long units in the F half sweep, then in the G half sweep (and its end-of-iteration sums)
    (g,), desc = TC.run(name, (3,), True)
    assert ("force_long=1" in desc) == (%r == "1"), desc
    assert "long_form_units=" + TC.LONG_UNITS[name] in desc, desc
    out.update({name + "_" + k: v for k, v in g.items()})
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
    """BNMTF_OBS_LONG=1 (every unit down the long form) in a fresh child process against a default one, on the row-count and
    column-count shapes: three iterations each with permuted orders, all twelve state arrays and the record."""
    a = _child_run(tmp_path, False, "reg")
    c = _child_run(tmp_path, True, "long")
    assert len(a.files) == 2 * (len(NAMES) + 6)
    for key in a.files:
        assert np.array_equal(a[key], c[key], equal_nan=True), "the long form differs from the default in %s" % key
    assert len(set(a["rows_mse"])) == 3 and len(set(a["cols_mse"])) == 3


# ---------------------------------------------------------------- 7. neighbours untouched
def test_the_neighbours_are_untouched_in_the_same_process():
    M, K = SHAPES["row_counts"]()
    Rt, Mt, Kt, Lt, st, _b = TC.model("KL2x3")
    _b.close()

    def vb_obs():
        _, _, b = vb_model(M, K)
        b.run(2)
        out = (b.expU.copy(), b.tauV.copy(), np.array(b.all_exp_tau), np.array(b.all_elbo_terms))
        b.close()
        return out

    def gibbs_obs():
        b = bnmtf_gibbs_optimised(Rt, Mt, Kt, Lt, TC.PRI, verbose=False, seed=13, layout='observed')
        b.F, b.S, b.G, b.tau = st["expF"].copy(), st["expS"].copy(), st["expG"].copy(), 1.3
        b.run(3)
        out = (b.all_F.copy(), b.all_S.copy(), b.all_G.copy(), b.all_tau.copy())
        b.close()
        return out

    def dense():
        b = bnmtf_vb_optimised(Rt, Mt, Kt, Lt, TC.PRI, verbose=False)
        TC.seed_state(b, st)
        b.run(3, orders=TC.orders(Kt, Lt, 3, True))
        out = (b.expF.copy(), b.varG.copy(), b.tauS.copy(), np.array(b.all_exp_tau), np.array(b.all_elbo_terms))
        assert "layout=observed" not in b.describe()
        b.close()
        return out

    before = vb_obs() + gibbs_obs() + dense()
    _, _, _, _, _, ob = TC.model("KL2x3")
    ob.run(2, orders=TC.orders(Kt, Lt, 2, True))
    during = vb_obs() + gibbs_obs() + dense()            # (the new model is still alive)
    ob.run(1, orders=TC.orders(Kt, Lt, 1, False))
    ob.close()
    after = vb_obs() + gibbs_obs() + dense()
    for x, y, z in zip(before, during, after):
        assert np.array_equal(x, y) and np.array_equal(x, z)
