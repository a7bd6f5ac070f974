"""The non-probabilistic models on the device (csrc/kernel_np.hip): the reference's trajectories (tests/golden/np.npz), its single
updates, whole iterations at large shapes against a fp64 NumPy restatement written here, long rows and columns, a wide rank,
the same bits on two runs, and MatrixCrossValidation(method=NMF) against the reference's fold table.  The restatement
(tests/_np_restatement.py) is pinned to the reference's numbers by tests/test_np_restatement_cpu.py."""
import os
import random

import numpy as np
import pytest

from bnmtf_amd.nmf_np import NMF
from bnmtf_amd.nmtf_np import NMTF
from _np_restatement import ref_nmf_iteration, ref_nmtf_iteration

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "np.npz"))
TOY = np.load(os.path.join(HERE, "golden", "toy_data.npz"))
GDSC = np.load(os.path.join(HERE, "golden", "gdsc.npz"))


def close_to_scale(a, b, tol=1e-3):
    assert a.shape == b.shape
    err = np.abs(a - b).max() / np.abs(b).max()
    assert err <= tol, err


def check_trajectory(model, tag, idiv):
    for key, m in [("mse", "MSE"), ("r2", "R^2")]:
        np.testing.assert_allclose(model.all_performances[m], G[tag + "/" + key], rtol=1e-4)
    np.testing.assert_allclose(model.all_performances["Rp"], G[tag + "/rp"], rtol=1e-4)
    np.testing.assert_allclose(idiv, G[tag + "/idiv"], rtol=1e-4, equal_nan=True)
    assert len(model.all_times) == len(G[tag + "/mse"]) and np.all(np.diff(model.all_times) >= 0)


def run_capturing_idiv(model, iterations, capsys):
    model.verbose = True
    model.run(iterations)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Iteration ")]
    assert len(lines) == iterations
    return np.array([float(l.split("I-divergence: ")[1].split(". MSE")[0]) for l in lines])


# ---------------------------------------------------------------- the reference's trajectories
@pytest.mark.parametrize("tag,R,M,K,iters", [
    ("nmf_rand", TOY["bnmf/R"], TOY["bnmf/M"], 10, 100),
    ("nmf_exp", TOY["bnmf/R"], TOY["bnmf/M"], 10, 100),
    ("nmf_gdsc", GDSC["ex/X_min"], GDSC["ex/M"], 10, 50),
    ("nmf_ragged", G["nmf_ragged/R"], G["nmf_ragged/M"], 3, 30),
])
def test_nmf_trajectory(tag, R, M, K, iters, capsys):
    n = NMF(R, M, K, verbose=False)
    n.U, n.V = G[tag + "/U0"].copy(), G[tag + "/V0"].copy()
    if tag + "/idiv0" in G:
        np.testing.assert_allclose(n.compute_I_div(), G[tag + "/idiv0"], rtol=1e-5)
    idiv = run_capturing_idiv(n, iters, capsys)
    check_trajectory(n, tag, idiv)
    close_to_scale(n.U, G[tag + "/U"]); close_to_scale(n.V, G[tag + "/V"])
    if tag + "/Mpred" in G:
        p = n.predict(G[tag + "/Mpred"])
        np.testing.assert_allclose([p["MSE"], p["R^2"], p["Rp"]], G[tag + "/pred"], rtol=1e-4)
    n.close()


def test_nmf_train_matches_the_seeded_reference():
    np.random.seed(int(G["nmf_rand/seed"]))
    n = NMF(TOY["bnmf/R"], TOY["bnmf/M"], 10, verbose=False)
    n.train(100, init_UV='random')
    np.testing.assert_allclose(n.all_performances["MSE"], G["nmf_rand/mse"], rtol=1e-4)
    close_to_scale(n.U, G["nmf_rand/U"])


@pytest.mark.parametrize("tag,init_S,init_FG", [("nmtf_expkm", "exponential", "kmeans"), ("nmtf_rand", "random", "random")])
def test_nmtf_trajectory(tag, init_S, init_FG, capsys):
    seed = int(G[tag + "/seed"])
    np.random.seed(seed); random.seed(seed)
    t = NMTF(TOY["bnmtf/R"], TOY["bnmtf/M"], 5, 5, verbose=False)
    t.initialise(init_S, init_FG)
    for n in "SFG":
        np.testing.assert_allclose(getattr(t, n), G[tag + "/%s0" % n], rtol=1e-12)
    np.testing.assert_allclose(t.compute_I_div(), G[tag + "/idiv0"], rtol=1e-5, equal_nan=True)
    idiv = run_capturing_idiv(t, 50, capsys)
    check_trajectory(t, tag, idiv)
    for n in "SFG":
        close_to_scale(getattr(t, n), G[tag + "/" + n])
    t.close()


# ---------------------------------------------------------------- the update hooks
def test_nmf_update_hooks():
    n = NMF(TOY["bnmf/R"], TOY["bnmf/M"], 10, verbose=False)
    n.U, n.V = G["nmf_rand/U0"].copy(), G["nmf_rand/V0"].copy()
    n.update_U(3)
    np.testing.assert_allclose(n.U, G["nmf_upd/U_after_U3"], rtol=1e-5)
    np.testing.assert_allclose(n.V, G["nmf_rand/V0"], rtol=1e-7)
    n.U, n.V = G["nmf_rand/U0"].copy(), G["nmf_rand/V0"].copy()
    n.update_V(5)
    np.testing.assert_allclose(n.V, G["nmf_upd/V_after_V5"], rtol=1e-5)


@pytest.mark.parametrize("name", ["S21", "F3", "G4"])
def test_nmtf_update_hooks(name):
    t = NMTF(TOY["bnmtf/R"], TOY["bnmtf/M"], 5, 5, verbose=False)
    t.S, t.F, t.G = G["nmtf_rand/S0"].copy(), G["nmtf_rand/F0"].copy(), G["nmtf_rand/G0"].copy()
    {"S21": lambda: t.update_S(2, 1), "F3": lambda: t.update_F(3), "G4": lambda: t.update_G(4)}[name]()
    for n in "SFG":
        np.testing.assert_allclose(getattr(t, n), G["nmtf_upd/%s/%s" % (name, n)], rtol=1e-5)


# ---------------------------------------------------------------- large shapes against a fp64 restatement
def problem(I, J, K, seed, frac=0.5):
    rs = np.random.RandomState(seed)
    U0, V0 = rs.rand(I, K), rs.rand(J, K)
    R = U0 @ V0.T * (0.8 + 0.4 * rs.rand(I, J))
    M = (rs.rand(I, J) < frac).astype(float)
    M[:, 0] = 1; M[0, :] = 1
    return R, M, rs.rand(I, K) + 0.1, rs.rand(J, K) + 0.1


def masked_mse(R, M, P):
    return float((M * (R - P) ** 2).sum() / M.sum())


@pytest.mark.parametrize("I,J,K", [(4096, 4096, 32), (256, 8192, 64), (8192, 256, 64), (300, 190, 200)])
def test_nmf_iteration_against_restatement(I, J, K):
    R, M, U0, V0 = problem(I, J, K, seed=I + J + K)
    n = NMF(R, M, K, verbose=False)
    n.U, n.V = U0.copy(), V0.copy()
    n.run(1)
    U, V = ref_nmf_iteration(R, M.astype(bool), U0, V0)
    close_to_scale(n.U, U); close_to_scale(n.V, V)
    np.testing.assert_allclose(n.all_performances["MSE"][0], masked_mse(R, M, U @ V.T), rtol=1e-4)
    n.close()


def test_nmtf_iteration_against_restatement():
    I = J = 1024; K = L = 16
    rs = np.random.RandomState(5)
    R = rs.rand(I, K) @ rs.rand(K, L) @ rs.rand(J, L).T * (0.8 + 0.4 * rs.rand(I, J))
    M = (rs.rand(I, J) < 0.6).astype(float); M[:, 0] = 1; M[0, :] = 1
    F0, S0, G0 = rs.rand(I, K) + 0.1, rs.rand(K, L) + 0.1, rs.rand(J, L) + 0.1
    t = NMTF(R, M, K, L, verbose=False)
    t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
    t.run(1)
    F, S, G = ref_nmtf_iteration(R, M, F0, S0, G0)
    close_to_scale(t.S, S); close_to_scale(t.F, F); close_to_scale(t.G, G)
    np.testing.assert_allclose(t.all_performances["MSE"][0], masked_mse(R, M, F @ S @ G.T), rtol=1e-4)
    t.close()


# ---------------------------------------------------------------- determinism
def test_same_bits_on_two_runs():
    R, M, U0, V0 = problem(700, 900, 24, seed=3)
    out = []
    for _ in range(2):
        n = NMF(R, M, 24, verbose=False)
        n.U, n.V = U0.copy(), V0.copy()
        n.run(5)
        out.append((n.U, n.V, np.array(n.all_performances["MSE"]), n.compute_I_div()))
        n.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2]) and out[0][3] == out[1][3]
    t_out = []
    R, M = TOY["bnmtf/R"], TOY["bnmtf/M"]
    for _ in range(2):
        t = NMTF(R, M, 5, 5, verbose=False)
        t.F, t.S, t.G = G["nmtf_rand/F0"].copy(), G["nmtf_rand/S0"].copy(), G["nmtf_rand/G0"].copy()
        t.run(3)
        t_out.append((t.F, t.S, t.G))
        t.close()
    for a, b in zip(*t_out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- cross-validation
def test_matrix_cross_validation_fold_table(tmp_path):
    from bnmtf_amd.cross_validation import MatrixCrossValidation
    random.seed(int(G["cv/seed"])); np.random.seed(int(G["cv/seed"]))
    cv = MatrixCrossValidation(method=NMF, X=GDSC["ex/X_min"], M=GDSC["ex/M"], K=5, parameter_search=[{"K": 2}, {"K": 4}],
                               train_config={"iterations": 50, "init_UV": "ones"}, file_performance=str(tmp_path / "cv.txt"))
    cv.run()
    for K in (2, 4):
        perf = cv.all_performances[cv.JSON({"K": K})]
        np.testing.assert_allclose(np.array([perf["MSE"], perf["R^2"], perf["Rp"]]), G["cv/K%d" % K], rtol=1e-4)
