"""The non-probabilistic models' kernels (csrc/kernel_np.hip) at every launch shape they select, against the fp64 restatement
(tests/_np_restatement.py, pinned to the reference by tests/test_np_restatement_cpu.py).

np_sweep_kernel<E, RB> is picked by the inner extent m: E = 2, 4, 8, 16 for m up to 2048, 4096, 8192, 16384.  CASES puts every
instance at its index guards -- a partial last block (n % RB != 0) and idle lanes (T E > m) -- in the row and the column half
sweep (tests/test_np_restatement_cpu.py checks the table below and that dropping an edge entry moves the result by far more
than the tolerances here).  Also: the 16 384 limit, NMTF with K != L and I > 1024 (the S step's grid-stride path), the update
hooks at wide rank, five-iteration drift with predict() and compute_I_div() (np_metrics_kernel), and the same bits on two runs.

The tolerances are about ten times the largest fp32-against-fp64 error measured on an MI355X (entrywise relative errors of
the factors, relative errors of MSE, R^2, Rp and the I-divergence)."""
import numpy as np
import pytest

import _np_restatement as NR
from bnmtf_amd.nmf_np import NMF
from bnmtf_amd.nmtf_np import NMTF

pytestmark = pytest.mark.gpu

# (I, J, K): launch shape of the rows' / the columns' half sweep as E, T, RB, n % RB, idle lanes T E - m
CASES = [
    (37, 2048, 16),        # 2, 1024, 16, 5, 0       | 2, 64, 16, 0, 91
    (45, 2049, 33),        # 4, 576, 8, 5, 255       | 2, 64, 16, 1, 83
    (29, 4097, 64),        # 8, 576, 4, 1, 511       | 2, 64, 16, 1, 99
    (3, 8193, 65),         # 16, 576, 1, 0, 1023     | 2, 64, 16, 1, 125
    (21, 16384, 256),      # 16, 1024, 1, 0, 0       | 2, 64, 16, 0, 107 (1 024 blocks)
    (16383, 19, 1),        # 2, 64, 16, 15, 109      | 16, 1024, 1, 0, 1
    (2050, 4099, 24),      # 8, 576, 4, 2, 509       | 4, 576, 8, 3, 254
]
NMTF_CASES = [
    (2500, 700, 7, 3),     # S step: 1 024 blocks of 2-3 rows each
    (1100, 2049, 3, 11),   # G sweep over 1 100, F sweep E = 4
    (150, 120, 200, 5),    # wide K in the products
]

# measured on an MI355X: at most 1.1e-6 after one iteration or one update (V at (21, 16384, 256)), 1.8e-6 after five
TOL_ONE = 1e-5             # one iteration / one update: factors and metrics
TOL_DRIFT = 2e-5           # five iterations


def nmf_case(I, J, K):
    return NR.edge_problem(I, J, K, seed=I + 7 * J + K, sparse=True)


def nmtf_case(I, J, K, L):
    return NR.edge_problem(I, J, K, seed=I + 7 * J + K + 13 * L, sparse=True, L=L)


def run_capturing_idiv(model, iterations, capsys):
    model.verbose = True
    model.run(iterations)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Iteration ")]
    assert len(lines) == iterations
    return np.array([float(l.split("I-divergence: ")[1].split(". MSE")[0]) for l in lines])


def metric_errors(model, idiv, ref, it=0):
    """relative errors of iteration it's four metrics against the restatement's metrics dict"""
    got = {"MSE": model.all_performances["MSE"][it], "R^2": model.all_performances["R^2"][it], "Rp": model.all_performances["Rp"][it],
           "I_div": idiv[it]}
    return {m: abs(got[m] - ref[m]) / abs(ref[m]) for m in got}


def check(errs, tol, record_property, prefix=""):
    for name, e in errs.items():
        record_property(prefix + name, "%.3e" % e)
    bad = {n: e for n, e in errs.items() if not e <= tol}
    assert not bad, (bad, tol)


def f32(X):
    return np.asarray(X, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------- every sweep instance at its edges, one iteration
@pytest.mark.parametrize("I,J,K", CASES)
def test_nmf_iteration_at_launch_edges(I, J, K, capsys, record_property):
    R, M, U0, V0 = nmf_case(I, J, K)
    n = NMF(R, M, K, verbose=False)
    n.U, n.V = U0.copy(), V0.copy()
    idiv = run_capturing_idiv(n, 1, capsys)
    U, V = NR.ref_nmf_iteration(R, M, U0, V0)
    errs = {"U": NR.rel_err(n.U, U), "V": NR.rel_err(n.V, V)}
    errs.update(metric_errors(n, idiv, NR.metrics(R, M, U @ V.T)))
    n.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- the 16 384 limit
@pytest.mark.parametrize("I,J", [(16384, 5), (5, 16384)])
def test_longest_rows_and_columns_run(I, J, capsys, record_property):
    R, M, U0, V0 = NR.edge_problem(I, J, 2, seed=I + J, sparse=True)
    n = NMF(R, M, 2, verbose=False)
    n.U, n.V = U0.copy(), V0.copy()
    idiv = run_capturing_idiv(n, 1, capsys)
    U, V = NR.ref_nmf_iteration(R, M, U0, V0)
    errs = {"U": NR.rel_err(n.U, U), "V": NR.rel_err(n.V, V)}
    errs.update(metric_errors(n, idiv, NR.metrics(R, M, U @ V.T)))
    n.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- NMTF with K != L and I > 1024
@pytest.mark.parametrize("I,J,K,L", NMTF_CASES)
def test_nmtf_iteration_k_not_l(I, J, K, L, capsys, record_property):
    R, M, F0, S0, G0 = nmtf_case(I, J, K, L)
    t = NMTF(R, M, K, L, verbose=False)
    t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
    idiv = run_capturing_idiv(t, 1, capsys)
    F, S, G = NR.ref_nmtf_iteration(R, M, F0, S0, G0)
    errs = {"F": NR.rel_err(t.F, F), "S": NR.rel_err(t.S, S), "G": NR.rel_err(t.G, G)}
    errs.update(metric_errors(t, idiv, NR.metrics(R, M, F @ S @ G.T)))
    t.close()
    check(errs, TOL_ONE, record_property)


@pytest.mark.parametrize("I,J,K,L", NMTF_CASES)
def test_nmtf_single_updates_k_not_l(I, J, K, L, record_property):
    """update_S(K-1, L-1), update_S(0, L-1), update_F(K-1), update_G(L-1), each from the same start: only its own entry or
    column moves (the rest keep their bits), and to the restatement's value."""
    R, M, F0, S0, G0 = nmtf_case(I, J, K, L)
    t = NMTF(R, M, K, L, verbose=False)
    start = {"F": f32(F0), "S": f32(S0), "G": f32(G0)}
    errs = {}
    for name, call, ref, which, idx in [
        ("S%d,%d" % (K - 1, L - 1), lambda: t.update_S(K - 1, L - 1), lambda: NR.update_S(R, M, F0, S0, G0, K - 1, L - 1), "S", (K - 1, L - 1)),
        ("S0,%d" % (L - 1), lambda: t.update_S(0, L - 1), lambda: NR.update_S(R, M, F0, S0, G0, 0, L - 1), "S", (0, L - 1)),
        ("F%d" % (K - 1), lambda: t.update_F(K - 1), lambda: NR.update_F(R, M, F0, S0, G0, K - 1), "F", (slice(None), K - 1)),
        ("G%d" % (L - 1), lambda: t.update_G(L - 1), lambda: NR.update_G(R, M, F0, S0, G0, L - 1), "G", (slice(None), L - 1)),
    ]:
        t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
        call()
        for n in "FSG":
            got, want = getattr(t, n), start[n]
            keep = np.ones(got.shape, dtype=bool)
            if n == which:
                keep[idx] = False
            assert np.array_equal(got[keep], want[keep]), (name, n)
        errs[name] = NR.rel_err(getattr(t, which)[idx], ref()[idx])
    t.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- the update hooks at wide rank
@pytest.mark.parametrize("I,J,K", [(45, 2049, 256), (3, 8193, 65)])
def test_nmf_update_hooks_wide_rank(I, J, K, record_property):
    R, M, U0, V0 = nmf_case(I, J, K)
    n = NMF(R, M, K, verbose=False)
    errs = {}
    for which in "UV":
        for k in (0, 63, 64, K - 1):
            n.U, n.V = U0.copy(), V0.copy()
            (n.update_U if which == "U" else n.update_V)(k)
            ref = (NR.update_U if which == "U" else NR.update_V)(R, M, U0, V0, k)
            got, other = (n.U, n.V) if which == "U" else (n.V, n.U)
            start, other0 = (U0, V0) if which == "U" else (V0, U0)
            rest = np.arange(K) != k
            assert np.array_equal(got[:, rest], f32(start)[:, rest]), (which, k)
            assert np.array_equal(other, f32(other0)), (which, k)
            errs["%s%d" % (which, k)] = NR.rel_err(got[:, k], ref[:, k])
    n.close()
    check(errs, TOL_ONE, record_property)


# ---------------------------------------------------------------- drift, predict() and compute_I_div()
def held_out(M):
    Mp = ~M
    assert Mp.any()
    return Mp.astype(float)


def predict_errors(model, R, Mtrain, P):
    p = model.predict(held_out(Mtrain))
    ref = NR.metrics(R, ~Mtrain, P)
    errs = {"pred_" + m: abs(p[m] - ref[m]) / abs(ref[m]) for m in ("MSE", "R^2", "Rp")}
    errs["compute_I_div"] = abs(model.compute_I_div() - NR.metrics(R, Mtrain, P)["I_div"]) / abs(NR.metrics(R, Mtrain, P)["I_div"])
    return errs


@pytest.mark.parametrize("I,J,K", [(2050, 4099, 24), (21, 16384, 256)])
def test_nmf_five_iterations(I, J, K, capsys, record_property):
    R, M, U0, V0 = nmf_case(I, J, K)
    n = NMF(R, M, K, verbose=False)
    n.U, n.V = U0.copy(), V0.copy()
    idiv = run_capturing_idiv(n, 5, capsys)
    U, V = U0, V0
    errs = {}
    for it in range(5):
        U, V = NR.ref_nmf_iteration(R, M, U, V)
        for m, e in metric_errors(n, idiv, NR.metrics(R, M, U @ V.T), it).items():
            errs["%s_%d" % (m, it)] = e
    errs.update({"U": NR.rel_err(n.U, U), "V": NR.rel_err(n.V, V)})
    errs.update(predict_errors(n, R, M, U @ V.T))
    n.close()
    check(errs, TOL_DRIFT, record_property)


def test_nmtf_five_iterations(capsys, record_property):
    I, J, K, L = NMTF_CASES[0]
    R, M, F0, S0, G0 = nmtf_case(I, J, K, L)
    t = NMTF(R, M, K, L, verbose=False)
    t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
    idiv = run_capturing_idiv(t, 5, capsys)
    F, S, G = F0, S0, G0
    errs = {}
    for it in range(5):
        F, S, G = NR.ref_nmtf_iteration(R, M, F, S, G)
        for m, e in metric_errors(t, idiv, NR.metrics(R, M, F @ S @ G.T), it).items():
            errs["%s_%d" % (m, it)] = e
    errs.update({"F": NR.rel_err(t.F, F), "S": NR.rel_err(t.S, S), "G": NR.rel_err(t.G, G)})
    errs.update(predict_errors(t, R, M, F @ S @ G.T))
    t.close()
    check(errs, TOL_DRIFT, record_property)


# ---------------------------------------------------------------- the same bits on two runs
def test_same_bits_e16_and_grid_stride_s_step(capsys):
    I, J, K = 21, 16384, 256
    R, M, U0, V0 = nmf_case(I, J, K)
    out = []
    for _ in range(2):
        n = NMF(R, M, K, verbose=False)
        n.U, n.V = U0.copy(), V0.copy()
        idiv = run_capturing_idiv(n, 3, capsys)
        out.append([n.U, n.V, np.array([n.all_performances[m] for m in ("MSE", "R^2", "Rp")]), idiv, np.array(n.compute_I_div())])
        n.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    I, J, K, L = NMTF_CASES[0]
    R, M, F0, S0, G0 = nmtf_case(I, J, K, L)
    out = []
    for _ in range(2):
        t = NMTF(R, M, K, L, verbose=False)
        t.F, t.S, t.G = F0.copy(), S0.copy(), G0.copy()
        idiv = run_capturing_idiv(t, 3, capsys)
        out.append([t.F, t.S, t.G, np.array([t.all_performances[m] for m in ("MSE", "R^2", "Rp")]), idiv, np.array(t.compute_I_div())])
        t.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
