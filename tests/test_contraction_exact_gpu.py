"""The masked contraction (K1 / K2: csrc/kernel_gemm.hip, gemm_bf16x3_body) checked bit for bit at every launch shape.

Through the conditional hook (bnmf_cond_params / bnmtf_cond_params: the real K1 / K2 launch, then the generic sweep for one
column) on integer grids where every partial sum is an integer below 2^24 (tests/_contraction_cases.py; the CPU side,
test_contraction_cases_cpu.py, shows that the cases meet that budget and that each retained split product, a step read twice
and a lost inner slice would move a checked output), so that the only correct fp32 result is the exact one.  Then, on data
with full 24-bit significands, a bound on the rounding error that pins the accumulation order."""
import re

import numpy as np
import pytest

from bnmtf_amd import bnmf_gibbs_optimised, bnmtf_gibbs_optimised
from _contraction_cases import CASES, LAM, exact, operands, problems

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=LAM, lambdaV=LAM)
PRI_TRI = dict(alpha=1., beta=1., lambdaF=LAM, lambdaS=LAM, lambdaG=LAM)
_DESC = re.compile(r"(rows|cols)\[n=(\d+) n_pad=(\d+) split=(\d+) ipw=(\d+)")


def _launches(model):
    return {g[0]: dict(n_pad=int(g[2]), split=int(g[3]), ipw=int(g[4])) for g in _DESC.findall(model.describe())}


def _cond(model, state, k):
    """(numer, tau) of column k of the state's direction, the state set on the device with tau = 1"""
    d = state[0]
    if len(state) == 4:
        model.F, model.S, model.G = (x.astype(np.float64) for x in state[1:])
        model.tau = 1.0
        return model._cond(0, k, 0, model.I) if d == "rows" else model._cond(2, 0, k, model.J)
    model.U, model.V = state[1].astype(np.float64), state[2].astype(np.float64)
    model.tau = 1.0
    return model._cond(0 if d == "rows" else 1, k)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_contraction_is_exact_at_every_launch_shape(case):
    for p in problems(case):
        if case.L:
            model = bnmtf_gibbs_optimised(p.R, p.M, case.K, case.L, PRI_TRI, verbose=False, seed=1)
        else:
            model = bnmf_gibbs_optimised(p.R, p.M, case.K, PRI, verbose=False, seed=1)
        try:
            for st in p.states:
                d = st[0]
                v, X, Y = operands(p, st)
                numer, _, tau, _, tau_ok = exact(v, X, Y)
                for k in range(X.shape[1]):
                    got, gtau = _cond(model, st, k)
                    bad = np.flatnonzero(got != numer[:, k])
                    assert bad.size == 0, "%s %s column %d: %d units wrong, first %s: %r, want %r" % (
                        p.fam, d, k, bad.size, bad[:4], got[bad[:4]], numer[bad[:4], k])
                    if tau_ok:
                        np.testing.assert_array_equal(gtau, tau[:, k], err_msg="%s %s tau column %d" % (p.fam, d, k))
                # the case is where it means to be: the launch's fields as the device built them
                want = case.expect[d]
                assert _launches(model)[d] == {f: want[f] for f in ("n_pad", "split", "ipw")}, (d, model.describe())
        finally:
            model.close()


# Full 24-bit significands: |numer - (P - lambda)| <= C_ROUND * 2^-24 * (|M o R| . |X_k|) for every unit and column.
# C_ROUND is about ten times the largest ratio measured on the MI355X: 3.79 (KP = 32), 3.71 (KP = 64, tw = 2), 3.90 (tw = 4).
C_ROUND = 40.0


@pytest.mark.parametrize("I,J,K", [(1000, 3000, 24), (1500, 3000, 48), (2100, 3000, 64)], ids=["KP32", "KP64-tw2", "KP64-tw4"])
def test_full_precision_contraction_stays_within_its_rounding_bound(I, J, K):
    rs = np.random.RandomState(I + K)
    R = rs.uniform(0.5, 8.0, (I, J)).astype(np.float32)
    M = (rs.random_sample((I, J)) < 0.7).astype(np.uint8)
    V = rs.uniform(0.25, 1.0, (J, K)).astype(np.float32)
    model = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, seed=1)
    try:
        model.U, model.V, model.tau = np.zeros((I, K)), V.astype(np.float64), 1.0
        Rt = np.where(M == 1, R, 0).astype(np.float64)
        P = Rt @ V.astype(np.float64)
        unit = 2.0 ** -24 * (np.abs(Rt) @ np.abs(V.astype(np.float64)))
        worst = 0.0
        for k in range(K):
            numer, _ = model._cond(0, k)
            worst = max(worst, float((np.abs(numer - (P[:, k] - LAM)) / unit[:, k]).max()))
        print("rounding %dx%dx%d %s: max |numer - fp64| / (2^-24 |M o R|.|X|) = %.3f" % (I, J, K, _launches(model)["rows"], worst))
        assert worst <= C_ROUND, worst
    finally:
        model.close()
