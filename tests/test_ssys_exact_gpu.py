"""The tri-factorisation's S system (csrc/kernel_ssys.hip) checked bit for bit at every launch shape.

Through the conditional hook bnmtf_cond_params(which = 1) -- the whole system rebuilt for the state, then (numer_a, tauS_a) of
one entry -- on integer grids where every intermediate is an integer below 2^24 (tests/_ssys_cases.py; the CPU side,
test_ssys_cases_cpu.py, lists the budget, shows that each split product, missing entry, slot, range, mirror write, tri_pos
tile, b block and the S_a A_aa term would move a checked output, and that the cases cover the launch edges).  Every checked
entry (k, l) of every state must come back exact, on the dense system, on the per-row path (BNMTF_SSYS=0) and, for the
variational model, through update_S."""
import re

import numpy as np
import pytest

from bnmtf_amd import bnmtf_gibbs_optimised, bnmtf_vb_optimised
from _ssys_cases import CASES, LAM, MU_ULPS, System, describe_fields, gibbs_states, problem, row_path_ok, vb_states

pytestmark = pytest.mark.gpu

PRI_TRI = dict(alpha=1., beta=1., lambdaF=LAM, lambdaS=LAM, lambdaG=LAM)
_SSYS = re.compile(r"ssys\[on=(\d)(?: nsplit=(\d+) range=(\d+) bblocks=(\d+))?\]")
DENSE = [c for c in CASES if c.dense]


def _ssys_fields(model):
    m = _SSYS.findall(model.describe())
    assert len(m) == 1, model.describe()
    on, nsplit, per, bblocks = m[0]
    return dict(on=int(on)) if on == "0" else dict(on=1, nsplit=int(nsplit), range=int(per), bblocks=int(bblocks))


def _all_cond(model, st):
    """(numer, tau) of every entry a = k L + l for the state, set on the device with tau = 1"""
    model.F, model.S, model.G = (x.astype(np.float64) for x in (st.F, st.S, st.G))
    model.tau = 1.0
    K, L = st.S.shape
    numer, tau = np.zeros(K * L), np.zeros(K * L)
    for k in range(K):
        for l in range(L):
            n, t = model._cond(1, k, l, 1)
            numer[k * L + l], tau[k * L + l] = n[0], t[0]
    return numer, tau


def _check(what, L, got, want, ok):
    bad = np.flatnonzero((got != want) & ok)
    assert bad.size == 0, "%s: %d of %d checked entries wrong, first (k, l): %s, got %r, want %r" % (
        what, bad.size, int(ok.sum()), [divmod(int(a), L) for a in bad[:4]], got[bad[:4]].tolist(), want[bad[:4]].tolist())


def _run_gibbs(case, row_path):
    p = problem(case)
    model = bnmtf_gibbs_optimised(p.R, p.M, case.K, case.L, PRI_TRI, verbose=False, seed=1)
    try:
        checked = 0
        for st in gibbs_states(p):
            s = System(p, st)
            ok = row_path_ok(p, st, s) if row_path else s.ok
            if not ok.any():
                continue
            numer, tau = _all_cond(model, st)
            _check("%s %s numer" % (case.id, st.fam), case.L, numer, s.numer.astype(np.float64), ok)
            _check("%s %s tauS" % (case.id, st.fam), case.L, tau, s.tau, ok)
            checked += int(ok.sum())
        assert checked > 0
        # the case ran where it means to: the dense system with its ranges and b blocks, or the per-row path
        want = describe_fields(case.launch()) if not row_path else dict(on=0)
        assert _ssys_fields(model) == want, model.describe()
    finally:
        model.close()


@pytest.mark.parametrize("case", DENSE, ids=[c.id for c in DENSE])
def test_dense_system_is_exact(case):
    _run_gibbs(case, row_path=False)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_per_row_path_is_exact(case, monkeypatch):
    monkeypatch.setenv("BNMTF_SSYS", "0")          # (read when the model is built)
    _run_gibbs(case, row_path=True)


VB_CASES = [c for c in CASES if c.vb]


@pytest.mark.parametrize("case", VB_CASES, ids=[c.id for c in VB_CASES])
def test_variational_system_is_exact(case):
    """update_S(k, l) (moments = 0) on the second-moment system: scol_gram_kernel<1, 1> (the missing rows' variances),
    gamma_pack with varG, C~f's diagonal from the column sums of the second moments.  tauS bit for bit; muS within MU_ULPS ulps
    of numer / tauS (ssys_chain_vb_kernel multiplies by a rounded reciprocal: two roundings)."""
    p = problem(case)
    K, L = case.K, case.L
    model = bnmtf_vb_optimised(p.R, p.M, K, L, PRI_TRI, verbose=False)
    try:
        for st in vb_states(p):
            s = System(p, st, vb=True)
            model.expF, model.varF = st.F.astype(np.float64), st.varF.astype(np.float64)
            model.expG, model.varG = st.G.astype(np.float64), st.varG.astype(np.float64)
            model.expS, model.varS = st.S.astype(np.float64), np.ones((K, L))
            for n, shape in (("muF", (case.I, K)), ("tauF", (case.I, K)), ("muG", (case.J, L)), ("tauG", (case.J, L)),
                             ("muS", (K, L)), ("tauS", (K, L))):
                setattr(model, n, np.ones(shape))
            model.exptau = 1.0
            mu, tau = np.zeros(K * L), np.zeros(K * L)
            for k in range(K):
                for l in range(L):
                    model.update_S(k, l)
                    mu[k * L + l], tau[k * L + l] = model.muS[k, l], model.tauS[k, l]
                    model.expS = st.S.astype(np.float64)          # (update_S leaves the moments alone; the pull brings them back)
            _check("%s VB tauS" % case.id, L, tau, s.tau, s.ok)
            q = (s.num - LAM) / s.tau
            ulp = np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
            err = np.abs(mu - q) / ulp
            bad = np.flatnonzero((err > MU_ULPS) & s.ok)
            assert bad.size == 0, "%s VB muS: %d entries beyond %d ulps, first (k, l): %s, err %r ulps" % (
                case.id, bad.size, MU_ULPS, [divmod(int(a), L) for a in bad[:4]], err[bad[:4]].tolist())
            print("%s VB muS: max %.2f ulps over %d entries" % (case.id, err[s.ok].max(), int(s.ok.sum())))
    finally:
        model.close()
