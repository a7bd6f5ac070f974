"""The cases of the step-by-step test of the variational S pass (tests/_s_pass_cases.py; GPU side: test_s_pass_gpu.py) cover what
they claim, the NumPy fp32 restatement of both chain kernels passes checks (a) and (b), and the same restatement with one fault
at a time fails one of them on every case the fault can occur on: the checks would notice a wave that misses one block's deltas,
a dropped tail step, a wrong row, a stale LDS region, a wrong table segment, a wrong fast-path threshold, a missing fall-back
and a stored mean taken from the table."""
import numpy as np
import pytest

import _s_pass_cases as SP
from _s_pass_cases import BLOCKED_SHAPES, CASES, FAULTS, HOOK_SHAPE, HOOK_TAUS, HOOK_X, OBSERVED_CASES, STEP_SHAPES

IDS = [c.id for c in CASES]


def test_the_launch_rule_and_the_shapes():
    assert [K * L for K, L in STEP_SHAPES] == [1, 12, 13, 25, 63]
    assert [K * L for K, L in BLOCKED_SHAPES] == [64, 65, 66, 195, 192, 256, 961, 992, 1024]
    for K, L in STEP_SHAPES:
        assert SP.chain_kernel(K, L) == "steps"
    for K, L in BLOCKED_SHAPES:
        assert SP.chain_kernel(K, L) == "blocked"
        assert SP.chain_kernel(K, L, n_order=1, only_params=False) == "steps"          # the single-step hook
        assert SP.chain_kernel(K, L, only_params=True) == "steps"
        assert SP.chain_kernel(K, L, steps_switch=True) == "steps"
    # two orders per shape, one of them not the identity (1 x 1 has only one), exptau = 1 and two other powers of two
    for K, L in STEP_SHAPES + BLOCKED_SHAPES:
        mine = [c for c in CASES if (c.K, c.L) == (K, L)]
        assert len(mine) == 2
        o = [SP.order_of(c) for c in mine]
        assert sorted(o[1].tolist()) == list(range(K * L))
        assert K * L == 1 or (not np.array_equal(o[0], o[1]) and np.array_equal(o[0], np.arange(K * L)))
    assert {c.tau for c in CASES} == {1.0, 0.25, 8.0}
    assert len(OBSERVED_CASES) == 3 and all(c.kernel == "blocked" and c.variant == 1 for c in OBSERVED_CASES)
    # the systems stay small: the size of the 140 x 17 case of _ssys_cases.py, J grown only to give every column of G two rows
    assert SP.SIZE_I == 140 and SP.size_J(1) == 17 and SP.size_J(32) == 67


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_conditions(case):
    st = SP.case_conditions(case)
    reg = SP.regime(st.x)
    print("%s: %s" % (case.id, {r: int((reg == r).sum()) for r in ("fast", "neg", "tab", "far", "beyond")}))


def test_coverage_over_all_shapes():
    segs, places, patterns = SP.global_coverage()
    print(len(segs), sorted(places), sorted(patterns))


def test_the_reference_moments():
    """tn_moments_ref against 40-digit values, across the regimes and both branches"""
    import mpmath as mp          # (the generators under tools/ that the restatement loads need it anyway)
    mp.mp.dps = 40
    for x in (-40.0, -12.0, -6.0, -1e-3, 0.0, 1e-3, 3.0, 12.0, 25.9, 29.9):
        for tau in (2.0 ** -10, 1.0, 2.0 ** 20):
            mu = -x / np.sqrt(tau)
            e, v, xr, _, _ = SP.tn_moments_ref(mu, tau)
            xm, sg = -mp.mpf(mu) * mp.sqrt(mp.mpf(tau)), 1 / mp.sqrt(mp.mpf(tau))
            lam = mp.npdf(xm) / (mp.erfc(xm / mp.sqrt(2)) / 2)
            assert abs(mp.mpf(float(e)) / (sg * (lam - xm)) - 1) < 1e-12
            assert abs(mp.mpf(float(v)) / (sg * sg * (1 - lam * (lam - xm))) - 1) < 1e-9
    e, v, x, fe, fv = SP.tn_moments_ref(-35.0, 1.0)
    assert fe == 1 / 35.0 and fv == fe * fe


def test_kseg_minus_one_is_not_reachable():
    """The blocked kernel's step that fails nm >= thr and still lands below segment 0 (_s_pass_cases.py: why not): the largest fp32
    nm below thr = RN(6 / hh) gives xq = fma(nm, -2 hh, 12) >= 0, for hh over the range of sqrt(1 / tauS)."""
    rs = np.random.RandomState(5)
    hh = np.exp(rs.uniform(np.log(2.0 ** -12), np.log(2.0 ** 6), 200000)).astype(np.float32)
    thr = (np.float32(6.0) / hh).astype(np.float32)
    nm = np.nextafter(thr, np.float32(0))
    xq = SP.fma32(nm, -hh * np.float32(2.0), np.float32(12.0))
    assert (nm < thr).all() and (xq >= 0).all() and (np.floor(xq) == 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_passes_and_every_fault_fails(case):
    st = SP.steered(case)
    (ra_e, ra_v, rb), fails = SP.check_all(case, st.lam, *SP.chain_f32(case, st.lam))
    print("%s: largest difference / bound  (a) mean %.3f variance %.3f  (b) %.3f" % (case.id, ra_e, ra_v, rb))
    assert not fails, fails
    for fault in FAULTS:
        if not SP.fault_applies(fault, case):
            continue
        ratios, fails = SP.check_all(case, st.lam, *SP.chain_f32(case, st.lam, fault))
        print("    %-20s (a) %.3g %.3g  (b) %.3g  %s" % (fault, *ratios, "; ".join(fails)))
        assert fails, "%s: the checks do not notice %s" % (case.id, fault)


def test_every_fault_occurs_somewhere():
    for fault in FAULTS:
        on = [c.id for c in CASES if SP.fault_applies(fault, c)]
        assert on, fault
        # the faults of the arithmetic occur on every blocked shape, the faults of the walk on every shape that has the structure
        if fault in ("segment_off_by_one", "fast_to_minus_4", "no_fallback", "stored_from_table"):
            assert all(SP.fault_applies(fault, c) for c in CASES if c.kernel == "blocked"), fault
    assert all(SP.fault_applies("fast_to_minus_4", c) for c in CASES if c.n > 1)


def test_hook_grid():
    K, L = HOOK_SHAPE
    assert SP.chain_kernel(K, L, n_order=1) == "steps" and K * L >= len(HOOK_X)
    _, _, s = SP.system(K, L)
    assert s.ok.all()
    lo, hi = np.inf, 0.0
    for tau in HOOK_TAUS:
        lam, x, tauS = SP.hook_lambda(tau)
        lo, hi = min(lo, tauS.min()), max(hi, tauS.max())
        # the single step in NumPy fp32 passes check (a); moderate exptau: the grid is hit to 1e-4 (a large one: lambda's own fp32
        # spacing against tau s moves x, the check takes whatever (muS, tauS) come back)
        if 2.0 ** -7 <= tau <= 1.0:
            assert np.abs(x - np.array([HOOK_X[a % len(HOOK_X)] for a in range(K * L)])).max() < 1e-4
        mu, tq, E, V = SP.hook_f32(tau, lam)
        ra_e, ra_v, bad = SP.check_moments(mu, tq, E, V)
        assert bad.size == 0, (tau, bad, ra_e, ra_v)
    assert lo <= 2.0 ** -10 and hi >= 2.0 ** 20
