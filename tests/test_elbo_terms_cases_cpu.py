"""The cases and the reference of tests/test_elbo_terms_gpu.py (tests/_elbo_terms_cases.py), without a GPU: the host restatement
of the factor sums gives the oracle's ELBO; every case's state stays clear of the erfc band for the iterations the GPU file checks,
with the planted entries the only dead ones (three shapes with fewer than four units: and the listed entries they starve);
the residual form that stands in for the oracle on the large tri-factorisation shapes is the oracle's sweep; the pair-panel, on-chip and list-form cases keep their kernel and block shape by the
host slot layout and cover every unit count modulo four; and the defects the GPU file is there for each move a sum by more than
1000 tolerances."""
import math

import numpy as np
import pytest
from scipy.special import gammaln

import _elbo_terms_cases as E
from _slot_layout import slot_layout

LOG2PI = math.log(2 * math.pi)


# ------------------------------------------------------------------------------------------------ the reference against the oracle
def _case(name):
    return next(c for c in E.ALL_CASES if c.name == name)


def _elbo_from_sums(o, widths, sums, extra=0.0):
    """the scalar part of elbo() (bnmf_vb_optimised.py:163-177, bnmtf_vb_optimised.py:208-223) around the factor sums:
    sums = ((lambda, (quad, log erfc, log tau, lambda E)), ...) of the outer factors, extra = the terms of S"""
    v = o.size_Omega / 2.0 * (o.explogtau - LOG2PI) - o.exptau / 2.0 * o.exp_square_diff() \
        + o.alpha * math.log(o.beta) - gammaln(o.alpha) + (o.alpha - 1.0) * o.explogtau - o.beta * o.exptau \
        - o.alpha_s * math.log(o.beta_s) + gammaln(o.alpha_s) - (o.alpha_s - 1.0) * o.explogtau + o.beta_s * o.exptau + extra
    for (lam, (quad, lerfc, ltau, lamx)), n in zip(sums, widths):
        v += np.log(lam).sum() - lamx - 0.5 * ltau + n / 2.0 * LOG2PI + lerfc + quad
    return v


def _oracle_after(case, variant, iterations):
    p = case.problem(variant)
    o = case.oracle(p)
    for it in range(iterations):
        case.oracle_sweep(o, p, it)
    return p, o


@pytest.mark.parametrize("name", ["generic_5x7_K3", "vb_pairs", "tri_generic_5x7_K2_L3", "obs_tri_KL7x9"])
def test_factor_sums_give_the_oracles_elbo(name):
    """factor_sums of the oracle's state (fp64 values that are no fp32 values: the oracle's state rounded to fp32 is fed to both)
    inside the scalar part of elbo() is the oracle's own elbo() to 1e-12; with a dead entry both are -inf."""
    case = _case(name)
    for variant in E.VARIANTS:
        p, o = _oracle_after(case, variant, 2)
        for f in (case.first, case.second) + (("S",) if case.tri else ()):
            for n in ("mu", "tau", "exp", "var"):
                setattr(o, n + f, E.widen(getattr(o, n + f)))
        want = o.elbo()
        I, J = p.M.shape
        sums = [(lam, E.factor_sums(*E.factor_state(o, f), lam)[0]) for f, lam in zip((case.first, case.second), p.lam)]
        extra = 0.0
        if case.tri:
            with np.errstate(all="ignore"):
                extra = np.log(o.lambdaS).sum() - (o.lambdaS * o.expS).sum() - 0.5 * np.log(o.tauS).sum() + p.K * p.L / 2.0 * LOG2PI \
                    + np.log(0.5 * E.scipy.special.erfc(-o.muS * np.sqrt(o.tauS) / math.sqrt(2))).sum() + (o.tauS / 2.0 * (o.varS + (o.expS - o.muS) ** 2)).sum()
        got = _elbo_from_sums(o, (I * case.widths()[0], J * case.widths()[1]), sums, extra)
        if variant == "dead":
            assert want == -np.inf and got == -np.inf, (want, got)
        else:
            assert np.isfinite(want) and abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_a_term_of_minus_infinity_gives_minus_infinity():
    mu, tau = np.array([[1.0, -40.0]]), np.array([[1.0, 2.0]])
    s, a = E.factor_sums(mu, tau, np.ones((1, 2)), np.ones((1, 2)), np.ones((1, 2)))
    assert s[1] == -np.inf and np.isfinite(s[[0, 2, 3]]).all() and np.isfinite(a).all()
    assert a[1] == abs(math.log(0.5 * math.erfc(-1.0 / math.sqrt(2))))
    ordinary, band, dead = E.classify(mu, tau)
    assert ordinary.tolist() == [[True, False]] and dead.tolist() == [[False, True]] and not band.any()
    assert E.classify(np.array([-27.0]), np.array([2.0]))[1].all()


# ------------------------------------------------------------------------------------------------ the inputs are valid
@pytest.mark.parametrize("name", ["tri_generic_7x8_K4_L5", "tri_pairs_211x153_K6_L9", "obs_tri_KL5x13", "obs_tri_rows"])
def test_residual_form_of_the_tri_sweep_is_the_oracles_sweep(name):
    """tri_sweep_residual_form, which stands in for the as-written oracle on the three large shapes, against that oracle: every q
    parameter after each of three iterations in permuted orders, scaled by the array's largest value, to 1e-11 (the two add the
    same fp64 terms in another order; 3e-13 is the largest difference seen)."""
    case = _case(name)
    for variant in E.VARIANTS:
        p = case.problem(variant)
        a, b = case.oracle(p), case.oracle(p)
        for it in range(E.ITERATIONS):
            od = E.TC.oracle_orders(p.orders[it], p.K, p.L)
            a.sweep(*od)
            E.tri_sweep_residual_form(b, *od)
            for n in E.TC.NAMES:
                x, y = getattr(a, n), getattr(b, n)
                assert np.abs(x - y).max() <= 1e-11 * max(1.0, np.abs(x).max()), (name, variant, it, n)
            assert abs(a.exptau / b.exptau - 1) <= 1e-12 and abs(a.beta_s / b.beta_s - 1) <= 1e-12


def test_the_large_tri_shapes_take_the_residual_form():
    big = {c.name for c in E.ALL_CASES if c.tri and c.problem("finite").M.size > E.RESIDUAL_FORM_FROM}
    assert big == {"tri_%s_%dx%d_K%d_L%d" % ((k,) + s) for k in ("generic", "pairs") for s in E.TRI_SHARED}


_KEYS = sorted({c.problem_key for c in E.ALL_CASES})


@pytest.mark.parametrize("variant", E.VARIANTS)
@pytest.mark.parametrize("key", _KEYS)
def test_no_entry_near_the_band(key, variant):
    """The fp64 oracle from the case's state, the iterations the GPU file checks: no entry of either factor at 25 <= w <= 29 (the
    band widened by one on each side: the device's state differs from the oracle's by up to 5e-4), none above 29 in the finite
    variant, exactly the planted ones in the dead variant."""
    case = next(c for c in E.ALL_CASES if c.problem_key == key)
    p = case.problem(variant)
    o = case.oracle(p)
    for it in range(E.ITERATIONS):
        case.oracle_sweep(o, p, it)
        E.check_entries(case, p, variant, o, 1.0, "oracle it %d" % (it + 1), it + 1)
        ref = E.reference_sums(case, p, o)[0]
        assert np.isfinite(ref[[0, 2, 3, 4, 6, 7]]).all() and (np.isfinite(ref[[1, 5]]).all() if variant == "finite" else (ref[[1, 5]] == -np.inf).all()), ref


def test_cases_of_one_key_have_one_problem():
    for key in _KEYS:
        cs = [c for c in E.ALL_CASES if c.problem_key == key]
        for c in cs[1:]:
            a, b = cs[0].problem("dead"), c.problem("dead")
            assert (a.R == b.R).all() and (a.M == b.M).all() and (a.K, a.L) == (b.K, b.L) and all((a.state[n] == b.state[n]).all() for n in a.state)


# ------------------------------------------------------------------------------------------------ paths, block shapes, unit counts
def _mod4(cases):
    return ({c.problem("finite").M.shape[0] % 4 for c in cases}, {c.problem("finite").M.shape[1] % 4 for c in cases})


@pytest.mark.parametrize("hc", E.HANDOVER_BASE + E.HANDOVER_MOVED + E.HANDOVER_KP64, ids=E.ids(E.HANDOVER_BASE + E.HANDOVER_MOVED + E.HANDOVER_KP64))
def test_panel_cases_keep_their_kernel_and_block_shape(monkeypatch, hc):
    """what api_models.inc enqueue_vb_sweep asks of a direction's layout before it leaves the generic kernel, and the block shape"""
    hc.setenv(monkeypatch)
    for L, nw in zip(hc.layouts(), hc.nw):
        assert L.wide_can and L.pair_ok and len(L.gen_units) == 0 and L.nch == 1, hc.name
        assert L.use_wide == (nw == 16), (hc.name, L.use_wide, nw)
        assert L.vb_path == {"masked": 1, "pairs": 2}[hc.env["BNMTF_VB_PATH"]]


def test_list_form_cases_are_batchable_by_their_layouts(monkeypatch):
    """api_many.inc vb_batchable: both directions on the pair-panel kernel in its 8-wave shape, no switch set"""
    E.MANY_CASES[0].setenv(monkeypatch)
    for c in E.MANY_CASES:
        miss = c.problem("finite").M == 0
        for L in (slot_layout(miss, KP=32), slot_layout(np.ascontiguousarray(miss.T), KP=32)):
            assert L.wide_can and L.pair_ok and len(L.gen_units) == 0 and not L.use_wide and L.vb_path == 0, c.name
    assert [c.problem("finite").M.shape[0] % 4 for c in E.MANY_CASES] == [1, 2, 0] and len({c.K for c in E.MANY_CASES}) == 3


def test_unit_counts_cover_every_remainder():
    full = {0, 1, 2, 3}
    assert _mod4(E.GENERIC_CASES)[0] | _mod4(E.GENERIC_CASES)[1] == full
    assert {(32 if c.K <= 32 else 64, c.K in (32, 64)) for c in E.GENERIC_CASES} == {(32, False), (32, True), (64, False), (64, True)}
    for producer in ("vb_pieces_kernel", "vb_pieces_slabs_kernel"):
        rows, cols = _mod4([c for c in E.PANEL_CASES if c.producer == producer])
        assert rows == full and cols == full, (producer, rows, cols)
    for nw in ((16, 16), (8, 8)):
        rows, cols = _mod4([c for c in E.PANEL_CASES if c.producer == "vb_pieces_slabs_kernel" and c.nw == nw])
        assert rows >= {1, 3} and cols >= {1, 3}, (nw, rows, cols)
    # vb_pieces_kernel and vb_pieces_slabs_kernel at K = KP and K < KP, at KP = 32 and at KP = 64 (the tri-factorisation: KP = 32)
    for producer in ("vb_pieces_kernel", "vb_pieces_slabs_kernel"):
        widths = {w for c in E.PANEL_CASES + E.TRI_PAIRS if c.producer == producer for w in c.widths()}
        assert widths & {32, 64} and any(w < 32 for w in widths) and any(32 < w <= 64 for w in widths), (producer, widths)
    assert {(c.K, c.L) for c in E.TRI_PAIRS} >= {(32, 32), (5, 32)} and {(c.K, c.L) for c in E.TRI_GENERIC} >= {(32, 32), (5, 32)}
    rows, cols = _mod4(E.TRI_PAIRS)
    assert rows == full and cols >= {0, 1, 3}
    rows, cols = _mod4(E.TRI_GENERIC)
    assert rows | cols == full
    assert {c.name[4:] for c in E.OBS_CASES} == set(E.OBS_SHAPES) and {c.name[8:] for c in E.OBS_TRI_CASES} == set(E.TC.CASES)
    assert len({c.name for c in E.ALL_CASES}) == len(E.ALL_CASES)


# ------------------------------------------------------------------------------------------------ the test can fail
def _sums_of(state, lam):
    return E.factor_sums(*state, lam)


def test_the_defects_move_a_sum_by_a_thousand_tolerances():
    """On the first factor of vb_pairs_p1p3 (71 units: the last block of four holds three) after one oracle sweep, dead variant for
    lambda: the last unit dropped, the last block of four dropped, a padding column of zeros with tau = 0 counted, lambda taken
    from the unit before."""
    case = _case("vb_pairs_p1p3")
    tol = np.array(E.TOLS)

    def moved(a, b, scale):
        return np.abs(np.asarray(a) - np.asarray(b)) / (tol * scale)

    p, o = _oracle_after(case, "finite", 1)
    st = E.factor_state(o, "U")
    n = st[0].shape[0]
    assert n % 4 == 3
    full, full_abs = _sums_of(st, p.lam[0])
    for keep in (n - 1, 4 * ((n - 1) // 4)):                                  # the last unit; the last block of four
        part = _sums_of([x[:keep] for x in st], p.lam[0][:keep])[0]
        assert (moved(part, full, full_abs) > 1000).all(), (keep, moved(part, full, full_abs))
    pad = _sums_of([np.concatenate([x, np.zeros((n, 1))], axis=1) for x in st], np.concatenate([p.lam[0], np.zeros((n, 1))], axis=1))[0]
    assert pad[2] == -np.inf                                                   # log tau of the padding column
    assert moved(pad[1], full[1], full_abs[1])[1] > 1000                       # ... and n log(1/2) in the log erfc sum
    assert pad[0] == full[0] and pad[3] == full[3]
    # lambda of the wrong unit: visible where lambda differs between units -- the dead variant's planted entry
    p, o = _oracle_after(case, "dead", 1)
    st = E.factor_state(o, "U")
    full, full_abs = _sums_of(st, p.lam[0])
    shifted = _sums_of(st, np.roll(p.lam[0], 1, axis=0))[0]
    assert moved(shifted[3], full[3], full_abs[3])[3] > 1000
    assert full[1] == -np.inf and shifted[1] == -np.inf and (shifted[[0, 2]] == full[[0, 2]]).all()
