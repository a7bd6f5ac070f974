"""The eight factor sums of the variational record, all_elbo_terms[:, 2:10], term by term at every launch shape: each producer
(the generic sweep, vb_pieces_kernel, vb_pieces_many, vb_pieces_slabs_kernel, obs_vb_pieces<COV>) and each fold (vb_finish_body,
vb_finish_many, obs_vb_finish_kernel, obs_trivb_finish_kernel) against the host restatement of tests/_elbo_terms_cases.py on the
state the model itself returns.  The cases, the reference and what each case is there for: _elbo_terms_cases.py;
tests/test_elbo_terms_cases_cpu.py pins them to the fp64 oracle and shows that a dropped unit, a dropped block of four, a counted
padding column and a lambda of the wrong unit each move a sum by more than 1000 tolerances.

Every case runs from a seeded state, run(1) three times, in two variants: finite (all eight sums finite) and dead (two planted
entries whose erfc is exactly 0: the log erfc sums of both factors are -inf, the other six stay finite and are compared).  After
every call, on the returned state: no entry in the band of _elbo_terms_cases.BAND and the dead entries the planted ones (on the three shapes of
_elbo_terms_cases.STARVED also the entries listed there); each sum
within tol x sum |terms| of the reference, -inf exactly where the reference is -inf; beta_s = beta + exp_square_diff / 2 and
exptau = alpha_s / beta_s to one ulp; the ELBO of the dead variant -inf and not NaN.

Tolerances.  The quadratic, log tau and lambda E sums: 1e-9 (_elbo_terms_cases.TOL_SUM).  The log erfc sum compares the device
library's fp64 erfc and log with SciPy's.  The largest |device - reference| / sum |terms| over all finite cases and iterations,
measured on an MI355X against the SciPy reference, is 2.46e-14 (tri_generic_1100x900_K10_L7, first iteration: thousands of terms near
log 1, each carrying the 1e-16 granularity of erfc near 2, over a sum of absolute values that is small for the same reason); the
next largest are 3.3e-15 (generic_4x9_K1) and 2.3e-15 (obs_tri_KL5x26).  TOL_ERFC = 2.5e-12 is two decades above it.  The other
six sums were at most 6.4e-16 of their sums of absolute values."""
import re

import numpy as np
import pytest

import _elbo_terms_cases as E
from bnmtf_amd import bnmf_vb_observed, bnmf_vb_optimised, bnmtf_vb_observed, bnmtf_vb_optimised, run_many

pytestmark = pytest.mark.gpu

MEASURED_ERFC = 2.46e-14        # see above


def test_the_log_erfc_tolerance_is_two_decades_above_the_measured_deviation():
    assert MEASURED_ERFC <= 1e-10 and 100 * MEASURED_ERFC <= E.TOL_ERFC <= 100 * MEASURED_ERFC * 1.02


def _build(case, p):
    if case.kind == "vb":
        b = bnmf_vb_optimised(p.R, p.M, p.K, p.pri, verbose=False)
    elif case.kind == "vb_obs":
        b = bnmf_vb_observed(p.R, p.M, p.K, p.pri, verbose=False)
    elif case.kind == "tri":
        b = bnmtf_vb_optimised(p.R, p.M, p.K, p.L, p.pri, verbose=False)
    else:
        b = bnmtf_vb_observed(p.R, p.M, p.K, p.L, p.pri, verbose=False)
    E.seed_state(b, p.state)
    return b


def _assert_path(case, b):
    d = b.describe()
    for what in case.expect:
        assert what in d, (case.name, what, d)
    if case.nw is not None:
        assert tuple(int(x) for x in re.findall(r"sweep_nw=(\d+)", d)) == case.nw, (case.name, d)


def _ulp_apart(a, b):
    return abs(a - b) <= np.spacing(max(abs(a), abs(b)))


def _check_record(case, p, variant, b, it):
    """the statements of the module's docstring on the last iteration of the model's last call, iteration it (from 1) of the case"""
    where = "it %d" % it
    E.check_entries(case, p, variant, b, 0.0, where, it)
    terms = np.asarray(b.all_elbo_terms)[-1]
    ref, ref_abs = E.reference_sums(case, p, b)
    ratio, bad = E.compare_sums(terms[2:10], ref, ref_abs, "%s %s %s terms" % (case.name, variant, where))
    print("ELBO-TERMS %s %s %s: %s" % (case.name, variant, where, " ".join("%.2e" % r for r in ratio)))
    assert not bad, "\n".join(bad)
    if variant == "dead":
        assert ref[1] == -np.inf and ref[5] == -np.inf and np.isfinite(ref[[0, 2, 3, 4, 6, 7]]).all(), ref
    else:
        assert np.isfinite(ref).all(), ref
    assert np.isfinite(terms[0]) and _ulp_apart(terms[1], b.beta + 0.5 * terms[0]), (terms[0], terms[1])
    assert b.beta_s == terms[1]
    assert _ulp_apart(b.exptau, (b.alpha + b.size_Omega / 2.0) / b.beta_s), (b.exptau, b.beta_s)
    if variant == "dead":
        # (the tri-factorisation keeps no all_elbo: elbo() forms every factor sum again on the host from the returned state, so for
        # those models this line says nothing about a device fold -- their device side is held by the exact -inf of terms[3] and
        # terms[7] above alone)
        elbo = b.elbo() if case.tri else b.all_elbo[-1]
        assert elbo == -np.inf, elbo
    return ratio


@pytest.mark.parametrize("variant", E.VARIANTS)
@pytest.mark.parametrize("case", E.SINGLE_CASES, ids=E.ids(E.SINGLE_CASES))
def test_factor_sums_of_the_record(monkeypatch, case, variant):
    case.setenv(monkeypatch)
    p = case.problem(variant)
    b = _build(case, p)
    try:
        for it in range(E.ITERATIONS):
            if case.tri:
                b.run(1, orders=p.orders[it:it + 1])
            else:
                b.run(1)
            _assert_path(case, b)
            _check_record(case, p, variant, b, it + 1)
    finally:
        b.close()


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_factor_sums_of_models_run_together(monkeypatch, variant):
    """The list form: three models of different I (I mod 4 = 1, 2, 0) and K in one run_many call of two iterations, each model's
    last record from its own returned state.  The call's launch information says that the three shared their launches: a model
    that fell back to a run of its own fails the case."""
    E.MANY_CASES[0].setenv(monkeypatch)
    ps = [c.problem(variant) for c in E.MANY_CASES]
    ms = [_build(c, p) for c, p in zip(E.MANY_CASES, ps)]
    try:
        assert run_many(ms, 2) == [None] * len(ms)
        for c, p, b in zip(E.MANY_CASES, ps, ms):
            assert b._many_info[0] == len(ms), b._many_info
            assert np.asarray(b.all_elbo_terms).shape == (2, 10)
            _assert_path(c, b)
            _check_record(c, p, variant, b, 2)
    finally:
        for b in ms:
            b.close()
