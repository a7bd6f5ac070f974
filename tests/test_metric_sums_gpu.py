"""The fp64 metric sums (csrc/kernel_misc.hip: metric_kernel, metric_reduce_kernel) checked bit for bit at every launch shape.

Through the entry points the model classes use -- bnmtf_metric_sums, bnmtf_metric_sums_wide (a model in column blocks),
bnmtf_beta_s, bnmf_vb_exp_square_diff, bnmf_vb_esd_terms -- on integer data where every product and every sum is an integer
below 2^53 (tests/_metric_cases.py; the CPU side, test_metric_cases_cpu.py, bounds the sums, shows that each single fault of a
model of the tiling would move a checked sum, and that the cases cover the launch edges).  The device must return the integer
reference exactly, twice the same, and predict() must be metrics_from_sums of that reference.  One real-valued test rides
along: the cancelling SSE of a near-exact fit within a derived bound."""
import numpy as np
import pytest

from bnmtf_amd import _lib, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised
from bnmtf_amd._base import metrics_from_sums
from _metric_cases import as_doubles, by_family, problem, real_case, reference

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI_TRI = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)


def _same(got, want, what):
    assert np.array_equal(got, want), "%s: device %r, reference %r" % (what, list(got), list(want))


def _same_metrics(got, want, what):
    keys = ("MSE", "R^2", "Rp")
    assert np.array_equal([got[k] for k in keys], [want[k] for k in keys], equal_nan=True), "%s: predict %r, from the reference %r" % (what, got, want)


def _check_masks(case, p, sums, predict):
    """sums(M_pred) -> the six sums; predict(M_pred) -> the metrics.  Every mask of the case: exact, the same bits twice,
    predict() = metrics_from_sums(reference) (an empty mask has no metrics: the reference divides by n, too)."""
    for name in case.masks:
        want = as_doubles(reference(p, name)[:6])
        got = sums(p.argument(name))
        print("%s %s: %r" % (case.id, name, got.tolist()))
        _same(got, want, "%s %s" % (case.id, name))
        _same(sums(p.argument(name)), got, "%s %s, second call" % (case.id, name))
        if name != "empty":
            _same_metrics(predict(p.argument(name)), metrics_from_sums(want), "%s %s" % (case.id, name))


def _gibbs_predict(model, names, arrays):
    """predict(M_pred, 0, 1) over a single stored sample = the given factors"""
    for n, a in zip(names, arrays):
        setattr(model, n, [a])
    model.all_tau = [1.0]
    return lambda Mp: model.predict(Mp, 0, 1)


TWO = by_family("plain", "wide")


@pytest.mark.parametrize("case", TWO, ids=[c.id for c in TWO])
def test_two_factor_sums_are_exact(case):
    """bnmtf_metric_sums on a handle of K = width (widths 1 .. 64), bnmtf_metric_sums_wide for a model in column blocks (65 .. 256)"""
    p = problem(case)
    model = bnmf_gibbs_optimised(p.R, p.M, case.K, PRI, verbose=False, seed=1)
    try:
        assert (model._blocks is not None) == (case.family == "wide")
        _check_masks(case, p, lambda Mp: model._metric_sums(Mp, p.A, None, p.B), _gibbs_predict(model, ("all_U", "all_V"), (p.A, p.B)))
    finally:
        model.close()


TRI = by_family("tri")


@pytest.mark.parametrize("case", TRI, ids=[c.id for c in TRI])
def test_tri_factor_sums_are_exact(case):
    p = problem(case)
    model = bnmtf_gibbs_optimised(p.R, p.M, case.K, case.L, PRI_TRI, verbose=False, seed=1)
    try:
        _check_masks(case, p, lambda Mp: model._metric_sums(Mp, p.A, p.S, p.B),
                     _gibbs_predict(model, ("all_F", "all_S", "all_G"), (p.A, p.S, p.B)))
    finally:
        model.close()


STATE = by_family("state", "state_tri")


@pytest.mark.parametrize("small", (False, True), ids=("multi-launch", "one-launch"))
@pytest.mark.parametrize("case", STATE, ids=[c.id for c in STATE])
def test_sums_of_the_state_the_handle_holds(case, small, monkeypatch):
    """A = None: the factors come from the handle -- its multi-launch buffers, or the arena of a one-launch model -- and give
    the sums of the call that hands the same factors over; beta_s() = beta + SSE / 2 exactly"""
    if not small:
        monkeypatch.setenv("BNMTF_SMALL", "0")          # (read when the handle is built)
    p = problem(case)
    tri = case.family == "state_tri"
    if tri:
        model = bnmtf_gibbs_optimised(p.R, p.M, case.K, case.L, PRI_TRI, verbose=False, seed=1)
        model.F, model.S, model.G = p.A.copy(), p.S.copy(), p.B.copy()
    else:
        model = bnmf_gibbs_optimised(p.R, p.M, case.K, PRI, verbose=False, seed=1)
        model.U, model.V = p.A.copy(), p.B.copy()
    model.tau = 1.0
    try:
        model._push()
        assert ("small[" in model.describe()) == small, model.describe()
        for name in case.masks:
            want = as_doubles(reference(p, name)[:6])
            held = model._metric_sums(p.argument(name), None, None, None)
            _same(held, want, "%s %s, held state" % (case.id, name))
            _same(model._metric_sums(p.argument(name), p.A, p.S, p.B), held, "%s %s, handed over" % (case.id, name))
        s = reference(p, "train")
        assert model.beta_s() == 1.0 + 0.5 * (s[2] - 2 * s[5] + s[4])
        _same_metrics(model.predict_while_running(), metrics_from_sums(as_doubles(s[:6])), case.id)
    finally:
        model.close()


VB = by_family("vb")


@pytest.mark.parametrize("case", VB, ids=[c.id for c in VB])
def test_vb_expected_square_difference_is_exact(case):
    """bnmf_vb_set_state, then exp_square_diff() = sum (R - P)^2 + sum_k [(var + exp^2)(var + exp^2) - exp^2 exp^2] over the
    training mask, its two terms (bnmf_vb_esd_terms: what a model in column blocks adds up), and the six sums"""
    p = problem(case)
    model = bnmf_vb_optimised(p.R, p.M, case.K, PRI, verbose=False)
    try:
        model.expU, model.varU, model.expV, model.varV = p.A.copy(), p.varA.copy(), p.B.copy(), p.varB.copy()
        model.exptau = 1.0
        want = reference(p, "train")
        esd = model.exp_square_diff()
        terms = np.zeros(2)
        _lib.check(_lib.lib().bnmf_vb_esd_terms(model._handle(), _lib.ptr(terms)))
        print("%s: esd %r, terms %r" % (case.id, esd, terms.tolist()))
        _same(terms, as_doubles(want[6:8]), "%s esd_terms" % case.id)
        assert esd == float(want[6] + want[7]), (esd, want[6:8])
        assert model.exp_square_diff() == esd
        again = np.zeros(2)
        _lib.check(_lib.lib().bnmf_vb_esd_terms(model._handle(), _lib.ptr(again)))
        _same(again, terms, "%s esd_terms, second call" % case.id)
        six = as_doubles(want[:6])
        _same(model._metric_sums(None, None, None, None), six, "%s, held state" % case.id)
        _same(model._metric_sums(None, model.expU, None, model.expV), six, "%s, handed over" % case.id)
        _same_metrics(model.predict(None), metrics_from_sums(six), case.id)
        model.update_tau()
        assert model.beta_s == 1.0 + 0.5 * float(want[6] + want[7])
    finally:
        model.close()


def test_cancelling_sse_of_a_near_exact_fit_is_within_the_derived_bound():
    """Real-valued data (tests/_metric_cases.py: RealCase): the device's sum R^2 - 2 sum R P + sum P^2 against the residual
    form summed with math.fsum.  Bound 2 (N + 2 K + 2) 2^-53 (sum R^2 + sum P^2 + 2 sum |R P|); with SEED's data N = 9028,
    reference SSE 1.3223, bound 5.89e-4."""
    rc = real_case()
    model = bnmf_gibbs_optimised(rc.R, rc.M, rc.K, PRI, verbose=False, seed=1)
    try:
        s = model._metric_sums(rc.Mp, rc.U, None, rc.V)
        sse = s[2] - 2.0 * s[5] + s[4]
        print("device SSE %.12e, reference %.12e, difference %.3e, bound %.3e" % (sse, rc.sse, abs(sse - rc.sse), rc.bound))
        assert s[0] == rc.N
        assert rc.bound < 1e-3 * rc.sse
        assert abs(sse - rc.sse) <= rc.bound
    finally:
        model.close()
