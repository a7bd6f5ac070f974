"""bnmtf_amd.variational_predictive / bnmtf_predictive_moments (csrc/api_predictive_q.inc, kernel_predictive_q.hip; DESIGN.md
section 2.8a): the closed-form predictive mean and variance of a mean-field q at a list of entries against the NumPy fp64
restatement of tests/_predictive_q_cases.py, at the launch shapes where the kernels can go wrong, the bits that must not depend on
how the call is made, and the function on fitted models and on a fold_in result.

Exact.  On integer moments in {0, 1, 2, 3} every mean, variance and partial sum is an integer below 2^53 (test_predictive_q_cpu.py
asserts it), so every order of summation is exact and the device must give the int64 NumPy answer bit for bit: indexing, not
rounding.

Real-valued moments (exponential means, small variances).  Every term of the mean and of the variance is a product of non-negative
numbers, so the relative error of either side is at most (the number of roundings an addend goes through) 2^-53: K L + K + L + 8
bounds that depth for the device's fma chains and for the restatement's matrix products alike, and the two are compared within
relative 2 (K L + K + L + 8) 2^-53 with no absolute term.  The bound is derived, not measured; each case prints its largest ratio
of difference to bound."""
import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (Entries, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_vb_observed, bnmtf_vb_optimised, fold_in,
                       posterior_predictive, top_entries, variational_predictive)

import _predictive_q_cases as cases

pytestmark = pytest.mark.gpu

PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)
from_moments = variational_predictive.from_moments


def _call(shape, c, drop=(), rows=None, cols=None):
    """from_moments on a case: (mean, variance)"""
    P = from_moments(cases.as_factors(c["m"], drop), shape[:2], c["rows"] if rows is None else rows, c["cols"] if cols is None else cols)
    assert P.mean.dtype == np.float64 and P.variance.dtype == np.float64 and np.isnan(P.noise) and P.count == 0
    return P.mean, P.variance


def _within(name, got, want, K, L):
    """|got - want| <= bound(K, L) * want, entry by entry; prints the largest ratio"""
    assert (want >= 0).all() and want.sum() > 0
    diff, allowed = np.abs(got - want), cases.bound(K, L) * want
    ratio = np.where(allowed > 0, diff / np.where(allowed > 0, allowed, 1.0), np.where(diff > 0, np.inf, 0.0))
    print("%s: largest difference / bound %.3g" % (name, ratio.max()))
    assert ratio.max() <= 1.0, "%s: off by %.3g of its bound at entry %d" % (name, ratio.max(), int(ratio.argmax()))


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_integer_moments_give_the_int64_closed_form_bit_for_bit(shape):
    c = cases.case(shape, True)
    L = shape[3]
    for drop in ((), (0,), (2,)) + (((1,),) if L else ()):
        if drop:
            m = tuple(None if (q % 2 == 1 and q // 2 in drop) else a for q, a in enumerate(c["m"]))
            want_mean, want_var = cases.closed_form(c["rows"], c["cols"], *m)
        else:
            want_mean, want_var = c["mean"], c["var"]
        mean, var = _call(shape, c, drop)
        assert np.array_equal(mean, want_mean.astype(np.float64)) and np.array_equal(var, want_var.astype(np.float64)), drop
        assert not np.signbit(mean).any() and not np.signbit(var).any()
    assert c["var"].max() > 0 and c["mean"].max() > 0


@pytest.mark.parametrize("K", cases.RANKS)
def test_two_factors_are_the_tri_factorisation_with_an_identity_in_the_middle(K):
    shape = (cases.I, cases.J, K, 0, 'mixed')
    c = cases.case(shape, True)
    EA, VA, EB, VB = [a.astype(np.float64) for a in c["m"] if a is not None]
    two = from_moments(((EA, VA), (EB, VB)), shape[:2], c["rows"], c["cols"])
    tri = from_moments(((EA, VA), (np.eye(K), np.zeros((K, K))), (EB, VB)), shape[:2], c["rows"], c["cols"])
    fixed = from_moments(((EA, VA), (np.eye(K), None), (EB, VB)), shape[:2], c["rows"], c["cols"])
    for P in (tri, fixed):
        assert P.mean.tobytes() == two.mean.tobytes() and P.variance.tobytes() == two.variance.tobytes()


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_real_moments_lie_within_the_derived_bound_of_numpy(shape):
    c = cases.case(shape, False)
    K, L = shape[2], shape[3]
    mean, var = _call(shape, c)
    _within("%s mean" % cases.shape_id(shape), mean, c["mean"], K, L)
    _within("%s variance" % cases.shape_id(shape), var, c["var"], K, L)
    # each variance as None: a fixed factor -- the bits of a variance of zeros, and NumPy's number
    for which in (0, 2) + ((1,) if L else ()):
        m = list(c["m"])
        m[2 * which + 1] = np.zeros_like(m[2 * which + 1])
        zeros = from_moments(cases.as_factors(tuple(m)), shape[:2], c["rows"], c["cols"])
        none_mean, none_var = _call(shape, c, (which,))
        assert none_mean.tobytes() == mean.tobytes() == zeros.mean.tobytes() and none_var.tobytes() == zeros.variance.tobytes()
        _within("%s variance, factor %d fixed" % (cases.shape_id(shape), which), none_var, cases.closed_form(c["rows"], c["cols"], *m)[1], K, L)
        assert (none_var <= var).all()


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_the_bits_depend_on_the_entry_and_the_moments_alone(shape):
    c = cases.case(shape, False)
    rows, cols = c["rows"], c["cols"]
    base = _call(shape, c)
    assert not any(np.isnan(o).any() for o in base)
    again = _call(shape, c)
    for a, b in zip(again, base):
        assert a.tobytes() == b.tobytes()
    order = np.random.RandomState(11).permutation(len(rows))
    perm = _call(shape, c, rows=np.ascontiguousarray(rows[order]), cols=np.ascontiguousarray(cols[order]))
    for a, b in zip(perm, base):
        assert a.tobytes() == np.ascontiguousarray(b[order]).tobytes()
    for x, y in c["twins"]:
        assert rows[x] == rows[y] and cols[x] == cols[y]
        for b in base:
            assert b[x].tobytes() == b[y].tobytes()
    # a sub-list, and an entry on its own: what else is in the list does not matter
    pick = np.arange(0, len(rows), 3)
    sub = _call(shape, c, rows=np.ascontiguousarray(rows[pick]), cols=np.ascontiguousarray(cols[pick]))
    for a, b in zip(sub, base):
        assert a.tobytes() == np.ascontiguousarray(b[pick]).tobytes()
    x = c["twins"][0][0] if c["twins"] else 0
    alone = _call(shape, c, rows=rows[x:x + 1].copy(), cols=cols[x:x + 1].copy())
    for a, b in zip(alone, base):
        assert a[0].tobytes() == b[x].tobytes()


# ---------------------------------------------------------------- through the models
def _data(n_i, n_j, K, L=0, seed=3):
    rs = np.random.RandomState(seed)
    if L:
        R = rs.exponential(1.0, (n_i, K)) @ rs.exponential(1.0, (K, L)) @ rs.exponential(1.0, (n_j, L)).T
    else:
        R = rs.exponential(1.0, (n_i, K)) @ rs.exponential(1.0, (n_j, K)).T
    M = (rs.rand(n_i, n_j) >= 0.3).astype(float)
    M[rs.randint(n_i, size=n_j), np.arange(n_j)] = 1; M[np.arange(n_i), rs.randint(n_j, size=n_i)] = 1
    return R, M


def _model(kind):
    np.random.seed(4)
    import random
    random.seed(4)
    if kind == "bnmf vb":
        R, M = _data(20, 15, 3); m = bnmf_vb_optimised(R, M, 3, PRI2, verbose=False)
    elif kind == "bnmf vb observed":
        R, M = _data(20, 15, 3); m = bnmf_vb_observed(R, M, 3, PRI2, verbose=False)
    elif kind == "bnmf vb entries":
        R, M = _data(20, 15, 3); m = bnmf_vb_observed(Entries.from_dense(R, M), None, 3, PRI2, verbose=False)
    elif kind == "bnmtf vb":
        R, M = _data(20, 15, 3, 2); m = bnmtf_vb_optimised(R, M, 3, 2, PRI3, verbose=False)
    elif kind == "bnmtf vb observed":
        R, M = _data(20, 15, 3, 2); m = bnmtf_vb_observed(R, M, 3, 2, PRI3, verbose=False)
    else:
        R, M = _data(30, 25, 4); m = bnmf_vb_optimised(R, M, 70, PRI2, verbose=False)
    m.initialise()
    m.run(5)
    return m


def _snapshot(m):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in vars(m).items()
            if isinstance(v, (np.ndarray, int, float, str, tuple, list, type(None)))}


@pytest.mark.parametrize("kind", ["bnmf vb", "bnmf vb observed", "bnmf vb entries", "bnmtf vb", "bnmtf vb observed", "bnmf vb blocked K=70"])
def test_variational_predictive_of_a_fitted_model(kind):
    m = _model(kind)
    rs = np.random.RandomState(9)
    n = 2 * m.I * m.J                                   # any order, entries more than once, missing and observed ones alike
    rows, cols = rs.randint(m.I, size=n).astype(np.int32), rs.randint(m.J, size=n).astype(np.int32)
    E = Entries((m.I, m.J), rows, cols, np.zeros(n))
    before = _snapshot(m)
    P = variational_predictive(m, E)
    Q = variational_predictive(m, (rows, cols))
    assert _snapshot(m) == before                       # the model's own attributes: byte for byte what they were
    tri = len(m._FACTORS) == 3
    K, L = m.K, (m.L if tri else 0)
    exp = [np.asarray(getattr(m, "exp" + f), dtype=np.float64) for f in m._FACTORS]
    var = [np.asarray(getattr(m, "var" + f), dtype=np.float64) for f in m._FACTORS]
    left = exp[0] @ exp[1] if tri else exp[0]
    _within(kind + " mean", P.mean, np.einsum('ek,ek->e', left[rows], exp[-1][cols]), K, L)
    want = cases.closed_form(rows, cols, exp[0], var[0], exp[1] if tri else None, var[1] if tri else None, exp[-1], var[-1])
    _within(kind + " variance", P.variance, want[1], K, L)
    assert (P.variance > 0).all() and P.count == 0 and "closed form of q" in repr(P)
    assert m.alpha_s > 1 and P.noise == m.beta_s / (m.alpha_s - 1.0)
    assert np.array_equal(P.std(), np.sqrt(P.variance + P.noise)) and np.array_equal(P.std(noise=False), np.sqrt(P.variance))
    assert np.array_equal(P.rows, rows) and np.array_equal(P.cols, cols) and P.rows.dtype == np.int32
    for a, b in ((P.mean, Q.mean), (P.variance, Q.variance)):
        assert a.tobytes() == b.tobytes()
    assert P.noise == Q.noise
    # the neighbours in the same process: the refusal stays, the ranking runs
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        posterior_predictive(m, (rows, cols), 0, 1)
    assert "closed form of q" in str(e.value) and "out of scope here" in str(e.value)
    T = top_entries(m, 2)
    assert T.cols.shape[1] == 2
    t_rows, t_cols = T.entries()
    if len(t_rows):
        V = variational_predictive(m, (t_rows, t_cols))                 # how sure the model is about what it ranks first
        assert len(V) == len(t_rows) and (V.variance > 0).all()


def test_an_entries_built_model_gives_the_bits_of_its_dense_built_twin():
    a, b = _model("bnmf vb observed"), _model("bnmf vb entries")
    rs = np.random.RandomState(2)
    rows, cols = rs.randint(a.I, size=200), rs.randint(a.J, size=200)
    P, Q = variational_predictive(a, (rows, cols)), variational_predictive(b, (rows, cols))
    assert P.mean.tobytes() == Q.mean.tobytes() and P.variance.tobytes() == Q.variance.tobytes() and P.noise == Q.noise


def test_the_uncertainty_of_a_folded_in_rows_predictions():
    m = _model("bnmf vb")
    rs = np.random.RandomState(8)
    idx = np.concatenate([rs.choice(m.J, size=5, replace=False) for _ in range(4)])
    new = Entries((4, m.J), np.repeat(np.arange(4), 5), idx, rs.exponential(2.0, 20))
    F = fold_in(m, new, 30, seed=7)
    rows, cols = np.repeat(np.arange(4), m.J), np.tile(np.arange(m.J), 4)
    Q = from_moments(((F.mean, F.variance), (F.other, None)), (4, m.J), rows, cols, alpha_s=m.alpha_s, beta_s=m.beta_s)
    K = F.mean.shape[1]
    assert F.variance.max() > 0
    _within("fold-in mean", Q.mean, np.einsum('ek,ek->e', F.mean[rows], F.other[cols]), K, 0)
    _within("fold-in variance", Q.variance, np.einsum('ek,ek->e', F.variance[rows], F.other[cols] ** 2), K, 0)
    assert Q.noise == m.beta_s / (m.alpha_s - 1.0) and np.array_equal(Q.std(), np.sqrt(Q.variance + Q.noise))
    # new columns: the fixed factor stands first
    new_c = Entries((m.I, 2), np.array([0, 3, 5, 1, 2, 9]), np.repeat(np.arange(2), 3), rs.exponential(2.0, 6))
    G = fold_in(m, new_c, 30, axis=1, seed=7)
    rows, cols = np.tile(np.arange(m.I), 2), np.repeat(np.arange(2), m.I)
    Qc = from_moments(((G.other, None), (G.mean, G.variance)), (m.I, 2), rows, cols)
    _within("fold-in variance, columns", Qc.variance, np.einsum('ek,ek->e', G.other[rows] ** 2, G.variance[cols]), K, 0)
    assert np.isnan(Qc.noise) and np.isnan(Qc.std()).all() and not np.isnan(Qc.std(noise=False)).any()
