"""bnmtf_amd.top_entries / bnmtf_top_entries (csrc/api_top.inc, kernel_top.hip) on the device: the n best
candidates per row against the NumPy restatement of tests/_top_entries_cases.py.

The kernel's constants: kTopStep = 64 columns per wave step (a lane each), kTopRows = 4 (row, segment) pairs per block, two list
slots per lane (n <= 128: slot 64 is the first of the second), 16-byte loads of B's rows with one 8-byte load at the end of an odd
width; segment s of a row is the steps [s ceil(steps / split), ...) of its ceil(J / 64).

Exact cases (compared with ==).  Integer-valued factors: every product and partial sum is an integer below 2^53, so the device's
fma chain and NumPy's product give the same bits in any order, and since the order is total the answer is unique: cols, scores and
counts are compared byte for byte.  B's rows repeat, so ties are plentiful and the tie rule decides; each case asserts a tie
between its n-th and (n + 1)-th candidate in some row (for J <= n, where no row has an (n + 1)-th: between two returned slots).

Generic floats.  Exponential factors: device and NumPy differ by summation order only, so a near-tie may flip and the checks are
those a flip leaves true, with RTOL = 1e-9, the project's tolerance for fp64 device sums of non-negative data
(tests/test_heldout_gpu.py)."""
import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, Entries, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_observed, nmtf_icm,
                       posterior_predictive, top_entries)
import _top_entries_cases as cases

pytestmark = pytest.mark.gpu

from_factors = top_entries.from_factors
RTOL = 1e-9
PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)

_CASES = {}


def _case(number, J, n, K, L):
    """factors, exclusion list and the restatement's answers of an exact case: made once, shared, never changed"""
    key = (number, J, n, K, L)
    if key not in _CASES:
        factors = cases.int_factors(J, K, L, number)
        ex = cases.exclusion(J, n, number)
        P = cases.dense_scores(factors)
        want = {lg: cases.restate(factors, n, None, ex, lg, scores=P) for lg in (True, False)}
        for a in list(factors) + list(ex) + [P] + [x for w in want.values() for x in w]:
            a.setflags(write=False)
        _CASES[key] = (factors, ex, P, want)
    return _CASES[key]


def _same(got, want, what=""):
    cols, scores, counts = want
    assert got.cols.dtype == np.int32 and got.scores.dtype == np.float64 and got.counts.dtype == np.int32
    assert got.counts.tobytes() == counts.tobytes(), what
    assert got.cols.tobytes() == cols.tobytes(), what
    assert (got.scores == scores)[cols >= 0].all() and np.isnan(got.scores[cols < 0]).all(), what       # (-0.0 == 0.0; nan in the padding)


EXACT = [(number,) + c for number, c in enumerate(cases.EXACT)]
SPLIT = [(len(cases.EXACT) + number,) + c for number, c in enumerate(cases.SPLIT_CASES)]


@pytest.mark.parametrize("number, J, n, K, L", EXACT + SPLIT)
def test_exact_cases_equal_the_restatement(number, J, n, K, L):
    factors, ex, P, want = _case(number, J, n, K, L)
    for largest in (True, False):
        tie = cases.has_boundary_tie(factors, n, ex, largest)
        assert tie or (tie is None and J == 1)
        got = from_factors(factors, n, exclude=ex, largest=largest)
        _same(got, want[largest], "largest=%s" % largest)
        assert np.array_equal(got.rows, np.arange(cases.ROWS)) and got.rows.dtype == np.int32
        # the exclusion rows: nothing, everything, all but one, n left, n - 1 left
        assert got.counts[0] == min(n, J) and got.counts[1] == 0 and (got.cols[1] == -1).all() and np.isnan(got.scores[1]).all()
        assert got.counts[2] == 1 and got.cols[2, 0] == J // 2 and got.counts[4] == min(n, J) and got.counts[5] == min(n - 1, J)
        if J >= n:
            assert got.cols[5, n - 1] == -1 and (got.cols[5, :n - 1] >= 0).all()
        assert not set(zip(np.repeat(got.rows, n)[got.cols.ravel() >= 0].tolist(), got.cols[got.cols >= 0].tolist())) & set(zip(ex[0].tolist(), ex[1].tolist()))
    # an Entries as the exclusion, and no exclusion at all
    E = Entries((cases.ROWS, J), ex[0], ex[1], np.zeros(len(ex[0])))
    _same(from_factors(factors, n, exclude=E), want[True])
    _same(from_factors(factors, n), cases.restate(factors, n, scores=P))
    if (P != P[:, :1]).any() and J > 1:
        assert from_factors(factors, n).cols.tobytes() != from_factors(factors, n, largest=False).cols.tobytes()


@pytest.mark.parametrize("number, J, n, K, L", [EXACT[1], EXACT[4], EXACT[9], SPLIT[1]])
def test_rows_in_any_order_give_the_bits_of_the_all_rows_call(number, J, n, K, L):
    factors, ex, P, want = _case(number, J, n, K, L)
    sel = [7, 0, 3]
    for largest in (True, False):
        got = from_factors(factors, n, rows=sel, exclude=ex, largest=largest)
        assert got.rows.tolist() == sel
        _same(got, tuple(w[sel] for w in want[largest]))
        _same(got, cases.restate(factors, n, sel, ex, largest, scores=P))
    one = from_factors(factors, n, rows=np.array([8], dtype=np.int64), exclude=ex)
    _same(one, tuple(w[[8]] for w in want[True]))


@pytest.mark.parametrize("number, J, n, K, L", SPLIT + [EXACT[4], EXACT[10]])
def test_every_split_gives_the_same_bytes(number, J, n, K, L):
    """split 1, 2, 3, 7 and 12: with J = 520 nine column steps, cut 5 + 4, 3 + 3 + 3, 2 + 2 + 2 + 2 + 1 + 0 + 0 and 1 x 9 + 0 x 3 --
    empty segments included; with J = 200 / 65 four steps / two, so 7 and 12 are more than there are"""
    factors, ex, P, want = _case(number, J, n, K, L)
    assert max(cases.SPLITS) > (J + cases.STEP - 1) // cases.STEP
    for largest in (True, False):
        base = from_factors(factors, n, exclude=ex, largest=largest, split=1)
        _same(base, want[largest])
        for split in cases.SPLITS + (0, 1):
            got = from_factors(factors, n, exclude=ex, largest=largest, split=split)
            for a, b in ((got.cols, base.cols), (got.scores, base.scores), (got.counts, base.counts)):
                assert a.tobytes() == b.tobytes(), "split=%d" % split
        few = from_factors(factors, n, rows=[5, 2], exclude=ex, largest=largest, split=3)
        assert few.cols.tobytes() == base.cols[[5, 2]].tobytes() and few.scores.tobytes() == base.scores[[5, 2]].tobytes()


def test_minus_zero_ties_with_zero_and_negative_scores_order():
    A = np.array([[1.0, 0.0], [-1.0, 0.0]])
    B = np.array([[0.0, 3.0], [-0.0, 1.0], [2.0, 0.0], [0.0, 0.0], [-2.0, 5.0]])
    for largest in (True, False):
        got = from_factors((A, B), 5, largest=largest)
        _same(got, cases.restate((A, B), 5, largest=largest))
    assert from_factors((A, B), 5).cols.tolist() == [[2, 0, 1, 3, 4], [4, 0, 1, 3, 2]]


# ---------------------------------------------------------------- generic floats
@pytest.mark.parametrize("K, L", [(5, 0), (32, 32)])
@pytest.mark.parametrize("largest", [True, False])
def test_generic_floats_agree_with_numpy_where_a_near_tie_cannot_matter(K, L, largest):
    factors, M = cases.float_factors(K, L)
    I, J = M.shape
    ex = np.nonzero(M)
    P = cases.dense_scores(factors)
    n = 10
    got = from_factors(factors, n, exclude=(ex[0].astype(np.int32), ex[1].astype(np.int32)), largest=largest)
    assert (got.counts == np.minimum(n, J - M.sum(axis=1))).all() and (got.counts == n).all()
    rows = np.repeat(np.arange(I), n).reshape(I, n)
    ref = P[rows, got.cols]
    worst = np.abs(got.scores - ref).max() / np.abs(ref).max()
    print("K=%d L=%d largest=%s: largest |device - numpy| / |numpy| %.3g" % (K, L, largest, (np.abs(got.scores - ref) / np.abs(ref)).max()))
    assert np.allclose(got.scores, ref, rtol=RTOL, atol=0), worst
    sign = 1.0 if largest else -1.0
    assert (sign * np.diff(got.scores, axis=1) <= 0).all()                        # best first
    assert not M[rows, got.cols].any()                                             # no returned column is excluded
    assert all(len(set(r)) == n for r in got.cols.tolist())
    rest = np.where(M != 0, np.nan, P)
    rest[rows, got.cols] = np.nan
    edge = np.nanmax(rest, axis=1) if largest else np.nanmin(rest, axis=1)         # the best candidate that was not returned
    if largest:
        assert (got.scores[:, -1] >= edge * (1 - RTOL)).all()
    else:
        assert (got.scores[:, -1] <= edge * (1 + RTOL)).all()


# ---------------------------------------------------------------- through the classes
def _data(n_i, n_j, K, L=0, seed=3):
    rs = np.random.RandomState(seed)
    if L:
        R = rs.exponential(1.0, (n_i, K)) @ rs.exponential(1.0, (K, L)) @ rs.exponential(1.0, (n_j, L)).T
    else:
        R = rs.exponential(1.0, (n_i, K)) @ rs.exponential(1.0, (n_j, K)).T
    M = (rs.rand(n_i, n_j) >= 0.3).astype(float)
    M[rs.randint(n_i, size=n_j), np.arange(n_j)] = 1; M[np.arange(n_i), rs.randint(n_j, size=n_i)] = 1
    return R, M


KINDS = ["bnmf dense", "bnmf observed", "bnmf entries", "bnmtf gibbs", "bnmf vb", "bnmtf vb observed", "nmtf icm", "NMF observed", "bnmf blocked K=70"]


def _model(kind):
    """(the fitted model, its training mask, the keyword arguments of its top_entries, the factors its predict() multiplies)"""
    np.random.seed(4)
    gibbs = {}
    if kind == "bnmf dense":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False)
    elif kind == "bnmf observed":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmf entries":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(Entries.from_dense(R, M), None, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmtf gibbs":
        R, M = _data(20, 15, 3, 2); m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False)
    elif kind == "bnmf vb":
        R, M = _data(20, 15, 3); m = bnmf_vb_optimised(R, M, 3, PRI2, verbose=False)
    elif kind == "bnmtf vb observed":
        R, M = _data(20, 15, 3, 2); m = bnmtf_vb_observed(R, M, 3, 2, PRI3, verbose=False)
    elif kind == "nmtf icm":
        R, M = _data(20, 15, 3, 2); m = nmtf_icm(R, M, 3, 2, PRI3, seed=1, verbose=False)
    elif kind == "NMF observed":
        R, M = _data(20, 15, 3); m = NMF(R, M, 3, verbose=False, layout='observed')
    else:
        R, M = _data(30, 25, 4); m = bnmf_gibbs_optimised(R, M, 70, PRI2, seed=1, verbose=False)
    m.initialise()
    m.run(6)
    if isinstance(m, (bnmf_gibbs_optimised, bnmtf_gibbs_optimised)) and not isinstance(m, nmtf_icm):
        gibbs = dict(burn_in=2, thinning=2)
        factors = list(m.approx_expectation(2, 2)[:-1])
    elif kind == "bnmf vb":
        factors = [m.expU, m.expV]
    elif kind == "bnmtf vb observed":
        factors = [m.expF, m.expS, m.expG]
    elif kind == "nmtf icm":
        factors = [m.F, m.S, m.G]
    else:
        factors = [m.U, m.V]
    return m, M, gibbs, factors


def _snapshot(m):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in vars(m).items()
            if isinstance(v, (np.ndarray, int, float, str, tuple, list, type(None)))}


@pytest.mark.parametrize("kind", KINDS)
def test_top_entries_of_a_fitted_model(kind):
    m, M, kw, factors = _model(kind)
    factors = [np.array(f, dtype=np.float64) for f in factors]
    before = _snapshot(m)
    assert any(isinstance(v, np.ndarray) for v in vars(m).values())
    T = top_entries(m, 5, **kw)
    L5 = top_entries(m, 5, largest=False, rows=[3, 1], **kw)
    C1 = top_entries(m, 4, axis=1, **kw)
    assert _snapshot(m) == before                       # the model's own attributes: byte for byte what they were
    ex = tuple(a.astype(np.int32) for a in np.nonzero(M))
    want = from_factors(factors, 5, exclude=ex)
    for a, b in ((T.cols, want.cols), (T.scores, want.scores), (T.counts, want.counts)):
        assert a.tobytes() == b.tobytes()
    rows, cols = T.entries()
    assert len(rows) == T.counts.sum() == len(T) and not M[rows, cols].any()               # no training entry is returned
    assert (T.counts == np.minimum(5, M.shape[1] - M.sum(axis=1))).all()
    low = from_factors(factors, 5, rows=[3, 1], exclude=ex, largest=False)
    assert L5.cols.tobytes() == low.cols.tobytes() and L5.scores.tobytes() == low.scores.tobytes() and L5.rows.tolist() == [3, 1]
    # axis=1 is axis=0 of the transposed problem
    swapped = [factors[-1]] + ([np.ascontiguousarray(factors[1].T)] if len(factors) == 3 else []) + [factors[0]]
    col = from_factors(swapped, 4, exclude=(ex[1], ex[0]))
    assert C1.cols.tobytes() == col.cols.tobytes() and C1.scores.tobytes() == col.scores.tobytes() and len(C1.rows) == M.shape[1]
    r1, c1 = C1.entries()
    assert not M[r1, c1].any() and (c1 == np.repeat(np.arange(M.shape[1]), 4)[C1.cols.ravel() >= 0]).all()
    # other exclusions: none, and training plus a validation list as an Entries
    assert top_entries(m, 5, exclude=None, **kw).cols.tobytes() == from_factors(factors, 5).cols.tobytes()
    more = (np.concatenate([ex[0], rows[:7]]), np.concatenate([ex[1], cols[:7]]))
    E = Entries(M.shape, more[0], more[1], np.zeros(len(more[0])))
    assert top_entries(m, 5, exclude=E, **kw).cols.tobytes() == from_factors(factors, 5, exclude=more).cols.tobytes()


def test_the_entries_go_straight_into_posterior_predictive():
    m, M, kw, factors = _model("bnmf entries")
    T = top_entries(m, 5, **kw)
    P = posterior_predictive(m, T.entries(), kw["burn_in"], kw["thinning"])
    assert len(P) == len(P.mean) == len(P.variance) == int(T.counts.sum()) == len(T)
    assert np.array_equal(P.rows, T.entries()[0]) and np.array_equal(P.cols, T.entries()[1])
    assert np.isfinite(P.mean).all() and (P.variance >= 0).all()
    E = Entries(M.shape, *T.entries(), np.zeros(len(T)))
    assert len(E) == len(T)
