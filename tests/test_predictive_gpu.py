"""bnmtf_amd.posterior_predictive / bnmtf_predictive_samples (csrc/api_predictive.inc, kernel_predictive.hip; DESIGN.md section
2.8): the posterior predictive mean and variance at a list of entries against NumPy fp64 on the same fp32 samples, at the launch
shapes where the kernel can go wrong, the bits that must not depend on how the call is made, and the function on fitted models.

Reference.  p[t, e] in fp64 by einsum over the fp32 samples widened to fp64 (tri-factorisation: (A64[t] @ S64[t])[rows] * B64[t][cols]
summed), mean = p.mean(0), var = ((p - mean)^2).mean(0).  Samples are exponential draws: non-negative, nothing cancels inside a dot
product.

Tolerances (derived, not measured).  Products of two fp32 values are exact in fp64, so device and NumPy differ by summation order
only.  mean and p_first: rtol 1e-9, the project's tolerance for fp64 device sums (tests/test_heldout_gpu.py), atol 0.  variance:
rtol 1e-9 plus, per entry, atol = 16 W u pmax dmax + 4 (T + 4) u dmax^2 with u = 2^-53, W = K (K + L for the tri-factorisation),
pmax = max_t p_t, dmax = max_t |p_t - p_0|: the 2 W u relative disagreement of two p's carried through the differences, and the
rounding of the T-term sums.  Each case prints its largest ratio of difference to bound.  With T = 1 the variance and sum_d are
exactly 0.0."""
import ctypes as C

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import Entries, _lib, bnmf_gibbs_optimised, bnmtf_gibbs_optimised, posterior_predictive, predictive

pytestmark = pytest.mark.gpu

RTOL = 1e-9
U = 2.0 ** -53
I, J = 97, 83                     # the last block of 4 rows is partial
STORED, FIRST, STEP, T = 20, 2, 3, 5
TWO = (1, 3, 4, 5, 32, 64, 65, 255, 256)
TRI = ((1, 1), (3, 5), (5, 3), (32, 32), (33, 7), (64, 65), (256, 2), (2, 256))
CHUNKS = (0, 1, 2, 4, 5, 9)
PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)


def _entry_list(n_i, n_j, counts, seed):
    """Rows with counts[i % len(counts)] entries (columns drawn with replacement: a row may be longer than the matrix is wide),
    the far corner, three entries given twice at the end of the list before the shuffle; (rows, cols, positions of the twins)."""
    rs = np.random.RandomState(seed)
    per_row = np.array([counts[i % len(counts)] for i in range(n_i)])
    rows = np.repeat(np.arange(n_i), per_row)
    cols = rs.randint(n_j, size=len(rows))
    rows = np.concatenate([rows, [n_i - 1], rows[[0, 70, 200]]])
    cols = np.concatenate([cols, [n_j - 1], cols[[0, 70, 200]]])
    order = rs.permutation(len(rows))
    where = np.empty(len(rows), dtype=np.int64); where[order] = np.arange(len(rows))
    twins = [(where[a], where[len(rows) - 3 + q]) for q, a in enumerate((0, 70, 200))]
    return rows[order].astype(np.int32), cols[order].astype(np.int32), twins


def _samples(n_i, n_j, K, L, seed):
    rs = np.random.RandomState(seed)
    A = rs.exponential(1.0, (STORED, n_i, K)).astype(np.float32)
    S = rs.exponential(1.0, (STORED, K, L)).astype(np.float32) if L else None
    B = rs.exponential(1.0, (STORED, n_j, L if L else K)).astype(np.float32)
    return A, S, B


def _raw(shape, rows, cols, A, S, B, first, step, n_samples, chunk=0):
    """bnmtf_predictive_samples as it stands: (p_first, sum_d, sum_d2)"""
    n = len(rows)
    out = [np.full(n, np.nan) for _ in range(3)]
    _lib.check(_lib.lib().bnmtf_predictive_samples(0, shape[0], shape[1], A.shape[2], S.shape[2] if S is not None else 0, C.c_uint64(n),
                                                   _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(A), _lib.ptr(S), _lib.ptr(B),
                                                   C.c_uint64(first), C.c_uint64(step), n_samples, chunk, *[_lib.ptr(o) for o in out]))
    return out


def _reference(rows, cols, A, S, B, sel):
    """p [T][n] in fp64"""
    p = np.empty((len(sel), len(rows)))
    for q, t in enumerate(sel):
        a = A[t].astype(np.float64)
        if S is not None:
            a = a @ S[t].astype(np.float64)
        p[q] = np.einsum('ek,ek->e', a[rows], B[t].astype(np.float64)[cols])
    return p


def _finish(p_first, sum_d, sum_d2, n_samples):
    md = sum_d / n_samples
    return p_first + md, np.maximum(0.0, sum_d2 / n_samples - md * md)


def _compare(name, p, W, p_first, mean, var):
    """the asserts of one case; prints the largest ratio of difference to bound"""
    assert p.sum() > 0
    n_samples = len(p)
    ref_mean = p.mean(0)
    ref_var = ((p - ref_mean) ** 2).mean(0)
    pmax, dmax = p.max(0), np.abs(p - p[0]).max(0)
    atol = 16 * W * U * pmax * dmax + 4 * (n_samples + 4) * U * dmax ** 2
    r_first = np.abs(p_first - p[0]) / (RTOL * np.abs(p[0]))
    r_mean = np.abs(mean - ref_mean) / (RTOL * np.abs(ref_mean))
    bound = RTOL * ref_var + atol
    diff = np.abs(var - ref_var)
    r_var = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
    print("%s: largest difference / bound: p_first %.3g, mean %.3g, variance %.3g" % (name, r_first.max(), r_mean.max(), r_var.max()))
    assert r_first.max() <= 1.0 and r_mean.max() <= 1.0
    assert r_var.max() <= 1.0, "%s: variance off by %.3g of its bound at entry %d" % (name, r_var.max(), int(r_var.argmax()))


_CASES = {}


def _case(n_i, n_j, K, L):
    """list, samples and reference of a launch shape: made once, shared by the tests, never changed"""
    key = (n_i, n_j, K, L)
    if key not in _CASES:
        counts = (0, 1, 63, 64, 65, 129) if n_i == I else (0, 1, 3, 65)
        rows, cols, twins = _entry_list(n_i, n_j, counts, seed=K * 1000 + L)
        A, S, B = _samples(n_i, n_j, K, L, seed=K * 7 + L)
        sel = list(range(FIRST, FIRST + T * STEP, STEP))
        p = _reference(rows, cols, A, S, B, sel)
        for a in (rows, cols, A, S, B, p):
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = (rows, cols, twins, A, S, B, p)
    return _CASES[key]


SHAPES = [(I, J, K, 0) for K in TWO] + [(I, J, K, L) for K, L in TRI] + [(1100, 7, 3, 0)]


@pytest.mark.parametrize("n_i, n_j, K, L", SHAPES)
def test_the_c_call_matches_numpy_at_every_launch_shape(n_i, n_j, K, L):
    rows, cols, twins, A, S, B, p = _case(n_i, n_j, K, L)
    if n_i == I:
        per_row = np.bincount(rows, minlength=n_i)
        assert per_row[0] == 0 and {1, 63, 64, 65, 129} <= set(per_row.tolist()) and (rows == I - 1).any() and per_row.max() >= 129
    else:
        assert (n_i + 3) // 4 == 275
    p_first, sum_d, sum_d2 = _raw((n_i, n_j), rows, cols, A, S, B, FIRST, STEP, T)
    mean, var = _finish(p_first, sum_d, sum_d2, T)
    _compare("%d x %d K=%d L=%d" % (n_i, n_j, K, L), p, K + L, p_first, mean, var)
    # T = 1: the first sample alone
    one = _raw((n_i, n_j), rows, cols, A, S, B, FIRST, STEP, 1)
    assert one[0].tobytes() == p_first.tobytes()
    assert (one[1] == 0.0).all() and (one[2] == 0.0).all() and not np.signbit(one[1]).any()
    assert (_finish(*one, 1)[1] == 0.0).all()


@pytest.mark.parametrize("n_i, n_j, K, L", SHAPES)
def test_the_bits_depend_on_the_entry_and_the_samples_alone(n_i, n_j, K, L):
    rows, cols, twins, A, S, B, p = _case(n_i, n_j, K, L)
    shape = (n_i, n_j)
    base = _raw(shape, rows, cols, A, S, B, FIRST, STEP, T)
    assert not any(np.isnan(o).any() for o in base)
    again = _raw(shape, rows, cols, A, S, B, FIRST, STEP, T)
    for chunk in CHUNKS:
        got = again if chunk == 0 else _raw(shape, rows, cols, A, S, B, FIRST, STEP, T, chunk)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), "chunk_samples=%d" % chunk
    order = np.random.RandomState(11).permutation(len(rows))
    perm = _raw(shape, np.ascontiguousarray(rows[order]), np.ascontiguousarray(cols[order]), A, S, B, FIRST, STEP, T, 2)
    for a, b in zip(perm, base):
        assert a.tobytes() == np.ascontiguousarray(b[order]).tobytes()
    for x, y in twins:
        assert rows[x] == rows[y] and cols[x] == cols[y]
        for b in base:
            assert b[x].tobytes() == b[y].tobytes()
    # an entry on its own: what else is in the list does not matter
    x = twins[0][0]
    alone = _raw(shape, rows[x:x + 1].copy(), cols[x:x + 1].copy(), A, S, B, FIRST, STEP, T, 3)
    for a, b in zip(alone, base):
        assert a[0].tobytes() == b[x].tobytes()


def test_from_samples_finishes_the_c_calls_sums_and_takes_fp64_and_lists():
    rows, cols, twins, A, S, B, p = _case(I, J, 5, 3)
    sel = range(FIRST, FIRST + T * STEP, STEP)
    taus = np.random.RandomState(5).gamma(2.0, 1.0, STORED)
    P = predictive.from_samples((A, S, B), taus, (I, J), rows, cols, sel, chunk_samples=2)
    mean, var = _finish(*_raw((I, J), rows, cols, A, S, B, FIRST, STEP, T), T)
    assert P.mean.tobytes() == mean.tobytes() and P.variance.tobytes() == var.tobytes() and P.count == T
    assert P.noise == np.mean(1.0 / taus[list(sel)])
    assert np.array_equal(P.rows, rows) and np.array_equal(P.cols, cols) and P.rows.dtype == np.int32
    assert np.array_equal(P.std(), np.sqrt(var + P.noise)) and np.array_equal(P.std(noise=False), np.sqrt(var))
    # fp64 arrays and lists of arrays are cast to the samples' own precision: the same bits
    for factors in ([a.astype(np.float64) for a in (A, S, B)], [list(a) for a in (A, S, B)]):
        Q = predictive.from_samples(factors, list(taus), (I, J), rows.astype(np.int64), list(cols), sel)
        assert Q.mean.tobytes() == mean.tobytes() and Q.variance.tobytes() == var.tobytes() and Q.noise == P.noise
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        predictive.from_samples((A, S, B), taus, (I, J), rows, cols, [2, 3, 5])
    assert "arithmetic progression" in str(e.value)


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
    if kind == "bnmf dense":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False)
    elif kind == "bnmf observed":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmf entries":
        R, M = _data(20, 15, 3); m = bnmf_gibbs_optimised(Entries.from_dense(R, M), None, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmtf dense":
        R, M = _data(20, 15, 3, 2); m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False)
    elif kind == "bnmtf observed":
        R, M = _data(20, 15, 3, 2); m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False, layout='observed')
    else:
        R, M = _data(30, 25, 4); m = bnmf_gibbs_optimised(R, M, 70, PRI2, seed=1, verbose=False)
    m.initialise()
    m.run(8)
    return m


def _snapshot(m):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in vars(m).items()
            if isinstance(v, (np.ndarray, int, float, str, tuple, list, type(None)))}


@pytest.mark.parametrize("kind", ["bnmf dense", "bnmf observed", "bnmf entries", "bnmtf dense", "bnmtf observed", "bnmf blocked K=70"])
def test_posterior_predictive_of_a_fitted_model(kind):
    m = _model(kind)
    burn_in, thinning = 2, 2
    rs = np.random.RandomState(9)
    n = 2 * m.I * m.J                                   # any order, entries more than once, missing and observed ones alike
    rows, cols = rs.randint(m.I, size=n).astype(np.int32), rs.randint(m.J, size=n).astype(np.int32)
    E = Entries((m.I, m.J), rows, cols, np.zeros(n))
    before = _snapshot(m)
    P = posterior_predictive(m, E, burn_in, thinning)
    Q = posterior_predictive(m, (rows, cols), burn_in, thinning)
    assert _snapshot(m) == before                       # the model's own attributes: byte for byte what they were
    tri = isinstance(m, bnmtf_gibbs_optimised)
    stored = [np.asarray(getattr(m, "all_" + f)) for f in m._FACTORS]
    assert all(a.dtype == np.float32 and len(a) == 8 for a in stored)
    sel = list(range(burn_in, 8, thinning))
    p = _reference(rows, cols, stored[0], stored[1] if tri else None, stored[-1], sel)
    assert p.sum() > 0
    W = m.K + (m.L if tri else 0)
    _compare(kind, p, W, p[0], P.mean, P.variance)      # (the wrapper hands out no p_first: the mean and the variance carry the check)
    assert P.count == len(sel) and P.noise == np.mean(1.0 / np.asarray(m.all_tau)[sel])
    assert np.array_equal(P.rows, rows) and np.array_equal(P.cols, cols)
    for a, b in ((P.mean, Q.mean), (P.variance, Q.variance)):
        assert a.tobytes() == b.tobytes()
    assert P.noise == Q.noise and P.mean.dtype == np.float64 and P.variance.dtype == np.float64
    # the means of the predictions are the prediction of nothing else: a check against approx_expectation's selection rule
    one = posterior_predictive(m, (rows, cols), 7, 1)
    assert one.count == 1 and (one.variance == 0.0).all()
    assert np.allclose(one.mean, _reference(rows, cols, stored[0], stored[1] if tri else None, stored[-1], [7])[0], rtol=RTOL, atol=0)
