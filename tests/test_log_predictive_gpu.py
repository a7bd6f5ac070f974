"""bnmtf_amd.log_predictive / bnmtf_log_predictive_samples (csrc/api_log_predictive.inc, kernel_log_predictive.hip; DESIGN.md
section 2.8b): the five per-entry numbers bit for bit against integer arithmetic where that is possible, the log-sum-exp against a
two-pass restatement in np.longdouble in every regime of the running maximum, everything against NumPy fp64 on real-valued samples
at the launch shapes where the kernel can go wrong (tests/_log_predictive_cases.py: test_predictive_gpu.py's), the bits that must
not depend on how the call is made, and the function on fitted models.

Tolerances (derived, not measured; u = 2^-53; every test prints its largest ratio of difference to bound).
  * exact cases: l_first, sum_d, sum_d2 and l_max have no tolerance; the test asserts that every intermediate fits 53 bits.
  * the log-sum-exp (sum_exp relative, lpd absolute): (2 T + 16) u max(1, |lpd_e|) -- T terms in (0, 1] whose largest is 1, exp
    and log within 2 ulp, one rounding per addition and per rescaling.  The l_t that go into the restatement are the device's own
    (T calls with one sample each: an entry's l_t depends on the entry and the sample alone), so this bound is the recurrence's.
  * against NumPy on real-valued samples: device and NumPy differ in the summation order of p, so l_t differs by at most
    dl_e = max_t h_t (2 |d_t| D + D^2), D = 2 W' u max_t p_t, W' = K (K + L for the tri-factorisation); mean and lpd: dl_e plus the
    log-sum-exp bound.  variance (divisor T - 1), as test_predictive_gpu.py carries 2 W u pmax through its differences: rtol 1e-9
    plus T / (T - 1) (8 el_e smax + 4 (T + 4) u smax^2) with smax = max_t |l_t - l_0| and el_e = dl_e + 4 u max_t (|c_t| + h_t d_t^2),
    the second term the two roundings of l_t itself on either side.
The device's exp is assumed within 2 ulp, which cannot be verified without a device; worst ratios observed are in DESIGN.md."""
from fractions import Fraction

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import Entries, bnmf_gibbs_optimised, bnmtf_gibbs_optimised, log_predictive
import _log_predictive_cases as cases
from _log_predictive_cases import CHUNKS, FIRST, I, J, SEL, STEP, STORED, T, U

pytestmark = pytest.mark.gpu

RTOL = 1e-9
PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)


def _same(a, b, what=""):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), what


def _dyadic(a, q):
    """the integers a over the power of two q as doubles, which they are exactly"""
    out = np.array([float(Fraction(int(v), q)) for v in a])
    assert all(Fraction(w) == Fraction(int(v), q) for v, w in zip(a, out))
    return out


def _device_l(shape, rows, cols, values, A, S, B, sel, c, h):
    """l [T][n] as the device forms it: one call per sample, whose l_first it is"""
    return np.array([cases.raw(shape, rows, cols, values, A, S, B, t, 1, 1, c[q:q + 1], h[q:q + 1])[0] for q, t in enumerate(sel)])


def _check_lse(name, l, l_max, sum_exp, n_samples):
    """sum_exp and the lpd finished from it against the two-pass restatement on the same l; prints the worst ratio to the bound"""
    ref_sum, ref_lpd = cases.lse(l)
    assert l_max.tobytes() == l.max(0).tobytes()
    lpd = l_max + np.log(sum_exp) - np.log(float(n_samples))
    assert np.isfinite(sum_exp).all() and np.isfinite(lpd).all() and (sum_exp >= 1.0).all() and (sum_exp <= n_samples).all()
    bound = cases.lse_bound(n_samples, ref_lpd.astype(np.float64))
    r_sum = np.abs(sum_exp - ref_sum).astype(np.float64) / ((2 * n_samples + 16) * U * ref_sum.astype(np.float64))
    r_lpd = np.abs(lpd - ref_lpd).astype(np.float64) / bound
    print("%s: largest difference / bound: sum_exp %.3g, lpd %.3g" % (name, r_sum.max(), r_lpd.max()))
    assert r_sum.max() <= 1.0, "%s: sum_exp off by %.3g of its bound at entry %d" % (name, r_sum.max(), int(r_sum.argmax()))
    assert r_lpd.max() <= 1.0, "%s: lpd off by %.3g of its bound at entry %d" % (name, r_lpd.max(), int(r_lpd.argmax()))


# ---------------------------------------------------------------- 1, 2: exact moments, and the log-sum-exp on the same cases
@pytest.mark.parametrize("K, L", cases.EXACT)
def test_the_moments_are_the_integer_answer_bit_for_bit(K, L):
    rows, cols, twins, values, A, S, B, p, l8 = cases.exact_case(K, L)
    per_row = np.bincount(rows, minlength=I)
    assert per_row[0] == 0 and {1, 63, 64, 65, 129} <= set(per_row.tolist()) and (rows == I - 1).any()
    # in integer arithmetic: every intermediate of the device's chain is an integer multiple of a power of two below 2^53
    d = values.astype(np.int64)[None, :] - p
    d8 = l8 - l8[0]                                                         # (l_t - l_first) * 8
    s8 = np.cumsum(d8, axis=0)                                              # the running sum_d * 8
    s64 = np.cumsum(d8 * d8, axis=0)                                        # the running sum_d2 * 64
    widest = max(int(np.abs(a).max()) for a in (p, d, l8, d8, s8, s64, d8 * d8))
    print("K=%d L=%d: widest intermediate %d bits (sum of squares %d bits)" % (K, L, widest.bit_length(), int(s64.max()).bit_length()))
    assert widest < 2 ** 53
    want = [_dyadic(a, q) for a, q in ((l8[0], 8), (s8[-1], 8), (s64[-1], 64), (l8.max(0), 8))]
    got = cases.raw((I, J), rows, cols, values, A, S, B, FIRST, STEP, T, cases.C_EXACT, cases.H_EXACT)
    for name, g, w in zip(("l_first", "sum_d", "sum_d2", "l_max"), got, want):
        assert not np.isnan(g).any() and len(g) == len(rows)                # (no entry is left out)
        assert g.tobytes() == w.tobytes(), "%s differs at %d entries, first %d" % (name, (g != w).sum(), int(np.flatnonzero(g != w)[0]))
    # item 2 on the same case: the l_t are exact, so the restatement needs no device call
    l = np.array([_dyadic(row, 8) for row in l8])
    _check_lse("exact K=%d L=%d" % (K, L), l, got[3], got[4], T)


# ---------------------------------------------------------------- 3: the regimes of the running maximum
def _patterns(n_samples):
    """l [T][patterns] <= 0: one column per regime"""
    t = np.arange(n_samples, dtype=np.float64)
    base = -(1.0 + 0.37 * ((t * 7) % 5))                                     # a spread of a few nats
    cols = {}
    for name, at in (("max first", 0), ("max last", n_samples - 1), ("max middle", n_samples // 2)):
        x = base.copy(); x[at] = -0.125
        cols[name] = x
    cols["ascending"] = -3.0 * (n_samples - t)                              # every step rescales
    cols["descending"] = -3.0 * (t + 1.0)
    cols["all equal"] = np.full(n_samples, -2.5)
    x = base.copy(); x[n_samples // 3] = -1e6                               # its exp underflows to 0
    cols["one 1e6 below"] = x
    x = base.copy(); x[0] = -1e3                                            # a shift by the first sample would overflow
    cols["first 1e3 below"] = x
    return list(cols), np.array(list(cols.values())).T


@pytest.mark.parametrize("n_samples", [5, 40])
def test_the_running_maximum_in_every_regime(n_samples):
    """K = 1, A = 1, r = 0, h = 1, c = 0: l_t = -(b_t[j]^2), one fp64 rounding of the fp32 b's square, which NumPy restates to the
    bit; column j carries pattern j, every row of the matrix reads it."""
    names, want = _patterns(n_samples)
    n_j, n_i = len(names), 5
    b = np.sqrt(-want).astype(np.float32)                                   # [T][J]
    A = np.ones((n_samples, n_i, 1), dtype=np.float32)
    B = np.ascontiguousarray(b[:, :, None])
    rows = np.repeat(np.arange(n_i), n_j).astype(np.int32); cols = np.tile(np.arange(n_j), n_i).astype(np.int32)
    b64 = b.astype(np.float64)
    l = -(b64 * b64)[:, cols]
    assert np.abs(l - want[:, cols]).max() <= 1e-6 * np.abs(want).max()
    c, h = np.zeros(n_samples), np.ones(n_samples)
    base = cases.raw((n_i, n_j), rows, cols, np.zeros(len(rows)), A, None, B, 0, 1, n_samples, c, h)
    assert base[0].tobytes() == l[0].tobytes()
    _check_lse("T=%d patterns" % n_samples, l, base[3], base[4], n_samples)
    lpd = cases.finish(*base, n_samples)[0]
    slack = cases.lse_bound(n_samples, lpd)
    for j, name in enumerate(names):
        col = l[:, j]
        assert col.max() - np.log(n_samples) - slack[j] <= lpd[j] <= col.max() + slack[j], name
        if name == "all equal":
            assert base[4][j] == float(n_samples) and base[1][j] == 0.0 and base[2][j] == 0.0
        if name == "one 1e6 below":
            rest = np.delete(col, n_samples // 3)
            assert abs(base[4][j] - np.exp(rest - rest.max()).sum()) <= (2 * n_samples + 16) * U * base[4][j]     # it added exactly 0
    for chunk in (1, 3, n_samples - 1):
        _same(cases.raw((n_i, n_j), rows, cols, np.zeros(len(rows)), A, None, B, 0, 1, n_samples, c, h, chunk), base, "chunk_samples=%d" % chunk)


def test_one_sample_gives_its_own_log_likelihood():
    rows, cols, twins, values, A, S, B, taus, c, h, p, l = cases.real_case(5, 3)
    one = cases.raw((I, J), rows, cols, values, A, S, B, FIRST + STEP, STEP, 1, c[1:2], h[1:2])
    assert (one[1] == 0.0).all() and (one[2] == 0.0).all() and not np.signbit(one[1]).any() and (one[4] == 1.0).all()
    assert one[3].tobytes() == one[0].tobytes()
    Q = log_predictive.from_samples((A, S, B), taus, (I, J), rows, cols, values, [FIRST + STEP])
    assert Q.count == 1 and Q.lpd.tobytes() == one[0].tobytes() and Q.mean.tobytes() == one[0].tobytes() and np.isnan(Q.variance).all()
    assert Q.lppd() == float(np.sum(one[0]))
    for f in (Q.waic, Q.p_waic):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            f()
        assert "at least two" in str(e.value)


# ---------------------------------------------------------------- 2, 4: real-valued samples at every launch shape
def _compare(name, W, c, h, values, p, l, lpd, mean, var):
    """the asserts of item 4 against NumPy fp64 (p, l: the reference's); prints the largest ratios of difference to bound"""
    n_samples = len(l)
    d = values[None, :] - p
    D = 2 * W * U * p.max(0)
    dl = (h[:, None] * (2 * np.abs(d) * D + D * D)).max(0)
    ref_lpd = cases.lse(l)[1].astype(np.float64)
    ref_mean = l.mean(0)
    bound = dl + cases.lse_bound(n_samples, ref_lpd)
    r_lpd, r_mean = np.abs(lpd - ref_lpd) / bound, np.abs(mean - ref_mean) / bound
    ref_var = l.var(0, ddof=1)
    smax = np.abs(l - l[0]).max(0)
    el = dl + 4 * U * (np.abs(c)[:, None] + h[:, None] * d * d).max(0)
    vbound = RTOL * ref_var + n_samples / (n_samples - 1.0) * (8 * el * smax + 4 * (n_samples + 4) * U * smax ** 2)
    r_var = np.abs(var - ref_var) / vbound
    print("%s: largest difference / bound: lpd %.3g, mean %.3g, variance %.3g" % (name, r_lpd.max(), r_mean.max(), r_var.max()))
    assert r_lpd.max() <= 1.0, "%s: lpd off by %.3g of its bound at entry %d" % (name, r_lpd.max(), int(r_lpd.argmax()))
    assert r_mean.max() <= 1.0, "%s: mean off by %.3g of its bound at entry %d" % (name, r_mean.max(), int(r_mean.argmax()))
    assert r_var.max() <= 1.0, "%s: variance off by %.3g of its bound at entry %d" % (name, r_var.max(), int(r_var.argmax()))
    slack = cases.lse_bound(n_samples, ref_lpd)
    assert (lpd <= l.max(0) + bound).all() and (lpd >= mean - slack).all()           # below the best sample; Jensen


@pytest.mark.parametrize("K, L", cases.SHAPES)
def test_the_c_call_matches_numpy_at_every_launch_shape(K, L):
    rows, cols, twins, values, A, S, B, taus, c, h, p, l = cases.real_case(K, L)
    assert p.sum() > 0 and len(rows) > 5000
    got = cases.raw((I, J), rows, cols, values, A, S, B, FIRST, STEP, T, c, h)
    assert not any(np.isnan(g).any() for g in got)
    lpd, mean, var = cases.finish(*got, T)
    name = "%d x %d K=%d L=%d" % (I, J, K, L)
    _compare(name, K + L, c, h, values, p, l, lpd, mean, var)
    # item 2 on real values: the recurrence alone, on the device's own l_t
    dev_l = _device_l((I, J), rows, cols, values, A, S, B, SEL, c, h)
    assert dev_l[0].tobytes() == got[0].tobytes()
    _check_lse(name, dev_l, got[3], got[4], T)


def test_a_matrix_of_many_short_rows():
    """1100 x 7: 275 blocks, rows of 0, 1, 3 and 65 entries"""
    n_i, n_j, K = 1100, 7, 3
    rs = np.random.RandomState(3)
    per_row = np.array([(0, 1, 3, 65)[i % 4] for i in range(n_i)])
    rows = np.repeat(np.arange(n_i), per_row)
    order = rs.permutation(len(rows))
    rows = rows[order].astype(np.int32); cols = rs.randint(n_j, size=len(rows)).astype(np.int32)
    A = rs.exponential(1.0, (STORED, n_i, K)).astype(np.float32); B = rs.exponential(1.0, (STORED, n_j, K)).astype(np.float32)
    taus = rs.gamma(4.0, 0.5, STORED)
    p = cases.predictions(rows, cols, A, None, B, SEL)
    values = p[1] + rs.randn(len(rows))
    c, h = 0.5 * (np.log(taus[SEL]) - np.log(2.0 * np.pi)), 0.5 * taus[SEL]
    d = values[None, :] - p
    l = c[:, None] - h[:, None] * d * d
    assert (n_i + 3) // 4 == 275
    got = cases.raw((n_i, n_j), rows, cols, values, A, None, B, FIRST, STEP, T, c, h)
    _compare("1100 x 7 K=3", K, c, h, values, p, l, *cases.finish(*got, T))
    _same(cases.raw((n_i, n_j), rows, cols, values, A, None, B, FIRST, STEP, T, c, h, 2), got)


# ---------------------------------------------------------------- 5: bits that must not move
@pytest.mark.parametrize("K, L", cases.SHAPES)
def test_the_bits_depend_on_the_entry_its_value_and_the_samples_alone(K, L):
    rows, cols, twins, values, A, S, B, taus, c, h, p, l = cases.real_case(K, L)
    shape = (I, J)
    base = cases.raw(shape, rows, cols, values, A, S, B, FIRST, STEP, T, c, h)
    assert not any(np.isnan(o).any() for o in base)
    for chunk in CHUNKS:
        _same(cases.raw(shape, rows, cols, values, A, S, B, FIRST, STEP, T, c, h, chunk), base, "chunk_samples=%d" % chunk)
    rev = cases.raw(shape, rows[::-1].copy(), cols[::-1].copy(), values[::-1].copy(), A, S, B, FIRST, STEP, T, c, h, 2)
    _same(rev, [np.ascontiguousarray(b[::-1]) for b in base], "the list reversed")
    for x, y in twins:
        assert rows[x] == rows[y] and cols[x] == cols[y]
        same_value = cases.raw(shape, rows[[x, y]].copy(), cols[[x, y]].copy(), values[[x, x]].copy(), A, S, B, FIRST, STEP, T, c, h)
        for g, b in zip(same_value, base):
            assert g[0].tobytes() == g[1].tobytes() == b[x].tobytes()
    # an entry on its own: what else is in the list does not matter
    x = twins[0][0]
    alone = cases.raw(shape, rows[x:x + 1].copy(), cols[x:x + 1].copy(), values[x:x + 1].copy(), A, S, B, FIRST, STEP, T, c, h, 3)
    for a, b in zip(alone, base):
        assert a[0].tobytes() == b[x].tobytes()
    # step 1 on the selected samples alone
    stop = FIRST + (T - 1) * STEP + 1
    sliced = [None if a is None else np.ascontiguousarray(a[FIRST:stop:STEP]) for a in (A, S, B)]
    _same(cases.raw(shape, rows, cols, values, *sliced, 0, 1, T, c, h), base, "pre-sliced samples")


def test_from_samples_finishes_the_c_calls_sums_and_takes_fp64_and_strided_arrays():
    rows, cols, twins, values, A, S, B, taus, c, h, p, l = cases.real_case(5, 3)
    got = cases.raw((I, J), rows, cols, values, A, S, B, FIRST, STEP, T, c, h)
    lpd, mean, var = cases.finish(*got, T)
    Q = log_predictive.from_samples((A, S, B), taus, (I, J), rows, cols, values, SEL, chunk_samples=2)
    assert Q.lpd.tobytes() == lpd.tobytes() and Q.mean.tobytes() == mean.tobytes() and Q.variance.tobytes() == var.tobytes() and Q.count == T
    assert np.array_equal(Q.rows, rows) and np.array_equal(Q.cols, cols) and Q.rows.dtype == np.int32 and np.array_equal(Q.values, values)
    assert len(Q) == len(rows) and all(a.dtype == np.float64 for a in (Q.lpd, Q.mean, Q.variance, Q.values))
    # fp64 arrays, lists of arrays and arrays that are not contiguous take the cast path: the same bits
    wide = [np.ascontiguousarray(np.repeat(a, 2, axis=2))[:, :, ::2] for a in (A, S, B)]
    assert not any(w.flags["C_CONTIGUOUS"] for w in wide)
    for factors in ([a.astype(np.float64) for a in (A, S, B)], [list(a) for a in (A, S, B)], wide):
        P = log_predictive.from_samples(factors, list(taus), (I, J), rows.astype(np.int64), list(cols), list(values), range(FIRST, STORED - 3, STEP))
        assert P.lpd.tobytes() == lpd.tobytes() and P.mean.tobytes() == mean.tobytes() and P.variance.tobytes() == var.tobytes()
    # the statistics of the whole list
    elpd = lpd - var
    assert Q.lppd() == float(np.sum(lpd)) and Q.p_waic() == float(np.sum(var)) and Q.waic() == -2.0 * (float(np.sum(lpd)) - float(np.sum(var)))
    assert np.array_equal(Q.pointwise(), elpd) and Q.se() == float(np.sqrt(len(rows) * np.var(-2.0 * elpd, ddof=1)))


# ---------------------------------------------------------------- 6: through the models
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
        R, M = _data(40, 30, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False)
    elif kind == "bnmf observed":
        R, M = _data(40, 30, 3); m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmf entries":
        R, M = _data(40, 30, 3)
        E = Entries.from_dense(R, M)
        order = np.random.RandomState(2).permutation(len(E))                # (its list, as it is: not row-major)
        m = bnmf_gibbs_optimised(Entries(E.shape, E.rows[order], E.cols[order], E.values[order]), None, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmtf dense":
        R, M = _data(40, 30, 3, 2); m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False)
    elif kind == "bnmtf observed":
        R, M = _data(40, 30, 3, 2); m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False, layout='observed')
    else:
        R, M = _data(40, 30, 4); m = bnmf_gibbs_optimised(R, M, 70, PRI2, seed=1, verbose=False)
    m.initialise()
    m.run(8)
    return m, R, M


def _snapshot(m):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in vars(m).items()
            if isinstance(v, (np.ndarray, int, float, str, tuple, list, type(None)))}


@pytest.mark.parametrize("kind", ["bnmf dense", "bnmf observed", "bnmf entries", "bnmtf dense", "bnmtf observed", "bnmf blocked K=70"])
def test_log_predictive_of_a_fitted_model(kind):
    m, R, M = _model(kind)
    burn_in, thinning = 2, 2
    sel = list(range(burn_in, 8, thinning))
    tri = isinstance(m, bnmtf_gibbs_optimised)
    stored = [np.asarray(getattr(m, "all_" + f)) for f in m._FACTORS]
    assert all(a.dtype == np.float32 and len(a) == 8 for a in stored)
    before = _snapshot(m)
    W = log_predictive(m, None, burn_in, thinning)
    assert _snapshot(m) == before                       # the model's own attributes: byte for byte what they were
    # the training entries: an Entries-built model's list as it is, else R[M != 0] in row-major order, the values in fp64
    if kind == "bnmf entries":
        rows, cols, values = m.R.rows, m.R.cols, m.R.values
        assert not (np.diff(rows.astype(np.int64) * m.J + cols) > 0).all()
    else:
        rows, cols = np.nonzero(M != 0)
        values = np.asarray(R, dtype=np.float64)[M != 0]
    assert np.array_equal(W.rows, rows) and np.array_equal(W.cols, cols) and W.values.tobytes() == np.ascontiguousarray(values).tobytes()
    assert W.count == len(sel) and len(W) == int(M.sum())
    Q = log_predictive.from_samples(stored, m.all_tau, (m.I, m.J), rows, cols, values, sel)
    for a, b in ((W.lpd, Q.lpd), (W.mean, Q.mean), (W.variance, Q.variance)):
        assert a.tobytes() == b.tobytes() and a.dtype == np.float64
    # against NumPy fp64 on the stored samples
    taus = np.asarray(m.all_tau, dtype=np.float64)[sel]
    c, h = 0.5 * (np.log(taus) - np.log(2.0 * np.pi)), 0.5 * taus
    p = cases.predictions(rows, cols, stored[0], stored[1] if tri else None, stored[-1], sel)
    d = values[None, :] - p
    l = c[:, None] - h[:, None] * d * d
    _compare(kind, m.K + (m.L if tri else 0), c, h, values, p, l, W.lpd, W.mean, W.variance)       # (with lpd <= max l and Jensen)
    # the list's statistics are their formulas on the returned arrays
    elpd = W.lpd - W.variance
    assert W.lppd() == float(np.sum(W.lpd)) and W.p_waic() == float(np.sum(W.variance))
    assert W.waic() == -2.0 * (W.lppd() - W.p_waic()) and np.array_equal(W.pointwise(), elpd)
    assert W.se() == float(np.sqrt(len(W) * np.var(-2.0 * elpd, ddof=1))) and np.isfinite(W.waic()) and W.p_waic() > 0
    # held-out values in any order, entries more than once, as held in fp64
    rs = np.random.RandomState(9)
    n = 50
    hr, hc = rs.randint(m.I, size=n), rs.randint(m.J, size=n)
    hv = R[hr, hc] + 1e-9 * rs.randn(n)                 # (not representable in fp32: taken as held)
    H = log_predictive(m, Entries((m.I, m.J), hr, hc, hv), burn_in, thinning)
    G = log_predictive.from_samples(stored, m.all_tau, (m.I, m.J), hr, hc, hv, sel)
    assert H.lpd.tobytes() == G.lpd.tobytes() and H.values.tobytes() == hv.tobytes()
    assert H.lpd.tobytes() != log_predictive.from_samples(stored, m.all_tau, (m.I, m.J), hr, hc, hv.astype(np.float32), sel).lpd.tobytes()
    one = log_predictive(m, None, 7, 1)
    assert one.count == 1 and np.isnan(one.variance).all() and one.lpd.tobytes() == one.mean.tobytes()
