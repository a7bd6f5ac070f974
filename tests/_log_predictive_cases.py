"""Lists, samples, raw calls and NumPy restatements shared by tests/test_log_predictive_gpu.py: test_predictive_gpu.py's launch
shapes (the kernel is its gather with another tail), with values and the two per-sample numbers c and h beside them.  Every case
is made once, write-protected and shared."""
import ctypes as C

import numpy as np

from bnmtf_amd import _lib

U = 2.0 ** -53
I, J = 97, 83                     # the last block of 4 rows is partial
STORED, FIRST, STEP, T = 20, 2, 3, 5
SEL = list(range(FIRST, FIRST + T * STEP, STEP))
TWO = (1, 3, 4, 5, 32, 64, 65, 255, 256)
TRI = ((1, 1), (3, 5), (5, 3), (32, 32), (33, 7), (64, 65), (256, 2), (2, 256))
SHAPES = [(K, 0) for K in TWO] + list(TRI)
EXACT = [(5, 0), (65, 0), (256, 0), (32, 32), (64, 65), (256, 2)]
CHUNKS = (0, 1, 2, 4, 5, 9)
COUNTS = (0, 1, 63, 64, 65, 129)  # entries per row, by i % 6: 129 is the lane loop's third trip
H_EXACT = np.array([0.25, 0.5, 0.125, 0.25, 1.0])
C_EXACT = np.array([-0.75, 1.5, -2.25, 0.5, -1.0])


def entry_list(seed):
    """Rows with COUNTS[i % 6] entries (columns drawn with replacement: a row may be longer than the matrix is wide), the far
    corner, three entries given twice at the end of the list before the shuffle; (rows, cols, positions of the twins)."""
    rs = np.random.RandomState(seed)
    per_row = np.array([COUNTS[i % len(COUNTS)] for i in range(I)])
    rows = np.repeat(np.arange(I), per_row)
    cols = rs.randint(J, size=len(rows))
    rows = np.concatenate([rows, [I - 1], rows[[0, 70, 200]]])
    cols = np.concatenate([cols, [J - 1], cols[[0, 70, 200]]])
    order = rs.permutation(len(rows))
    where = np.empty(len(rows), dtype=np.int64); where[order] = np.arange(len(rows))
    twins = [(where[a], where[len(rows) - 3 + q]) for q, a in enumerate((0, 70, 200))]
    return rows[order].astype(np.int32), cols[order].astype(np.int32), twins


def raw(shape, rows, cols, values, A, S, B, first, step, n_samples, c, h, chunk=0):
    """bnmtf_log_predictive_samples as it stands: [l_first, sum_d, sum_d2, l_max, sum_exp]"""
    n = len(rows)
    out = [np.full(n, np.nan) for _ in range(5)]
    values, c, h = (np.ascontiguousarray(a, dtype=np.float64) for a in (values, c, h))
    assert len(c) == n_samples and len(h) == n_samples
    _lib.check(_lib.lib().bnmtf_log_predictive_samples(0, shape[0], shape[1], A.shape[2], S.shape[2] if S is not None else 0, C.c_uint64(n),
                                                       _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(values), _lib.ptr(A), _lib.ptr(S), _lib.ptr(B),
                                                       C.c_uint64(first), C.c_uint64(step), n_samples, chunk, _lib.ptr(c), _lib.ptr(h),
                                                       *[_lib.ptr(o) for o in out]))
    return out


def predictions(rows, cols, A, S, B, sel, dtype=np.float64):
    """p [T][n] of the selected samples, in `dtype` (int64 for integer samples: exact)"""
    p = np.empty((len(sel), len(rows)), dtype=dtype)
    for q, t in enumerate(sel):
        a = A[t].astype(dtype)
        if S is not None:
            a = a @ S[t].astype(dtype)
        p[q] = np.einsum('ek,ek->e', a[rows], B[t].astype(dtype)[cols])
    return p


def lse(l):
    """(sum_t exp(l_t - max), log mean exp) of l [T][n], two passes in np.longdouble"""
    x = l.astype(np.longdouble)
    m = x.max(0)
    s = np.exp(x - m).sum(0)
    return s, m + np.log(s) - np.log(np.longdouble(len(l)))


def lse_bound(n_samples, lpd):
    """(2 T + 16) 2^-53 max(1, |lpd_e|): T terms in (0, 1] whose largest is 1, exp and log within 2 ulp, the additions of the
    running sum and of the finish"""
    return (2 * n_samples + 16) * U * np.maximum(1.0, np.abs(np.asarray(lpd, dtype=np.float64)))


def finish(l_first, sum_d, sum_d2, l_max, sum_exp, n_samples):
    """(lpd, mean, variance) as bnmtf_amd.log_predictive finishes them"""
    lpd = l_max + np.log(sum_exp) - np.log(float(n_samples))
    mean = l_first + sum_d / n_samples
    var = np.maximum(0.0, (sum_d2 - sum_d * sum_d / n_samples) / (n_samples - 1)) if n_samples > 1 else np.full(len(l_first), np.nan)
    return lpd, mean, var


def protect(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


_EXACT, _REAL = {}, {}


def exact_case(K, L):
    """Integer samples in {0, 1, 2} held in fp32; r = the integer p of the selected sample 2 plus an integer in [-3, 3]; with
    H_EXACT and C_EXACT every l_t is a multiple of 1/8: (rows, cols, twins, values, A, S, B, p [T][n] in int64, 8 l_t [T][n] as Python integers)."""
    if (K, L) not in _EXACT:
        rows, cols, twins = entry_list(seed=K * 1000 + L)
        rs = np.random.RandomState(K * 7 + L + 1)
        A = rs.randint(0, 3, (STORED, I, K)).astype(np.float32)
        S = rs.randint(0, 3, (STORED, K, L)).astype(np.float32) if L else None
        B = rs.randint(0, 3, (STORED, J, L if L else K)).astype(np.float32)
        p = predictions(rows, cols, A, S, B, SEL, dtype=np.int64)
        r = p[2] + rs.randint(-3, 4, len(rows))
        d = (r[None, :] - p).astype(object)
        h8, c8 = [int(v) for v in H_EXACT * 8], [int(v) for v in C_EXACT * 8]
        l8 = np.array([c8[t] - h8[t] * d[t] * d[t] for t in range(T)], dtype=object)
        values = r.astype(np.float64)
        protect(rows, cols, values, A, S, B, p)
        _EXACT[(K, L)] = (rows, cols, twins, values, A, S, B, p, l8)
    return _EXACT[(K, L)]


def real_case(K, L):
    """Exponential samples as test_predictive_gpu.py's; r = p of the selected sample 1 + N(0, 1); gamma taus: (rows, cols, twins,
    values, A, S, B, taus [STORED], c [T], h [T], p [T][n] in fp64, l [T][n] in fp64)."""
    if (K, L) not in _REAL:
        rows, cols, twins = entry_list(seed=K * 1000 + L)
        rs = np.random.RandomState(K * 7 + L)
        A = rs.exponential(1.0, (STORED, I, K)).astype(np.float32)
        S = rs.exponential(1.0, (STORED, K, L)).astype(np.float32) if L else None
        B = rs.exponential(1.0, (STORED, J, L if L else K)).astype(np.float32)
        taus = rs.gamma(4.0, 0.5, STORED)
        p = predictions(rows, cols, A, S, B, SEL)
        values = p[1] + rs.randn(len(rows))
        c, h = 0.5 * (np.log(taus[SEL]) - np.log(2.0 * np.pi)), 0.5 * taus[SEL]
        d = values[None, :] - p
        l = c[:, None] - h[:, None] * d * d
        protect(rows, cols, values, A, S, B, taus, c, h, p, l)
        _REAL[(K, L)] = (rows, cols, twins, values, A, S, B, taus, c, h, p, l)
    return _REAL[(K, L)]
