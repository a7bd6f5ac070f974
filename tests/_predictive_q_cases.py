"""Shapes, entry lists, moments and the NumPy fp64 restatement shared by tests/test_predictive_q_cpu.py and
tests/test_predictive_q_gpu.py (bnmtf_amd.variational_predictive).  No test in here; nothing here touches
the device.

The restatement.  closed_form: the two-factor sum, or the direct seven-term sum of the tri-factorisation, by einsum, in the dtype of
its inputs (int64 moments give the exact integer answer).  definition: for tiny ranks the brute-force definition
sum_{k,k',l,l'} E[F_k F_k'] E[S_kl S_k'l'] E[G_l G_l'] - mean^2 with E[X_a X_b] = x_a x_b + [a = b] var_a.

Shapes: the smallest at which the entry pass can go wrong -- rows with 0, 1, 63, 64, 65, 128 and 129 entries in one list (the
64-entry step and its prefetch), all entries in the last row, a partial last block of four rows, J = 1 and n = 1 at I in {1, 3, 4,
5}, the ranks at which the 16-byte loads, the lanes-along-l loop past 64 and the LDS row width change, non-square (K, L), shuffled
lists with duplicates.  A case is made once, shared and never changed."""
import numpy as np

U = 2.0 ** -53
I, J = 11, 137                                   # three blocks of four rows, the last one partial
COUNTS = (0, 1, 63, 64, 65, 128, 129)
RANKS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130, 256)
PAIRS = tuple((k, k) for k in RANKS) + ((3, 11), (33, 5), (5, 130), (130, 5), (256, 2), (2, 256))
# (I, J, K, L, list): list 'mixed' -- the counts above --, 'last' -- every entry in the last row --, 'one' -- a single entry
SHAPES = ([(I, J, K, 0, 'mixed') for K in RANKS] + [(I, J, K, L, 'mixed') for K, L in PAIRS]
          + [(I, J, 5, 0, 'last'), (I, J, 4, 3, 'last')]
          + [(n_i, 1, K, L, 'one') for n_i in (1, 3, 4, 5) for K, L in ((3, 0), (4, 5))])


def shape_id(s):
    return "%dx%d-K%d-L%d-%s" % s


def bound(K, L):
    """relative bound of the issue: 2 (K L + K + L + 8) 2^-53, no absolute term (every term is non-negative)"""
    return 2.0 * (K * L + K + L + 8) * U


def integer_limit(K, L):
    """what no mean, variance or partial sum of the integer cases exceeds: moments in 0 .. 3 give a variance of at most
    243 K L (K + L) + 513 K L <= 999 (K L)^2, a two-factor one of at most 63 K"""
    return (K * max(L, 1)) ** 2 * 12 ** 3


def _z(v, like):
    return np.zeros_like(like) if v is None else v


def closed_form(rows, cols, EA, VA, ES, VS, EB, VB):
    """(mean, variance) [n] in the dtype of the moments; ES None: two factors.  Any variance may be None: zero."""
    VA, VB = _z(VA, EA), _z(VB, EB)
    if ES is None:
        f, a, g, c = EA[rows], VA[rows], EB[cols], VB[cols]
        mean = np.einsum('ek,ek->e', f, g)
        var = np.einsum('ek,ek->e', a, g * g) + np.einsum('ek,ek->e', c, f * f) + np.einsum('ek,ek->e', a, c)
        return mean, var
    VS = _z(VS, ES)
    P = EA @ ES                                  # [I][L]
    H = EB @ ES.T                                # [J][K]
    u = VA @ (ES * ES)                           # [I][L]
    wf, wa = (EA * EA) @ VS, VA @ VS             # [I][L]: w = wf + wa
    g, c = EB[cols], VB[cols]
    mean = np.einsum('el,el->e', P[rows], g)
    var = (np.einsum('ek,ek->e', VA[rows], H[cols] * H[cols])
           + np.einsum('el,el->e', c, P[rows] * P[rows])
           + np.einsum('el,el->e', c, u[rows])
           + np.einsum('el,el->e', g * g, wf[rows])
           + np.einsum('el,el->e', g * g, wa[rows])
           + np.einsum('el,el->e', c, wf[rows])
           + np.einsum('el,el->e', c, wa[rows]))
    return mean, var


def definition(rows, cols, EA, VA, ES, VS, EB, VB):
    """(mean, variance) by the definition, O(n K^2 L^2): tiny ranks only.  ES None: S = I, its variance zero."""
    VA, VB = _z(VA, EA), _z(VB, EB)
    if ES is None:
        ES = np.eye(EA.shape[1], dtype=EA.dtype)
    VS = _z(VS, ES)
    K, L = ES.shape
    f, a, g, c = EA[rows], VA[rows], EB[cols], VB[cols]
    FF = np.einsum('ek,eq->ekq', f, f) + np.einsum('ek,kq->ekq', a, np.eye(K, dtype=EA.dtype))
    GG = np.einsum('el,em->elm', g, g) + np.einsum('el,lm->elm', c, np.eye(L, dtype=EA.dtype))
    SS = np.einsum('kl,qm->klqm', ES, ES) + np.einsum('kl,kq,lm->klqm', VS, np.eye(K, dtype=EA.dtype), np.eye(L, dtype=EA.dtype))
    mean = np.einsum('ek,kl,el->e', f, ES, g)
    return mean, np.einsum('ekq,klqm,elm->e', FF, SS, GG) - mean * mean


def entry_list(n_i, n_j, kind, seed):
    """(rows, cols, twins): int32 lists, shuffled, and the positions of entries given twice"""
    rs = np.random.RandomState(seed)
    if kind == 'one':
        return np.array([n_i - 1], dtype=np.int32), np.array([n_j - 1], dtype=np.int32), []
    if kind == 'last':
        rows = np.full(150, n_i - 1)
    else:
        per_row = np.array([COUNTS[i % len(COUNTS)] for i in range(n_i)])
        rows = np.repeat(np.arange(n_i), per_row)
    cols = rs.randint(n_j, size=len(rows))
    # (the twins go to rows of the second round of counts: the first round keeps 0, 1, 63, 64, 65, 128 and 129 entries)
    dup = (0, 70, len(rows) - 1) if kind == 'last' else tuple(int(np.flatnonzero(rows == r)[0]) for r in (n_i - 3, n_i - 2, n_i - 1))
    rows = np.concatenate([rows, [n_i - 1], rows[list(dup)]])
    cols = np.concatenate([cols, [n_j - 1], cols[list(dup)]])
    order = rs.permutation(len(rows))
    where = np.empty(len(rows), dtype=np.int64); where[order] = np.arange(len(rows))
    twins = [(int(where[a]), int(where[len(rows) - 3 + q])) for q, a in enumerate(dup)]
    return rows[order].astype(np.int32), cols[order].astype(np.int32), twins


def moments(n_i, n_j, K, L, integer, seed):
    """(EA, VA, ES, VS, EB, VB); integer: int64 draws from {0, 1, 2, 3}; else exponential means and small variances, float64"""
    rs = np.random.RandomState(seed)
    W = L if L else K

    def pair(shape):
        if integer:
            return rs.randint(4, size=shape).astype(np.int64), rs.randint(4, size=shape).astype(np.int64)
        return rs.exponential(1.0, shape), 0.05 * rs.exponential(1.0, shape)

    EA, VA = pair((n_i, K))
    ES, VS = pair((K, L)) if L else (None, None)
    EB, VB = pair((n_j, W))
    if integer:                                  # the far corner, which every list holds, has a mean and a variance at every rank
        EA[-1, 0], VA[-1, 0], EB[-1, 0], VB[-1, 0] = 2, 1, 3, 1
        if L:
            ES[0, 0], VS[0, 0] = 1, 2
    return EA, VA, ES, VS, EB, VB


_CASES = {}


def case(shape, integer):
    """the list, the moments and the restatement's answer at a shape: dict(rows, cols, twins, m=(EA, VA, ES, VS, EB, VB), mean, var)"""
    key = (shape, bool(integer))
    if key not in _CASES:
        n_i, n_j, K, L, kind = shape
        rows, cols, twins = entry_list(n_i, n_j, kind, seed=1000 * K + L)
        m = moments(n_i, n_j, K, L, integer, seed=7 * K + L + (1 if integer else 0))
        mean, var = closed_form(rows, cols, *m)
        for a in (rows, cols, mean, var) + m:
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = dict(rows=rows, cols=cols, twins=twins, m=m, mean=mean, var=var)
    return _CASES[key]


def as_factors(m, drop=()):
    """the moments as from_moments takes them, fp64; drop: which variances (0: A, 1: S, 2: B) are None"""
    EA, VA, ES, VS, EB, VB = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in m]
    A = (EA, None if 0 in drop else VA)
    B = (EB, None if 2 in drop else VB)
    return (A, B) if ES is None else (A, (ES, None if 1 in drop else VS), B)
