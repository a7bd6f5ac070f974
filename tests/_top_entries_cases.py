"""Cases and the NumPy restatement of bnmtf_amd.top_entries, shared by test_top_entries_cpu.py and
test_top_entries_gpu.py.

restate() is the answer written down in NumPy: dense fp64 scores, the excluded entries removed, np.lexsort((cols, -+scores)), the
first n, padded with -1 / nan.  brute_force() is the same by a loop that picks the best remaining candidate n times; the CPU test
holds the one against the other on tiny cases.

The exact cases have integer-valued factors -- 0 .. 7 for two factors, 0 .. 3 for three -- so every product and every partial sum
is an integer below 2^53 at K, L <= 256: the device's fma chain, NumPy's product and any other summation order give the same bits,
and the comparison is `==`.  The rows of B are drawn WITH repeats from a third as many distinct rows, so whole columns score alike
and the tie rule (lower column first) decides most slots; has_boundary_tie() is what each case asserts of that."""
import numpy as np

ROWS = 9                          # kTopRows = 4 rows per block: the last block is partial
STEP = 64                         # kTopStep: columns per wave step
# (J, n, K, L): about a dozen, not the cross product.  J in {1, 63, 64, 65, 200} around the 64-column step, n in {1, 5, 64, 128}
# (two list slots per lane: 64 is the last n on one), K in {1, 5, 32, 64, 65, 256} (odd widths end in an 8-byte load), three with J < n
EXACT = [(1, 1, 1, 0), (63, 5, 5, 0), (64, 64, 32, 0), (65, 64, 64, 0), (200, 128, 65, 0), (200, 5, 256, 0), (63, 128, 5, 0), (65, 1, 1, 0),
         (64, 5, 1, 1), (200, 64, 5, 3), (65, 128, 32, 32), (200, 5, 33, 65), (63, 1, 256, 256)]
# nine column steps, the last of 8 columns: splits 2, 3, 7 cut them 5 + 4, 3 + 3 + 3, 2 + 2 + 2 + 2 + 1 + 0 + 0; 12 leaves three empty
SPLIT_CASES = [(520, 5, 5, 0), (520, 128, 3, 2)]
SPLITS = (1, 2, 3, 7, 12)


def int_factors(J, K, L, seed, rows=ROWS):
    """integer-valued fp64 factors (A, B) or (A, S, B); B's rows repeat"""
    rs = np.random.RandomState(seed)
    top = 4 if L else 8
    W = L if L else K
    A = rs.randint(top, size=(rows, K)).astype(np.float64)
    distinct = rs.randint(top, size=((J + 2) // 3, W)).astype(np.float64)
    B = distinct[rs.randint(len(distinct), size=J)]
    if L:
        return A, rs.randint(top, size=(K, L)).astype(np.float64), np.ascontiguousarray(B)
    return A, np.ascontiguousarray(B)


def exclusion(J, n, seed, rows=ROWS):
    """The excluded entries of a case as (ex_rows, ex_cols), shuffled and with repeats.  Row 0: none; 1: every column; 2: all but
    one; 3: the first and the last column only; 4: exactly min(n, J) candidates left; 5: min(n - 1, J) left (n - 1 <= J: one
    padded slot); 6: every other column; 7: about a third at random; 8 (and beyond): none."""
    rs = np.random.RandomState(seed)
    allc = np.arange(J)
    per_row = {1: allc, 2: np.delete(allc, J // 2), 3: np.unique([0, J - 1]),
               4: rs.permutation(J)[min(n, J):], 5: rs.permutation(J)[min(n - 1, J):], 6: allc[::2], 7: allc[rs.rand(J) < 0.33]}
    er = np.concatenate([np.full(len(c), i) for i, c in per_row.items() if i < rows] + [np.zeros(0)]).astype(np.int32)
    ec = np.concatenate([c for i, c in per_row.items() if i < rows] + [np.zeros(0)]).astype(np.int32)
    if len(er):
        twice = rs.randint(len(er), size=max(3, len(er) // 5))
        er, ec = np.concatenate([er, er[twice]]), np.concatenate([ec, ec[twice]])
        order = rs.permutation(len(er))
        er, ec = er[order], ec[order]
    return np.ascontiguousarray(er), np.ascontiguousarray(ec)


def dense_scores(factors):
    """the I x J scores in fp64, NumPy's summation order (exact for the integer-valued cases)"""
    F = [np.asarray(f, dtype=np.float64) for f in factors]
    return (F[0] @ F[1] @ F[2].T) if len(F) == 3 else F[0] @ F[1].T


def candidates(J, rows, exclude):
    """per selected row the ascending array of its candidate columns"""
    excluded = {}
    if exclude is not None:
        for i, j in zip(*exclude):
            excluded.setdefault(int(i), set()).add(int(j))
    return [np.array([j for j in range(J) if j not in excluded.get(int(i), ())], dtype=np.int64) for i in rows]


def restate(factors, n, rows=None, exclude=None, largest=True, scores=None):
    """(cols int32 [r][n], scores fp64 [r][n], counts int32 [r]) of top_entries.from_factors, in NumPy"""
    P = dense_scores(factors) if scores is None else scores
    rows = np.arange(P.shape[0]) if rows is None else np.asarray(rows)
    cols = np.full((len(rows), n), -1, dtype=np.int32)
    out = np.full((len(rows), n), np.nan)
    counts = np.zeros(len(rows), dtype=np.int32)
    for q, (i, cand) in enumerate(zip(rows, candidates(P.shape[1], rows, exclude))):
        s = P[i, cand]
        order = np.lexsort((cand, -s if largest else s))[:n]
        counts[q] = len(order)
        cols[q, :len(order)] = cand[order]
        out[q, :len(order)] = s[order]
    return cols, out, counts


def brute_force(factors, n, rows=None, exclude=None, largest=True):
    """the same by picking the best remaining candidate n times, with the order spelt out"""
    P = dense_scores(factors)
    rows = np.arange(P.shape[0]) if rows is None else np.asarray(rows)
    cols = np.full((len(rows), n), -1, dtype=np.int32)
    out = np.full((len(rows), n), np.nan)
    counts = np.zeros(len(rows), dtype=np.int32)

    def first(a, b, i):                  # does column a come before column b in row i?
        sa, sb = (P[i, a], P[i, b]) if largest else (-P[i, a], -P[i, b])
        return sa > sb or (sa == sb and a < b)

    for q, (i, cand) in enumerate(zip(rows, candidates(P.shape[1], rows, exclude))):
        left = list(cand)
        while left and counts[q] < n:
            best = left[0]
            for j in left[1:]:
                if first(j, best, i):
                    best = j
            left.remove(best)
            cols[q, counts[q]], out[q, counts[q]] = best, P[i, best]
            counts[q] += 1
    return cols, out, counts


def has_boundary_tie(factors, n, exclude, largest=True):
    """True when some row's n-th and (n + 1)-th candidates score alike -- the tie rule then decides which of them is returned.  A
    case in which no row has more than n candidates (J <= n) has no such pair: for it, True when two neighbouring returned slots
    of some row score alike (the tie rule then decides their order); None when no row has two candidates at all (J = 1)."""
    cols, scores, counts = restate(factors, n + 1, None, exclude, largest)
    if (counts > n).any():
        return bool(((counts > n) & (scores[:, n - 1] == scores[:, n])).any())
    if (counts < 2).all():
        return None
    return bool((scores[:, 1:] == scores[:, :-1]).any())


def float_factors(K, L, seed=3, I=97, J=83):
    """exponential fp64 factors and a 0/1 mask of the excluded entries: every row and column keeps candidates and exclusions"""
    rs = np.random.RandomState(seed)
    A = rs.exponential(1.0, (I, K))
    B = rs.exponential(1.0, (J, L if L else K))
    S = rs.exponential(1.0, (K, L)) if L else None
    M = (rs.rand(I, J) < 0.3).astype(float)
    M[np.arange(I), np.arange(I) % J] = 1; M[np.arange(J) % I, np.arange(J)] = 1
    return ((A, S, B) if L else (A, B)), M
