"""Cases of the exact tests of the masked K-means kernels (csrc/kernel_kmeans.hip: kmeans_assign_kernel, kmeans_sums_kernel)
and NumPy models of their launches.

Assignment: a wave per point, four points per block, lanes striding the coordinates by 64; per centroid num = sum of squared
differences and overlap = count over the coordinates both know, mse = num / overlap; every cluster replaces the choice until
a defined MSE has been seen, after that only a strictly smaller defined one does (kmeans.py:104-113); distance +inf when none
is defined.  Sums: passes of 40 clusters, a block per 64 coordinates with four point groups (p = g, g + 4, ...) accumulating
in private LDS, added in order; cnt[c][j] = members of c observing j, tot[c][j] = the sum of their values.

X, the centroids and the masks are integers (X in [-6, 6]): num and overlap are integers far below 2^53 whatever the order of
the lanes, mse is ONE correctly rounded division of two exact doubles, counts and totals are integers -- the device must
return the reference bit for bit.  Seeds: case number n of CASES draws from RandomState(SEED + n).
"""
import numpy as np

SEED = 20261019
LANES, POINTS_PER_BLOCK, PASS, GROUPS = 64, 4, 40, 4           # kernel_kmeans.hip
INF = float("inf")


class Case:
    def __init__(self, name, X, M, C, Mc, sums, new_row=None, expect=None):
        self.name = name
        self.X, self.M = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(M, dtype=np.uint8)
        self.C, self.Mc = np.ascontiguousarray(C, dtype=np.float64), np.ascontiguousarray(Mc, dtype=np.uint8)
        self.sums = [np.ascontiguousarray(a, dtype=np.int32) for a in sums]     # assignments handed to bnmtf_kmeans_sums, in turn
        self.new_row = None if new_row is None else np.ascontiguousarray(new_row, dtype=np.float64)   # bnmtf_kmeans_set_row(n - 1, .)
        self.expect = expect or {}                                              # point -> (cluster, distance or None): what the case is about
        self.n, self.d = self.X.shape
        self.K = self.C.shape[0]

    @property
    def id(self):
        return "%s-%dx%dx%d" % (self.name, self.n, self.d, self.K)

    def X_after(self):
        X = self.X.copy()
        if self.new_row is not None:
            X[self.n - 1] = self.new_row
        return X


# ------------------------------------------------------------------ the reference
def distances(X, M, C, Mc, d_used=None):
    """num [n][K], overlap [n][K] as Python-exact int64 (over the first d_used coordinates)"""
    d = X.shape[1] if d_used is None else d_used
    Xi, Ci = X[:, :d].astype(np.int64), C[:, :d].astype(np.int64)
    assert np.array_equal(Xi, X[:, :d]) and np.array_equal(Ci, C[:, :d])
    both = ((M[:, None, :d] != 0) & (Mc[None, :, :d] != 0)).astype(np.int64)
    df = Xi[:, None, :] - Ci[None, :, :]
    return (both * df * df).sum(axis=2), both.sum(axis=2)


def choose(num, ov, fault=None):
    """the choice of kmeans.py:104-113 for every point: (assign int32, dist fp64)"""
    n, K = num.shape
    assign, dist = np.zeros(n, np.int32), np.zeros(n)
    for p in range(n):
        best, best_mse, have = -1, 0.0, False
        for c in range(K):
            defined = ov[p, c] > 0
            mse = float(num[p, c]) / float(ov[p, c]) if defined else 0.0
            if not have:
                if fault == "undefined_first_keeps" and best >= 0 and not defined:
                    continue
                best, have, best_mse = c, defined, mse
            elif defined and (mse <= best_mse if fault == "le_compare" else mse < best_mse):
                best, best_mse = c, mse
        assign[p], dist[p] = best, best_mse if have else INF
    return assign, dist


def assign_reference(X, M, C, Mc):
    return choose(*distances(X, M, C, Mc))


def sums_reference(X, M, assign, K):
    Xi, Mi = X.astype(np.int64), (M != 0).astype(np.int64)
    onehot = (assign[:, None] == np.arange(K)[None, :]).astype(np.int64)
    return (onehot.T @ Mi).astype(np.float64), (onehot.T @ (Xi * Mi)).astype(np.float64)


# ------------------------------------------------------------------ models of the launches, one line changed per fault
ASSIGN_FAULTS = ("lanes_stop_at_full_strides", "le_compare", "undefined_first_keeps", "tail_points_skipped")
SUMS_FAULTS = ("pass_writes_at_c", "fourth_group_dropped")


def assign_model(X, M, C, Mc, fault=None):
    n, d = X.shape
    num, ov = distances(X, M, C, Mc, d - d % LANES if fault == "lanes_stop_at_full_strides" else None)
    assign, dist = choose(num, ov, fault)
    if fault == "tail_points_skipped":                      # a grid of n / 4 blocks: the last n % 4 points are never written
        assign[n - n % POINTS_PER_BLOCK:] = -1; dist[n - n % POINTS_PER_BLOCK:] = 0.0
    return assign, dist


def sums_model(X, M, assign, K, fault=None):
    n, d = X.shape
    Xi, Mi = X.astype(np.int64), (M != 0).astype(np.int64)
    cnt, tot = np.zeros((K, d)), np.zeros((K, d))
    groups = GROUPS - 1 if fault == "fourth_group_dropped" else GROUPS
    for c0 in range(0, K, PASS):
        KC = min(PASS, K - c0)
        ac, at = np.zeros((GROUPS, KC, d), np.int64), np.zeros((GROUPS, KC, d), np.int64)
        for g in range(GROUPS):
            for p in range(g, n, GROUPS):
                c = int(assign[p]) - c0
                if 0 <= c < KC:
                    ac[g, c] += Mi[p]; at[g, c] += Xi[p] * Mi[p]
        for c in range(KC):
            row = c if fault == "pass_writes_at_c" else c0 + c
            cnt[row], tot[row] = ac[:groups, c].sum(axis=0), at[:groups, c].sum(axis=0)
    return cnt, tot


# ------------------------------------------------------------------ the cases
def _random(rs, n, d, K, observed=0.7):
    X = rs.randint(-6, 7, size=(n, d))
    M = (rs.random_sample((n, d)) < observed).astype(np.uint8)
    for p in np.flatnonzero(M.sum(axis=1) == 0):
        M[p, rs.randint(d)] = 1
    C = rs.randint(-6, 7, size=(K, d))
    Mc = (rs.random_sample((K, d)) < 0.8).astype(np.uint8)
    return X, M, C, Mc


SHAPES = [(1, 1, 1), (3, 63, 2), (4, 64, 39), (5, 65, 40), (255, 128, 41), (256, 129, 80), (257, 1, 81), (257, 129, 81)]


def _near(rs, v, n):
    """n points within one unit of the integer vector v (|v| <= 3), everything observed"""
    return v[None, :] + rs.randint(-1, 2, size=(n, len(v)))


def _build():
    cases = []
    rs_of = lambda: np.random.RandomState(SEED + len(cases))

    for n, d, K in SHAPES:
        rs = rs_of()
        X, M, C, Mc = _random(rs, n, d, K)
        cases.append(Case("shape", X, M, C, Mc, [rs.randint(0, K, size=n)]))

    for ties in (2, 3):                                     # identical centroids 0 .. ties - 1, nearest to every point: the lowest index wins
        rs = rs_of()
        n, d, K = 5, 65, ties + 2
        v = rs.randint(-3, 4, size=d)
        C = np.stack([v] * ties + [v + 5, v - 5])
        Mc = np.ones((K, d), np.uint8)
        Mc[:ties] = (rs.random_sample(d) < 0.8).astype(np.uint8)[None, :]
        Mc[:ties, d - 1] = 1
        X = _near(rs, v, n)
        cases.append(Case("tie%d" % ties, X, np.ones((n, d), np.uint8), C, Mc, [rs.randint(0, K, size=n)],
                          expect={p: (0, None) for p in range(n)}))

    rs = rs_of()                                            # centroid 0 undefined for every point, then the tie 1 = 2: 1 wins
    n, d, K = 5, 65, 4
    v = rs.randint(-3, 4, size=d)
    C = np.stack([v, v, v, v + 5])
    Mc = np.ones((K, d), np.uint8); Mc[0, 8:] = 0
    M = np.ones((n, d), np.uint8); M[:, :8] = 0
    cases.append(Case("tie_after_undefined", _near(rs, v, n), M, C, Mc, [rs.randint(0, K, size=n)], expect={p: (1, None) for p in range(n)}))

    rs = rs_of()                                            # point 2 observes only coordinates 3 and 64, which no centroid knows
    n, d, K = 6, 65, 5
    X, M, C, Mc = _random(rs, n, d, K)
    M[2] = 0; M[2, [3, 64]] = 1
    Mc[:, [3, 64]] = 0
    cases.append(Case("no_overlap", X, M, C, Mc, [rs.randint(0, K, size=n)], expect={2: (K - 1, INF)}))

    rs = rs_of()                                            # points whose only overlap is coordinate d - 1 = 99 / 64 / 63
    n, d, K = 7, 100, 6
    X, M, C, Mc = _random(rs, n, d, K)
    Mc[:] = 1
    for p, (j, c) in enumerate(((99, 3), (64, 2), (63, 4))):
        C[:, j] = np.arange(K) - 3                          # distinct values: one nearest centroid
        M[p] = 0; M[p, j] = 1
        X[p, j] = C[c, j]
    cases.append(Case("single_overlap", X, M, C, Mc, [rs.randint(0, K, size=n)], expect={0: (3, 0.0), 1: (2, 0.0), 2: (4, 0.0)}))

    rs = rs_of()                                            # centroid 2 sits ON point 0 but knows no coordinate: never chosen
    n, d, K = 20, 65, 6
    X, M, C, Mc = _random(rs, n, d, K)
    C[2] = X[0]; Mc[2] = 0
    cases.append(Case("zero_mask_centroid", X, M, C, Mc, [rs.randint(0, K, size=n)]))

    rs = rs_of()
    n, d, K = 257, 65, 3
    X, M, C, Mc = _random(rs, n, d, K)
    cases.append(Case("sums_one_cluster", X, M, C, Mc, [np.ones(n, np.int32)]))

    rs = rs_of()                                            # the last cluster of pass one and two, the first of pass two and three
    n, d, K = 256, 65, 81
    X, M, C, Mc = _random(rs, n, d, K)
    cases.append(Case("sums_straddle_passes", X, M, C, Mc, [np.array([39, 40, 79, 80])[rs.randint(0, 4, size=n)]]))

    rs = rs_of()                                            # no member of cluster 0 observes coordinates 64 and 69
    n, d, K = 9, 70, 2
    X, M, C, Mc = _random(rs, n, d, K, observed=0.9)
    M[:5, [64, 69]] = 0; M[5:, [64, 69]] = 1
    cases.append(Case("sums_unobserved_coordinate", X, M, C, Mc, [np.array([0] * 5 + [1] * 4)]))

    rs = rs_of()                                            # every cluster occupied, then only clusters 0 and 41
    n, d, K = 90, 65, 45
    X, M, C, Mc = _random(rs, n, d, K)
    cases.append(Case("sums_twice", X, M, C, Mc, [np.arange(n) % K, np.array([0, 41])[rs.randint(0, 2, size=n)]]))

    rs = rs_of()                                            # the last point sits on centroid 0, its new row on centroid 2
    n, d, K = 5, 65, 3
    X, M, C, Mc = _random(rs, n, d, K)
    M[n - 1] = 1; Mc[:] = 1
    C[2] = -C[0]; C[0, 0], C[2, 0] = 5, -5                  # (so that the two differ)
    X[n - 1] = C[0]
    cases.append(Case("set_row", X, M, C, Mc, [rs.randint(0, K, size=n)], new_row=C[2].copy(), expect={n - 1: (2, 0.0)}))
    return cases


CASES = _build()


def by_name(name):
    return [c for c in CASES if c.name == name]
