"""Sparse cases of the exact tests of the list forms of the masked K-means kernels (csrc/kernel_kmeans.hip:
kmeans_assign_list_kernel, kmeans_sums_list_kernel, kmeans_set_row_list_kernel), and what the tests share to reach them.

The list forms hold a point's entries ordered by (coordinate & 63, coordinate) -- lane l walks the sub-range with coordinate & 63
== l -- and a coordinate's entries ordered by (point & 3, point) -- point group g walks the sub-range with point & 3 == g.  The
cases put entries where a sub-range can go wrong: a point's single entry in the first lane, the last lane, the first lane's second
stride and the last coordinate; three entries in one lane; a fully observed point of 129 coordinates (lane 0 holds three); a point
and a coordinate without entries; a coordinate whose members all lie in point group 2; 5 and 257 points; 40, 41 and 81 clusters
(one pass, one more cluster than a pass, one more than two passes); about 3 % observed at 257 x 129.

Integers as in tests/_kmeans_cases.py (X, C in [-6, 6]; its Case, assign_reference and sums_reference are the reference here too):
the device must return the reference bit for bit.  Case number n draws from RandomState(SEED + n).
"""
import numpy as np

from _kmeans_cases import Case, INF

SEED = 20261020


def entries(X, M, rs=None):
    """(points, coords, values, n) of the observed entries of (X, M) -- shuffled when a RandomState is given: the list create
    takes them in any order"""
    points, coords = np.nonzero(np.asarray(M) != 0)
    if rs is not None:
        order = rs.permutation(len(points))
        points, coords = points[order], coords[order]
    return (np.ascontiguousarray(points, dtype=np.int32), np.ascontiguousarray(coords, dtype=np.int32),
            np.ascontiguousarray(np.asarray(X, dtype=np.float64)[points, coords]), len(points))


def _sparse(rs, n, d, K, observed):
    X = rs.randint(-6, 7, size=(n, d))
    M = (rs.random_sample((n, d)) < observed).astype(np.uint8)
    C = rs.randint(-6, 7, size=(K, d))
    Mc = (rs.random_sample((K, d)) < 0.8).astype(np.uint8)
    return X, M, C, Mc


def _build():
    cases = []
    rs_of = lambda: np.random.RandomState(SEED + len(cases))

    rs = rs_of()                                            # one entry at coordinate 0 / 63 / 64 / d - 1; three entries in lane 5
    n, d, K = 5, 140, 40
    X, M, C, Mc = _sparse(rs, n, d, K, 0.0)
    Mc[:] = 1
    expect = {}
    for p, (j, c) in enumerate(((0, 3), (63, 39), (64, 0), (d - 1, 17))):
        C[:, j] = 7                                         # one nearest centroid, at distance 0
        M[p, j] = 1; C[c, j] = X[p, j]
        expect[p] = (c, 0.0)
    M[4, [5, 69, 133]] = 1
    C[:, [5, 69, 133]] = 7; C[21, [5, 69, 133]] = X[4, [5, 69, 133]]
    expect[4] = (21, 0.0)
    cases.append(Case("lanes", X, M, C, Mc, [rs.randint(0, K, size=n)], expect=expect))

    rs = rs_of()                                            # point 0 observes all 129 coordinates, the others about a tenth
    n, d, K = 9, 129, 41
    X, M, C, Mc = _sparse(rs, n, d, K, 0.1)
    M[0] = 1
    cases.append(Case("full_point", X, M, C, Mc, [rs.randint(0, K, size=n), np.full(n, 40)]))

    rs = rs_of()                                            # about 3 % observed: point 2 and coordinate 64 without entries, the
    n, d, K = 257, 129, 81                                  # members of coordinate 7 all in point group 2; then a new last row
    X, M, C, Mc = _sparse(rs, n, d, K, 0.03)
    M[2] = 0
    M[:, 64] = 0; M[5, 63] = 1; M[9, 65] = 1
    M[:, 7] = 0; M[[6, 10, 254], 7] = 1
    M[n - 1, [0, 63, 64, 128]] = [1, 1, 0, 1]
    cases.append(Case("sparse", X, M, C, Mc, [rs.randint(0, K, size=n), np.array([39, 40, 79, 80])[rs.randint(0, 4, size=n)]],
                      new_row=rs.randint(-6, 7, size=d), expect={2: (K - 1, INF)}))
    return cases


CASES = _build()


def by_name(name):
    return [c for c in CASES if c.name == name][0]
