"""The list forms of the masked K-means kernels (csrc/kernel_kmeans.hip: kmeans_assign_list_kernel, kmeans_sums_list_kernel,
kmeans_set_row_list_kernel) against the integer reference and, bit for bit, against the dense kernels.

A handle of bnmtf_kmeans_create_list takes the observed entries in any order (here: shuffled) and is served by the calls of a dense
handle.  Checked: every case of tests/_kmeans_cases.py and the sparse cases of tests/_kmeans_list_cases.py exactly against
assign_reference / sums_reference (set_row and a second sums call included); real-valued data whose sums round, as uint64 views
against a dense handle of the same (X, M); KMeans(layout='observed') against KMeans() under one random.seed; and the four model
classes' initialise(init_FG='kmeans') on either layout."""
import ctypes as C
import random

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib
from bnmtf_amd.kmeans import KMeans
from _kmeans_cases import CASES, assign_reference, sums_reference
from _kmeans_list_cases import CASES as LIST_CASES, entries

pytestmark = pytest.mark.gpu


class Handle:
    """bnmtf_kmeans_create (lists=False) or bnmtf_kmeans_create_list over the shuffled entries of (X, M)"""

    def __init__(self, X, M, K, lists, seed=0):
        self.n, self.d = X.shape
        self.K = int(K)
        self.h = C.c_void_p()
        if lists:
            p, c, v, n = entries(X, M, np.random.RandomState(seed))
            _lib.check(_lib.lib().bnmtf_kmeans_create_list(self.n, self.d, C.c_uint64(n), _lib.ptr(p), _lib.ptr(c), _lib.ptr(v), self.K, 0, C.byref(self.h)))
        else:
            X = np.ascontiguousarray(X, dtype=np.float64); M = np.ascontiguousarray(M, dtype=np.uint8)
            _lib.check(_lib.lib().bnmtf_kmeans_create(_lib.ptr(X), _lib.ptr(M), self.n, self.d, self.K, 0, C.byref(self.h)))

    def assign(self, Cm, Mc):
        a = np.full(self.n, -7, dtype=np.int32); dist = np.full(self.n, -7.0)
        _lib.check(_lib.lib().bnmtf_kmeans_assign(self.h, _lib.ptr(Cm), _lib.ptr(Mc), _lib.ptr(a), _lib.ptr(dist)))
        return a, dist

    def sums(self, assign):
        cnt = np.full((self.K, self.d), -7.0); tot = np.full((self.K, self.d), -7.0)
        _lib.check(_lib.lib().bnmtf_kmeans_sums(self.h, _lib.ptr(assign), _lib.ptr(cnt), _lib.ptr(tot)))
        return cnt, tot

    def set_row(self, index, values):
        _lib.check(_lib.lib().bnmtf_kmeans_set_row(self.h, int(index), _lib.ptr(values)))

    def close(self):
        _lib.lib().bnmtf_kmeans_destroy(self.h)


# ------------------------------------------------------------------ exact against the integer reference
def _check(h, c, X, what):
    a, dist = h.assign(c.C, c.Mc)
    ra, rdist = assign_reference(X, c.M, c.C, c.Mc)
    bad = np.flatnonzero((a != ra) | (dist != rdist))
    assert bad.size == 0, "%s %s: %d points wrong, first %s: got %r / %r, want %r / %r" % (
        c.id, what, bad.size, bad[:4].tolist(), a[bad[:4]].tolist(), dist[bad[:4]].tolist(), ra[bad[:4]].tolist(), rdist[bad[:4]].tolist())
    assert np.array_equal(a, ra) and np.array_equal(dist, rdist)
    for turn, s in enumerate(c.sums):                        # (a second call holds nothing of the first)
        cnt, tot = h.sums(s)
        rcnt, rtot = sums_reference(X, c.M, s, c.K)
        for name, got, want in (("cnt", cnt, rcnt), ("tot", tot, rtot)):
            bad = np.argwhere(got != want)
            assert bad.size == 0, "%s %s, sums call %d: %s wrong at %d (cluster, coordinate) pairs, first %s: got %r, want %r" % (
                c.id, what, turn, name, len(bad), bad[:4].tolist(), [got[tuple(b)] for b in bad[:4]], [want[tuple(b)] for b in bad[:4]])
    return a, dist


EXACT = CASES + LIST_CASES


@pytest.mark.parametrize("case", EXACT, ids=[("dense-" if c in CASES else "list-") + c.id for c in EXACT])
def test_a_list_handle_is_exact_on_integer_data(case):
    h = Handle(case.X, case.M, case.K, lists=True, seed=len(case.id))
    try:
        a, dist = _check(h, case, case.X, "as created")
        if case.new_row is not None:
            h.set_row(case.n - 1, case.new_row)
            a, dist = _check(h, case, case.X_after(), "after set_row")
        for p, (c, dv) in case.expect.items():
            assert a[p] == c and (dv is None or dist[p] == dv), (p, a[p], dist[p])
    finally:
        h.close()


# ------------------------------------------------------------------ the same bits as the dense form
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n,d,K,observed", [(257, 129, 41, 0.30), (257, 129, 41, 0.03), (64, 64, 3, 0.30)])
def test_list_and_dense_handles_return_the_same_bits(n, d, K, observed):
    """randn scaled by 1e3: 53-bit products and sums that round at every step, so any other summation order shows"""
    rs = np.random.RandomState(77 + n + K + int(100 * observed))
    X = rs.randn(n, d) * 1e3
    M = (rs.random_sample((n, d)) < observed).astype(np.uint8)
    Cm = np.ascontiguousarray(rs.randn(K, d) * 1e3); Mc = (rs.random_sample((K, d)) < 0.8).astype(np.uint8)
    s = [rs.randint(0, K, size=n).astype(np.int32), rs.randint(-1, K, size=n).astype(np.int32)]       # (-1: in no cluster)
    row = n // 2
    new_row = np.ascontiguousarray(rs.randn(d) * 1e3)
    dense, lists = Handle(X, M, K, lists=False), Handle(X, M, K, lists=True, seed=n + d)
    try:
        for what in ("as created", "after set_row"):
            (a0, d0), (a1, d1) = dense.assign(Cm, Mc), lists.assign(Cm, Mc)
            assert np.array_equal(a0, a1), (what, np.flatnonzero(a0 != a1)[:8])
            assert np.array_equal(_bits(d0), _bits(d1)), (what, np.flatnonzero(_bits(d0) != _bits(d1))[:8])
            assert np.isfinite(d0).sum() > n // 2 and len(set(a0.tolist())) > 1
            for turn in s:
                (c0, t0), (c1, t1) = dense.sums(turn), lists.sums(turn)
                assert np.array_equal(_bits(c0), _bits(c1)), (what, np.argwhere(_bits(c0) != _bits(c1))[:8])
                assert np.array_equal(_bits(t0), _bits(t1)), (what, np.argwhere(_bits(t0) != _bits(t1))[:8])
                assert c0.max() >= 2 or observed < 0.1       # (sums of several members: an order to get wrong)
            dense.set_row(row, new_row); lists.set_row(row, new_row)
    finally:
        dense.close(); lists.close()


# ------------------------------------------------------------------ the class
def test_the_class_clusters_alike_on_either_layout():
    """60 x 45 at 20 % observed, K = 16, random.seed(3): picked with oracle/kmeans_oracle.py alone (eight iterations, two singleton
    refills, no point without overlap; at the K = 8 of a first try no seed below 40 empties a cluster on this data) -- conditions on
    the reference, asserted here on the dense run."""
    rs = np.random.RandomState(20261020)
    n, d, K = 60, 45, 16
    X = rs.randn(n, d) * 1e3
    M = (rs.random_sample((n, d)) < 0.2).astype(float)
    for p in np.flatnonzero(M.sum(axis=1) == 0):
        M[p, rs.randint(d)] = 1
    runs = []
    for kw in ({}, dict(layout='observed')):
        km = KMeans(X, M, K, **kw)
        km.initialise(3)
        km.cluster()
        runs.append(km)
        km.close()
    dense, lists = runs
    assert len(dense.assign_hist) >= 3 and sum(a is not None for a in dense._alias) >= 1
    assert np.array_equal(np.array(dense.assign_hist), np.array(lists.assign_hist))
    assert np.array_equal(_bits(np.array(dense.centroids)), _bits(np.array(lists.centroids)))
    assert np.array_equal(dense.mask_centroids, lists.mask_centroids)
    assert np.array_equal(dense.clustering_results, lists.clustering_results)
    assert dense._alias == lists._alias and np.array_equal(_bits(dense.X), _bits(lists.X))


# ------------------------------------------------------------------ the models
PRIORS = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
PAIRS = [
    ("bnmtf_gibbs_optimised", lambda R, M, obs: bnmtf_amd.bnmtf_gibbs_optimised(R, M, 3, 2, PRIORS, verbose=False, seed=1, **(dict(layout='observed') if obs else {})), ("F", "G")),
    ("nmtf_icm", lambda R, M, obs: bnmtf_amd.nmtf_icm(R, M, 3, 2, PRIORS, verbose=False, seed=1, **(dict(layout='observed') if obs else {})), ("F", "G")),
    ("bnmtf_vb", lambda R, M, obs: (bnmtf_amd.bnmtf_vb_observed if obs else bnmtf_amd.bnmtf_vb_optimised)(R, M, 3, 2, PRIORS, verbose=False), ("muF", "muG")),
    ("NMTF", lambda R, M, obs: bnmtf_amd.NMTF(R, M, 3, 2, verbose=False, **(dict(layout='observed') if obs else {})), ("F", "G")),
]


@pytest.mark.parametrize("name,make,factors", PAIRS, ids=[p[0] for p in PAIRS])
def test_kmeans_initialisation_is_the_same_on_either_layout(name, make, factors):
    from bnmtf_amd.synthetic import generate_bnmtf
    R, M, _, _, _ = generate_bnmtf(60, 40, 3, 2, 0.7, seed_data=5, seed_mask=6)
    got = []
    for obs in (False, True):
        m = make(R, M, obs)
        random.seed(0); np.random.seed(0)
        m.initialise('random', 'kmeans')
        got.append([np.array(getattr(m, f)) for f in factors])
        if obs:
            m.run(2)
            assert np.isfinite(m.all_performances['MSE']).all()
        m.close()
    for f, x, y in zip(factors, got[0], got[1]):
        assert np.array_equal(x, y), (name, f)
        assert len(np.unique(np.argmax(x, axis=1))) > 1, (name, f)        # (a clustering, not one cluster)
