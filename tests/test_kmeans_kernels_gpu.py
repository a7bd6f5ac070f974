"""The masked K-means kernels (csrc/kernel_kmeans.hip: kmeans_assign_kernel, kmeans_sums_kernel) checked bit for bit.

Through bnmtf_kmeans_create / _assign / _sums / _set_row / _destroy, as bnmtf_amd/kmeans.py calls them, on integer data
(tests/_kmeans_cases.py; the CPU side, test_kmeans_cases_cpu.py, shows that the cases are exact, that every named situation
occurs in its case and that each single fault of a model of the launches would change a checked output): assignments,
distances (+inf where a point shares no coordinate with any centroid), counts and totals must equal the integer reference."""
import ctypes as C

import numpy as np
import pytest

from bnmtf_amd import _lib
from _kmeans_cases import CASES, assign_reference, sums_reference

pytestmark = pytest.mark.gpu


class Handle:
    def __init__(self, case):
        self.case = case
        self.h = C.c_void_p()
        _lib.check(_lib.lib().bnmtf_kmeans_create(_lib.ptr(case.X), _lib.ptr(case.M), case.n, case.d, int(case.K), 0, C.byref(self.h)))

    def assign(self):
        c = self.case
        a = np.full(c.n, -7, dtype=np.int32); dist = np.full(c.n, -7.0)
        _lib.check(_lib.lib().bnmtf_kmeans_assign(self.h, _lib.ptr(c.C), _lib.ptr(c.Mc), _lib.ptr(a), _lib.ptr(dist)))
        return a, dist

    def sums(self, assign):
        c = self.case
        cnt = np.full((c.K, c.d), -7.0); tot = np.full((c.K, c.d), -7.0)
        _lib.check(_lib.lib().bnmtf_kmeans_sums(self.h, _lib.ptr(assign), _lib.ptr(cnt), _lib.ptr(tot)))
        return cnt, tot

    def set_last_row(self, values):
        _lib.check(_lib.lib().bnmtf_kmeans_set_row(self.h, self.case.n - 1, _lib.ptr(values)))

    def close(self):
        _lib.lib().bnmtf_kmeans_destroy(self.h)


def _check(h, X, what):
    c = h.case
    a, dist = h.assign()
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


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_assignment_and_sums_are_exact(case):
    h = Handle(case)
    try:
        a, dist = _check(h, case.X, "as created")
        if case.new_row is not None:
            h.set_last_row(case.new_row)
            a, dist = _check(h, case.X_after(), "after set_row")
        for p, (c, dv) in case.expect.items():
            assert a[p] == c and (dv is None or dist[p] == dv), (p, a[p], dist[p])
    finally:
        h.close()
