"""Host side of the masked K-means on entry lists (csrc/kernel_kmeans.hip): KMeans' `layout` keyword, the two
new entry points in the header and the binding, what bnmtf_kmeans_create_list refuses -- before any device call --, the two orders
and the permutation the host builder makes against np.lexsort, which layout the model classes hand to KMeans, that every named
situation occurs in its case of tests/_kmeans_list_cases.py, the resources of the new kernels and a sanitizer run of the K-means
host code through a stand-alone program.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, kmeans as kmeans_module
from bnmtf_amd.kmeans import KMeans
from _kmeans_cases import assign_reference, INF
from _kmeans_list_cases import CASES, by_name, entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ("bnmtf_kmeans_create_list", "bnmtf_kmeans_build_lists")
EINVAL = -1


# ------------------------------------------------------------------ the class
def test_layout_is_keyword_only_with_dense_as_default():
    p = inspect.signature(KMeans.__init__).parameters
    assert p["layout"].kind is inspect.Parameter.KEYWORD_ONLY and p["layout"].default == 'dense'
    assert list(p)[:5] == ["self", "X", "M", "K", "resolve_empty"] and p["device"].kind is inspect.Parameter.KEYWORD_ONLY
    X = np.arange(12.0).reshape(4, 3); M = np.ones((4, 3))
    assert KMeans(X, M, 2)._layout == 'dense' and KMeans(X, M, 2, layout='dense')._layout == 'dense'
    assert KMeans(X, M, 2, layout='observed')._layout == 'observed'
    with pytest.raises(AssertionError) as e:
        KMeans(X, M, 2, layout='bogus')
    assert str(e.value) == "Unknown layout: bogus. Should be 'dense' or 'observed'."


def test_the_observed_layout_hands_the_entries_of_the_compacted_matrix_to_the_list_create(monkeypatch):
    """column 1 is unobserved and dropped (kmeans.py:19-24): the list is that of the remaining 4 x 2 matrix, fp64, with K and the device"""
    X = np.arange(12.0).reshape(4, 3) / 3.0
    M = np.array([[1, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 1]])
    seen = {}

    class Lib(object):
        def bnmtf_kmeans_create_list(self, n_points, n_coords, n, points, coords, values, K, device, out):
            as_array = lambda p, t: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n.value,)).copy()
            seen.update(shape=(n_points, n_coords), K=K, device=device, points=as_array(points, C.c_int32), coords=as_array(coords, C.c_int32),
                        values=as_array(values, C.c_double))
            return 0

        def __getattr__(self, name):
            raise AssertionError("unexpected device call %s" % name)

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    km = KMeans(X, M, 3, device=0, layout='observed')
    km._device_handle()
    km._dh = None                                           # (nothing to destroy)
    assert seen["shape"] == (4, 2) and seen["K"] == 3 and seen["device"] == 0
    got = sorted(zip(seen["points"].tolist(), seen["coords"].tolist(), seen["values"].tolist()))
    assert got == [(0, 0, X[0, 0]), (0, 1, X[0, 2]), (1, 1, X[1, 2]), (2, 0, X[2, 0]), (3, 0, X[3, 0]), (3, 1, X[3, 2])]


# ------------------------------------------------------------------ the ABI
def test_header_and_binding_list_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmtf_kmeans_\w+)\s*\(", hdr, flags=re.M))
    old = {"bnmtf_kmeans_create", "bnmtf_kmeans_destroy", "bnmtf_kmeans_assign", "bnmtf_kmeans_sums", "bnmtf_kmeans_set_row"}
    assert declared == old | set(NEW)
    assert {n for n in _lib.EXPORTS if "_kmeans_" in n} == old | set(NEW)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    src = open(os.path.join(CSRC, "kernel_kmeans.hip")).read()
    for n in NEW:                                           # every one a function-try-block ending in the guard
        assert re.search(r"^int %s\([^{]*?\) try \{" % n, src, flags=re.M | re.S), n
    assert src.count("} BNMTF_ABI_GUARD") == len(NEW)
    for word in ("atomicAdd", "unsafeAtomicAdd", "__hip_atomic"):                # no floating-point atomics (no device atomics at all)
        assert word not in src, word


def _create(n_points, n_coords, points, coords, values, K, n=None, out="handle"):
    lib = bnmtf_amd.lib()
    h = C.c_void_p(12345)
    rc = lib.bnmtf_kmeans_create_list(n_points, n_coords, C.c_uint64(len(points) if n is None else n),
                                      None if points is None else _lib.ptr(points), None if coords is None else _lib.ptr(coords),
                                      None if values is None else _lib.ptr(values), K, 0, C.byref(h) if out == "handle" else None)
    return rc, h.value, lib.bnmtf_last_error().decode()


def test_create_list_refuses_before_any_device_call():
    """Every refusal is BNMTF_EINVAL with *out null (where there is no GPU a create that reached the device would answer
    BNMTF_EHIP instead)."""
    M = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 1]])
    p, c, v, _ = entries(np.arange(12.0).reshape(4, 3), M)

    def refused(text, *a, **kw):
        rc, h, msg = _create(*a, **kw)
        assert rc == EINVAL and h is None and text in msg, (rc, h, msg)

    refused("null argument", 4, 3, None, c, v, 2, n=len(c))
    refused("null argument", 4, 3, p, None, v, 2)
    refused("null argument", 4, 3, p, c, None, 2)
    rc, h, msg = _create(4, 3, p, c, v, 2, out=None)
    assert rc == EINVAL and "null argument" in msg
    refused("unsupported shape n_points=0 n_coords=3", 0, 3, p, c, v, 2)
    refused("unsupported shape n_points=4 n_coords=-1", 4, -1, p, c, v, 2)
    refused("unsupported K=0", 4, 3, p, c, v, 0)
    refused("unsupported K=1025", 4, 3, p, c, v, 1025)
    refused("at most 2^31 - 1 entries (n=2147483648)", 4, 3, p, c, v, 2, n=2 ** 31)
    p2 = p.copy(); p2[2] = 4
    refused("entry 2 (4, %d) lies outside the 4 x 3 matrix" % c[2], 4, 3, p2, c, v, 2)
    p2 = p.copy(); p2[0] = -1
    refused("lies outside", 4, 3, p2, c, v, 2)
    c2 = c.copy(); c2[1] = 3
    refused("entry 1 (%d, 3) lies outside the 4 x 3 matrix" % p[1], 4, 3, p, c2, v, 2)
    c2 = c.copy(); c2[1] = -1
    refused("lies outside", 4, 3, p, c2, v, 2)
    refused("the entry (%d, %d) occurs twice" % (p[3], c[3]), 4, 3, np.append(p, p[3]).astype(np.int32), np.append(c, c[3]).astype(np.int32), np.append(v, 1.0), 2)
    # a well-formed list gets as far as the device: a handle where there is one, BNMTF_EHIP where there is none
    rc, h, msg = _create(4, 3, p, c, v, 2)
    if rc == 0:
        bnmtf_amd.lib().bnmtf_kmeans_destroy(C.c_void_p(h))
    else:
        assert rc == -2 and h is None, (rc, h, msg)


# ------------------------------------------------------------------ the host builder
def _build(n_points, n_coords, points, coords, values):
    n = len(points)
    out = dict(point_ptr=np.full(n_points + 1, 7, np.uint32), point_coord=np.full(n, 7, np.uint32), point_val=np.full(n, 7.0),
               coord_ptr=np.full(n_coords + 1, 7, np.uint32), coord_point=np.full(n, 7, np.uint32), coord_val=np.full(n, 7.0),
               point_to_coord=np.full(n, 7, np.uint32))
    _lib.check(bnmtf_amd.lib().bnmtf_kmeans_build_lists(n_points, n_coords, C.c_uint64(n), _lib.ptr(points), _lib.ptr(coords), _lib.ptr(values),
                                                        *[_lib.ptr(out[k]) for k in ("point_ptr", "point_coord", "point_val", "coord_ptr", "coord_point",
                                                                                     "coord_val", "point_to_coord")]))
    return out


def _builder_inputs():
    rs = np.random.RandomState(5)
    n, d = 23, 140
    M = (rs.random_sample((n, d)) < 0.15).astype(np.uint8)
    M[0] = 0; M[0, 77] = 1                                  # a point with one entry
    M[1] = 0; M[1, [5, 69, 133]] = 1                        # a point whose entries share lane 5
    M[2] = 0; M[2, :129] = 1                                # the first 129 coordinates of a point (less the two below)
    M[:, 9] = 0; M[[3, 11, 19], 9] = 1                      # a coordinate whose entries all lie in point group 3
    M[:, 64] = 0                                            # an empty coordinate
    M2 = np.ones((3, 129), np.uint8)                        # full rows of 129
    return [(M, rs), (M2, rs), (np.ones((1, 1), np.uint8), rs), (np.eye(5, dtype=np.uint8), None)]


@pytest.mark.parametrize("which", range(4))
def test_the_host_builder_orders_both_lists_and_ties_them(which):
    M, rs = _builder_inputs()[which]
    n_points, n_coords = M.shape
    X = np.random.RandomState(6).randn(n_points, n_coords)
    p, c, v, n = entries(X, M, rs)                          # shuffled
    o = _build(n_points, n_coords, p, c, v)
    by_point = np.lexsort((c, c & 63, p))                   # keys (point, coord & 63, coord): the last key is the primary one
    by_coord = np.lexsort((p, p & 3, c))                    # keys (coord, point & 3, point)
    assert np.array_equal(o["point_coord"], c[by_point]) and np.array_equal(o["point_val"], v[by_point])
    assert np.array_equal(o["coord_point"], p[by_coord]) and np.array_equal(o["coord_val"], v[by_coord])
    assert np.array_equal(o["point_ptr"], np.concatenate(([0], np.cumsum(np.bincount(p, minlength=n_points)))))
    assert np.array_equal(o["coord_ptr"], np.concatenate(([0], np.cumsum(np.bincount(c, minlength=n_coords)))))
    # the permutation: one to one, and the entry at place t of the point list is the one at place point_to_coord[t] of the other
    q = o["point_to_coord"].astype(np.int64)
    assert np.array_equal(np.sort(q), np.arange(n))
    assert np.array_equal(o["coord_point"][q], p[by_point]) and np.array_equal(o["coord_val"][q], o["point_val"])
    coord_of_place = np.repeat(np.arange(n_coords), np.diff(o["coord_ptr"].astype(np.int64)))
    assert np.array_equal(coord_of_place[q], o["point_coord"])
    if which == 0:                                          # what the input is about
        ptr = o["point_ptr"]
        assert ptr[1] - ptr[0] == 1 and o["point_coord"][ptr[1]:ptr[2]].tolist() == [5, 69, 133]
        cp = o["coord_ptr"]
        assert o["coord_point"][cp[9]:cp[10]].tolist() == [3, 11, 19] and cp[65] == cp[64]
        row = o["point_coord"][ptr[2]:ptr[3]]
        assert len(row) == 127 and row[:3].tolist() == [0, 128, 1]            # lane 0 first: its strides 0 and 2 (64 is empty)
    # null outputs are skipped; the refusals are the create's
    lib = bnmtf_amd.lib()
    assert lib.bnmtf_kmeans_build_lists(n_points, n_coords, C.c_uint64(n), _lib.ptr(p), _lib.ptr(c), _lib.ptr(v), *([None] * 7)) == 0
    assert lib.bnmtf_kmeans_build_lists(n_points, n_coords, C.c_uint64(n), None, _lib.ptr(c), _lib.ptr(v), *([None] * 7)) == EINVAL
    c2 = c.copy(); c2[0] = n_coords
    assert lib.bnmtf_kmeans_build_lists(n_points, n_coords, C.c_uint64(n), _lib.ptr(p), _lib.ptr(c2), _lib.ptr(v), *([None] * 7)) == EINVAL
    assert "lies outside" in lib.bnmtf_last_error().decode()


def test_the_host_builder_takes_no_entries_at_all():
    p = np.zeros(1, np.int32); v = np.zeros(1)
    ptr, cptr = np.full(4, 7, np.uint32), np.full(3, 7, np.uint32)
    assert bnmtf_amd.lib().bnmtf_kmeans_build_lists(3, 2, C.c_uint64(0), _lib.ptr(p), _lib.ptr(p), _lib.ptr(v), _lib.ptr(ptr), None, None,
                                                    _lib.ptr(cptr), None, None, None) == 0
    assert not ptr.any() and not cptr.any()


# ------------------------------------------------------------------ the cases of the GPU tests
def test_every_named_situation_occurs_in_its_case():
    assert sorted((c.n, c.d, c.K) for c in CASES) == [(5, 140, 40), (9, 129, 41), (257, 129, 81)]
    lanes = by_name("lanes")
    assert [np.flatnonzero(lanes.M[p]).tolist() for p in range(5)] == [[0], [63], [64], [lanes.d - 1], [5, 69, 133]]
    a, dist = assign_reference(lanes.X, lanes.M, lanes.C, lanes.Mc)
    assert {p: (int(a[p]), float(dist[p])) for p in range(5)} == lanes.expect
    assert len({c for c, _ in lanes.expect.values()}) == 5
    full = by_name("full_point")
    assert full.d == 129 and full.M[0].all() and 0 < full.M[1:].mean() < 0.2
    assert len(full.sums) == 2 and (full.sums[1] == 40).all()                    # the one cluster of the second pass
    sp = by_name("sparse")
    assert 0.02 < sp.M.mean() < 0.04
    assert not sp.M[2].any() and sp.expect[2] == (sp.K - 1, INF)
    a, dist = assign_reference(sp.X, sp.M, sp.C, sp.Mc)
    assert a[2] == sp.K - 1 and dist[2] == INF
    assert not sp.M[:, 64].any() and sp.M[:, 63].any() and sp.M[:, 65].any()
    members = np.flatnonzero(sp.M[:, 7])
    assert len(members) == 3 and (members % 4 == 2).all()
    assert sp.new_row is not None and sp.M[sp.n - 1].sum() >= 3 and not sp.M[sp.n - 1, 64]
    changed = (sp.X_after() != sp.X) & (sp.M != 0)
    assert changed[sp.n - 1].any() and not changed[:sp.n - 1].any()
    assert {int(s) for s in sp.sums[1]} == {39, 40, 79, 80}
    for c in CASES:                                         # integers throughout: the reference is exact
        assert np.array_equal(c.X, np.rint(c.X)) and np.abs(c.X).max() <= 6 and np.array_equal(c.C, np.rint(c.C)) and np.abs(c.C).max() <= 7


# ------------------------------------------------------------------ the model classes
class _Stop(Exception):
    pass


def _spy(monkeypatch):
    seen = []

    def init(self, X, M, K, resolve_empty='singleton', **kw):
        seen.append(kw.get("layout", "nothing"))
        self._dh = None
        self._shape = (np.shape(X)[0], K)
        if len(seen) == 2:                                  # F's and G's: enough
            raise _Stop()

    def cluster(self):
        self.clustering_results = np.zeros(self._shape)

    monkeypatch.setattr(KMeans, "__init__", init)
    monkeypatch.setattr(KMeans, "initialise", lambda self, seed=None: None)
    monkeypatch.setattr(KMeans, "cluster", cluster)
    return seen


PRIORS = dict(alpha=1.0, beta=1.0, lambdaF=1.0, lambdaS=1.0, lambdaG=1.0)
PAIRS = [
    ("bnmtf_gibbs_optimised", lambda R, M, **kw: bnmtf_amd.bnmtf_gibbs_optimised(R, M, 2, 3, PRIORS, verbose=False, **kw), dict(layout='observed')),
    ("nmtf_icm", lambda R, M, **kw: bnmtf_amd.nmtf_icm(R, M, 2, 3, PRIORS, verbose=False, **kw), dict(layout='observed')),
    ("bnmtf_vb", lambda R, M, **kw: (bnmtf_amd.bnmtf_vb_observed if kw else bnmtf_amd.bnmtf_vb_optimised)(R, M, 2, 3, PRIORS, verbose=False), dict(observed=True)),
    ("NMTF", lambda R, M, **kw: bnmtf_amd.NMTF(R, M, 2, 3, verbose=False, **kw), dict(layout='observed')),
]


@pytest.mark.parametrize("name,make,observed", PAIRS, ids=[p[0] for p in PAIRS])
def test_the_observed_classes_cluster_on_lists_and_the_dense_ones_as_before(monkeypatch, name, make, observed):
    seen = _spy(monkeypatch)
    R = np.arange(1.0, 31.0).reshape(6, 5); M = np.ones((6, 5))
    for kw, want in ((observed, [("observed",), ("observed",)]), ({}, [("dense", "nothing"), ("dense", "nothing")])):
        del seen[:]
        m = make(R, M, **kw)
        with pytest.raises(_Stop):
            m.initialise('random', 'kmeans')
        assert len(seen) == 2 and all(s in w for s, w in zip(seen, want)), (name, kw, seen)
    assert kmeans_module.KMeans is KMeans


# ------------------------------------------------------------------ resources and the sanitizer
def test_the_new_kernels_compile_for_gfx950_without_spills_or_scratch():
    """kernel_kmeans.hip: the two dense kernels and the three list kernels without spills and without scratch; the list assignment --
    eight clusters' sums and overlaps in registers -- within 128 VGPRs, four waves per SIMD; the list sums takes the dense kernel's
    dynamic LDS and no static LDS."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_kmeans.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in (out.stdout + out.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    kernels = ("kmeans_assign_kernel", "kmeans_sums_kernel", "kmeans_assign_list_kernel", "kmeans_sums_list_kernel", "kmeans_set_row_list_kernel")
    assert len(found) == len(kernels), sorted(found)
    for kernel in kernels:
        hits = [r for n, r in found.items() if kernel in n]
        assert len(hits) == 1, (kernel, sorted(found))
        r = hits[0]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4 and r["LDS Size [bytes/block]"] == 0, (kernel, r)


def test_the_kmeans_entry_points_run_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_kmeans.cpp: a stand-alone program (its own main, the HIP stub as it is) over kernel_kmeans.hip's host
    code compiled with -fsanitize=address,undefined by `make asan_kmeans`, started as an ordinary child process."""
    exe = os.path.join(CSRC, "build", "san", "driver_kmeans_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_kmeans"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver kmeans: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
