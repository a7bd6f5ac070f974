"""Host side of list input and held-out curves on the observed-entry layout: bnmtf_amd.Entries, the three
classes on the two-factor handle built from one, what they and the other classes refuse -- before any device call --, host memory
that follows the number of entries, the entry point bnmtf_set_heldout_entries in the header, the exports map and the binding, the
resources of the new kernel and a sanitizer run of the new host code through a stand-alone program.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
import tracemalloc

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, Entries, _lib, _observed, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, nmf_icm, nmtf_icm)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = "bnmtf_set_heldout_entries"
# the three classes on the two-factor handle, from either form of input
MAKERS = ((lambda R, M, **kw: bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False, layout='observed', **kw)),
          (lambda R, M, **kw: nmf_icm(R, M, 2, PRI, verbose=False, layout='observed', **kw)),
          (lambda R, M, **kw: bnmf_vb_observed(R, M, 2, PRI, verbose=False, **kw)))


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def _dense(seed=0, shape=(I, J), share=0.5):
    """R, M with no empty row or column"""
    rs = np.random.RandomState(seed)
    n_i, n_j = shape
    M = (rs.rand(n_i, n_j) < share).astype(float)
    M[np.arange(n_i), np.arange(n_i) % n_j] = 1; M[np.arange(n_j) % n_i, np.arange(n_j)] = 1
    return rs.rand(n_i, n_j) * 3 + 0.1, M


def _with_state(m):
    """a state by hand: initialise() would ask the device for beta_s"""
    if isinstance(m, bnmf_vb_observed):
        for n in ("muU", "tauU", "expU", "varU"):
            setattr(m, n, np.ones((m.I, m.K)))
        for n in ("muV", "tauV", "expV", "varV"):
            setattr(m, n, np.ones((m.J, m.K)))
        m.exptau = 1.0
    else:
        m.U = np.ones((m.I, m.K)); m.V = np.ones((m.J, m.K)); m.tau = 1.0
    return m


# ---------------------------------------------------------------- Entries
def test_entries_keeps_contiguous_int32_lists_and_fp64_values():
    E = Entries((4, 3), [3, 0, 2], np.array([0, 2, 1], dtype=np.int64), [1.5, 2, 3])
    assert E.shape == (4, 3) and len(E) == 3
    assert E.rows.dtype == np.int32 and E.cols.dtype == np.int32 and E.values.dtype == np.float64
    assert all(a.flags["C_CONTIGUOUS"] for a in (E.rows, E.cols, E.values))
    assert list(E.rows) == [3, 0, 2] and list(E.cols) == [0, 2, 1] and list(E.values) == [1.5, 2.0, 3.0]
    assert len(Entries((4, 3), [], [], [])) == 0
    assert bnmtf_amd.Entries is Entries and "Entries" in bnmtf_amd.__all__ and bnmtf_amd.entries.Entries is Entries


@pytest.mark.parametrize("args, text", [
    (((4, 3), [[0, 1]], [[0, 1]], [[1., 2.]]), "one-dimensional"),
    (((4, 3), [0, 1], [0, 1], [[1., 2.]]), "one-dimensional"),
    (((4, 3), [0, 1], [0], [1., 2.]), "different lengths: 2, 1 and 2"),
    (((4, 3), [0, 1], [0, 1], [1.]), "different lengths: 2, 2 and 1"),
    (((4, 3), [0, 4], [0, 1], [1., 2.]), "entry 1 (4, 1) lies outside the 4 x 3 matrix"),
    (((4, 3), [0, -1], [0, 1], [1., 2.]), "entry 1 (-1, 1) lies outside the 4 x 3 matrix"),
    (((4, 3), [0, 1], [3, 1], [1., 2.]), "entry 0 (0, 3) lies outside the 4 x 3 matrix"),
    (((4, 3), [0, 1], [0, -2], [1., 2.]), "entry 1 (1, -2) lies outside the 4 x 3 matrix"),
    (((4, 3), [0, 1], [0, 1], [1., np.nan]), "the value of entry 1 (1, 1) is not finite"),
    (((4, 3), [0, 1], [0, 1], [np.inf, 1.]), "the value of entry 0 (0, 0) is not finite"),
    (((4, 3), [0.5, 1], [0, 1], [1., 2.]), "rows holds integers"),
    (((4, 3, 2), [0], [0], [1.]), "shape is (I, J)"),
    (((0, 3), [], [], []), "shape is (I, J)"),
    ((4, [0], [0], [1.]), "shape is (I, J)"),
])
def test_entries_refuses_what_is_no_list_of_entries(args, text):
    with pytest.raises(ValueError) as e:
        Entries(*args)
    assert text in str(e.value)


def test_from_dense_is_entry_list_and_to_dense_and_counts_go_back():
    R, M = _dense(3, (37, 29), 0.2)
    R[5, 7] = 1.0 + 2.0 ** -30                       # (a value that fp32 rounds: the lists carry the same bits)
    M[5, 7] = 1
    E = Entries.from_dense(R, M)
    rows, cols, vals = _observed.entry_list(R, M)
    assert np.array_equal(E.rows, rows) and np.array_equal(E.cols, cols) and E.rows.dtype == rows.dtype
    assert np.array_equal(E.values, R[M != 0]) and E.values.dtype == np.float64
    v32 = E.values32()
    assert v32.dtype == np.float32 and v32.tobytes() == vals.tobytes()
    R2, M2 = E.to_dense()
    assert np.array_equal(M2, M) and np.array_equal(R2, R * M) and R2.dtype == np.float64
    n, per_row, per_col = E.counts()
    assert n == int(M.sum()) and per_row.dtype == np.uint32 and per_col.dtype == np.uint32
    assert np.array_equal(per_row, M.sum(axis=1)) and np.array_equal(per_col, M.sum(axis=0))
    # a shuffled list is the same matrix
    order = np.random.RandomState(1).permutation(len(E))
    S = Entries(E.shape, E.rows[order], E.cols[order], E.values[order])
    assert all(np.array_equal(a, b) for a, b in zip(S.to_dense(), (R2, M2))) and all(np.array_equal(a, b) for a, b in zip(S.counts()[1:], (per_row, per_col)))
    with pytest.raises(ValueError):
        Entries.from_dense(R, M[:, :-1])


# ---------------------------------------------------------------- the three classes
def test_the_three_classes_are_built_from_entries_with_the_same_attributes(no_device):
    R, M = _dense(0)
    E = Entries.from_dense(R, M)
    for make in MAKERS:
        d, m = make(R, M), make(E, None)
        assert sorted(vars(m)) == sorted(vars(d)), type(m).__name__
        assert m.R is E and m.M is None and m._layout == 'observed' and m._h is None
        assert (m.I, m.J, m.K) == (d.I, d.J, d.K) == (I, J, 2)
        assert m.size_Omega == d.size_Omega == len(E) == M.sum()
        for a, b in zip(m.omega_counts(), d.omega_counts()):
            assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype
        assert np.array_equal(m.lambdaU, d.lambdaU) and np.array_equal(m.lambdaV, d.lambdaV)
        # what becomes the handle's lists: the same bits from either form, and from a list in any order
        order = np.random.RandomState(2).permutation(len(E))
        s = make(Entries(E.shape, E.rows[order], E.cols[order], E.values[order]), None)
        for x in (m, s):
            for a, b in zip(_observed.entries_of(x), _observed.entries_of(d)):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes() and a.flags["C_CONTIGUOUS"]


def test_an_empty_row_or_column_keeps_check_R_Ms_text(no_device):
    R, M = _dense(0)
    for make in MAKERS:
        for axis, text in ((0, "Fully unobserved row in R, row 4."), (1, "Fully unobserved column in R, column 2.")):
            Mx = M.copy()
            if axis == 0:
                Mx[4] = 0
            else:
                Mx[:, 2] = 0
            texts = []
            for args in ((R, Mx), (Entries.from_dense(R, Mx), None)):
                with pytest.raises(AssertionError) as e:
                    make(*args)
                texts.append(str(e.value))
            assert texts == [text, text]


def test_entries_with_the_dense_layout_or_with_a_mask_are_refused(no_device):
    R, M = _dense(0)
    E = Entries.from_dense(R, M)
    for cls in (bnmf_gibbs_optimised, nmf_icm):
        for kw in ({}, {"layout": 'dense'}):
            with pytest.raises(bnmtf_amd.BnmtfError) as e:
                cls(E, None, 2, PRI, verbose=False, **kw)
            assert "layout='observed'" in str(e.value) and "Entries" in str(e.value) and cls.__name__ in str(e.value)
    for make in MAKERS:
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            make(E, M)
        assert "M must be None" in str(e.value)


def test_the_classes_out_of_scope_refuse_entries_and_name_the_limit(no_device):
    R, M = _dense(0)
    E = Entries.from_dense(R, M)
    five = ((bnmtf_gibbs_optimised, lambda: bnmtf_gibbs_optimised(E, None, 2, 2, PRI3, verbose=False, layout='observed')),
            (nmtf_icm, lambda: nmtf_icm(E, None, 2, 2, PRI3, verbose=False, layout='observed')),
            (bnmtf_vb_observed, lambda: bnmtf_vb_observed(E, None, 2, 2, PRI3, verbose=False)),
            (NMF, lambda: NMF(E, None, 2, verbose=False, layout='observed')),
            (NMTF, lambda: NMTF(E, None, 2, 2, verbose=False, layout='observed')))
    for cls, make in five:
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            make()
        assert str(e.value).startswith(cls.__name__ + ":") and "Entries" in str(e.value) and "two-factor" in str(e.value)
        assert "bnmf_gibbs_optimised, nmf_icm, bnmf_vb_observed" in str(e.value)


def test_host_memory_follows_the_entries_not_the_matrix(no_device):
    """8 192 x 8 192 with 100 000 entries: construction and omega_counts() stay below I * J BYTES (67 MB) -- no array of the
    matrix's size, even at one byte per entry, can hide under that; the list with its copies is a few MB."""
    n_i = n_j = 8192
    rs = np.random.RandomState(0)
    flat = np.unique(np.concatenate([np.arange(n_i, dtype=np.int64) * n_j + np.arange(n_i), rs.randint(0, n_i * n_j, 100000 - n_i)]))
    rows, cols, vals = (flat // n_j).astype(np.int32), (flat % n_j).astype(np.int32), rs.rand(len(flat))
    for make in MAKERS:
        tracemalloc.start()
        try:
            E = Entries((n_i, n_j), rows, cols, vals)
            m = make(E, None)
            tot, per_row, per_col = m.omega_counts()
            lists = _observed.entries_of(m)
            _, peak = tracemalloc.get_traced_memory()
        finally:
            tracemalloc.stop()
        assert tot == len(flat) and per_row.min() >= 1 and per_col.min() >= 1 and len(lists[0]) == len(flat)
        assert peak < n_i * n_j, "%s: a peak of %d bytes" % (type(m).__name__, peak)


# ---------------------------------------------------------------- held-out and predict refusals
def test_a_dense_M_test_is_still_refused_and_now_points_to_entries(no_device):
    R, M = _dense(0)
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    for make in MAKERS:
        for args in ((R, M), (Entries.from_dense(R, M), None)):
            m = _with_state(make(*args))
            with pytest.raises(bnmtf_amd.BnmtfError) as e:
                m.run(2, M_test=Mt)
            assert "M_test" in str(e.value) and "layout='observed'" in str(e.value) and type(m).__name__ in str(e.value) and "Entries" in str(e.value)
            assert not hasattr(m, "all_performances_test")
    assert "Entries" in _observed.REFUSALS["run(M_test=)"]


def test_entries_as_M_test_of_the_wrong_shape_or_empty_are_refused(no_device):
    R, M = _dense(0)
    for make in MAKERS:
        m = _with_state(make(Entries.from_dense(R, M), None))
        with pytest.raises(AssertionError) as e:
            m.run(2, M_test=Entries((I, J + 1), [0], [0], [1.]))
        assert "M_test" in str(e.value) and "(6, 5) and (6, 6)" in str(e.value)
        with pytest.raises(AssertionError) as e:
            m.run(2, M_test=Entries((I, J), [], [], []))
        assert "M_test" in str(e.value) and "empty" in str(e.value)
        assert not hasattr(m, "all_performances_test")


def test_entries_as_M_test_on_the_dense_layout_and_the_other_classes_are_refused(no_device):
    R, M = _dense(0)
    Et = Entries((I, J), [1], [2], [1.])
    dense = [_with_state(bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False)), _with_state(nmf_icm(R, M, 2, PRI, verbose=False))]
    vb = bnmf_vb_optimised(R, M, 2, PRI, verbose=False)
    for m in dense + [vb]:
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Et)
        assert "M_test" in str(e.value) and "0/1 mask" in str(e.value) and "layout='observed'" in str(e.value)
    tri = [bnmtf_gibbs_optimised(R, M, 2, 2, PRI3, verbose=False, layout='observed'), nmtf_icm(R, M, 2, 2, PRI3, verbose=False, layout='observed')]
    for m in tri:
        m.F = np.ones((I, 2)); m.S = np.ones((2, 2)); m.G = np.ones((J, 2)); m.tau = 1.0
    nps = [NMF(R, M, 2, verbose=False, layout='observed'), NMTF(R, M, 2, 2, verbose=False, layout='observed')]
    nps[0].initialise('ones'); nps[1].initialise('ones', 'ones')
    for m in tri + nps:
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Et)
        assert "M_test" in str(e.value) and "layout='observed'" in str(e.value) and "two-factor" in str(e.value)


def test_a_model_built_from_entries_takes_M_pred_as_entries_only(no_device):
    R, M = _dense(0)
    Mp = np.zeros((I, J)); Mp[1, 2] = 1
    for make in MAKERS:
        m = _with_state(make(Entries.from_dense(R, M), None))
        call = (lambda: m.predict(Mp, 0, 1)) if type(m) is bnmf_gibbs_optimised else (lambda: m.predict(Mp))
        if type(m) is bnmf_gibbs_optimised:
            m.all_U, m.all_V, m.all_tau = np.ones((1, I, 2)), np.ones((1, J, 2)), np.ones(1)
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            call()
        assert "M_pred" in str(e.value) and "Entries" in str(e.value) and type(m).__name__ in str(e.value)
        # ... and either model an Entries of its own shape only
        d = _with_state(make(R, M))
        for model in (m, d):
            with pytest.raises(AssertionError) as e:
                _observed.entries_of(model, Entries((I + 1, J), [0], [0], [1.]), "M_pred")
            assert "M_pred" in str(e.value) and "(6, 5) and (7, 5)" in str(e.value)
        rows, cols, vals = _observed.entries_of(d, Entries((I, J), [5, 0], [4, 1], [2.5, 1.0 + 2.0 ** -30]), "M_pred")
        assert list(rows) == [0, 5] and list(cols) == [1, 4] and vals.dtype == np.float32 and list(vals) == [1.0, 2.5]      # (row major, fp32)


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_point():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(bnmtf_handle h, uint64_t n, const int32_t\* rows, const int32_t\* cols, const float\* values\);" % NEW, hdr, flags=re.M)
    assert NEW in _lib.EXPORTS and _lib._SIGS[NEW] == ([C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    assert any(fnmatch.fnmatchcase(NEW, g) for g in globs)
    lib = bnmtf_amd.lib()
    assert hasattr(lib, NEW), "libbnmtf_hip.so does not export %s" % NEW
    src = open(os.path.join(CSRC, "api_obs.inc")).read()
    assert re.search(r"^int %s\([^{]*?\) try \{" % NEW, src, flags=re.M | re.S)
    # a null handle is an error code, not a crash; the other refusals need a handle: the stand-alone program below walks them
    rows = np.zeros(1, dtype=np.int32); vals = np.ones(1, dtype=np.float32)
    assert lib.bnmtf_set_heldout_entries(None, 1, _lib.ptr(rows), _lib.ptr(rows), _lib.ptr(vals)) == -1
    assert b"bnmtf_set_heldout_entries: null handle" in lib.bnmtf_last_error()
    assert lib.bnmtf_set_heldout_entries(None, 0, None, None, None) == -1
    # the dense layout's call is what it was
    assert "bnmtf_set_heldout" in _lib.EXPORTS and "bnmtf_get_heldout" in _lib.EXPORTS


def test_the_new_kernel_compiles_for_gfx950_without_spills_or_scratch():
    """kernel_obs_heldout.hip: one kernel, no spills, no scratch, the four waves' factor rows as doubles and their six sums in LDS
    (4 x 256 x 8 + 4 x 6 x 8 bytes), within 128 VGPRs: four waves per SIMD."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_obs_heldout.hip"), "-o", os.devnull]
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
    assert len(found) == 1 and "obs_heldout_kernel" in list(found)[0], sorted(found)
    r = list(found.values())[0]
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, r
    assert r["LDS Size [bytes/block]"] <= 4 * 256 * 8 + 4 * 6 * 8, r


def test_the_entry_point_and_the_run_hooks_run_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_obs_heldout.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_obs_heldout` and started as an ordinary child process: set / replace / clear /
    run / get / destroy on a Gibbs and a variational handle, a build that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_obs_heldout_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_obs_heldout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver obs_heldout: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
