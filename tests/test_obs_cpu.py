"""Host side of layout='observed' (DESIGN.md section 2.7): the keyword's place on the two classes, what the layout refuses --
before any device call --, the new entry points in the header, the exports map and the binding, and the library's host list
builder (bnmtf_obs_build_lists: the first half of bnmtf_obs_create) with what it refuses.
No GPU needed."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, _observed, bnmf_gibbs_optimised, bnmf_vb_optimised, nmf_icm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
I, J = 6, 5
NEW = ("bnmtf_obs_create", "bnmtf_obs_build_lists", "bnmf_obs_set_state", "bnmf_obs_get_state", "bnmf_obs_run", "bnmf_obs_cond_params", "bnmf_obs_metric_sums")


def _models(K=2, **kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    return [cls(R, M, K, PRI, verbose=False, layout='observed', **kw) for cls in (bnmf_gibbs_optimised, nmf_icm)]


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def test_layout_is_keyword_only_with_dense_as_default():
    for cls in (bnmf_gibbs_optimised, nmf_icm):
        p = inspect.signature(cls.__init__).parameters["layout"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 'dense', cls.__name__
    R = np.ones((I, J)); M = np.ones((I, J))
    assert bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False)._layout == 'dense'
    assert bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False, layout='observed')._layout == 'observed'
    # the variational class has no such layout
    with pytest.raises(TypeError):
        bnmf_vb_optimised(R, M, 2, PRI, verbose=False, layout='observed')


def test_an_unknown_layout_is_rejected(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for cls in (bnmf_gibbs_optimised, nmf_icm):
        with pytest.raises(AssertionError) as e:
            cls(R, M, 2, PRI, verbose=False, layout='bogus')
        assert str(e.value) == "Unknown layout: bogus. Should be 'dense' or 'observed'."


def test_a_sharded_model_is_refused_at_construction(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for cls in (bnmf_gibbs_optimised, nmf_icm):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            cls(R, M, 2, PRI, verbose=False, layout='observed', rank=0, world=2, comm_id=bytes(128))
        assert "layout='observed'" in str(e.value) and "world = 1" in str(e.value)


def test_a_rank_above_256_is_refused_and_256_runs_on_one_handle(no_device):
    R = np.ones((300, 290)); M = np.ones((300, 290))
    for cls in (bnmf_gibbs_optimised, nmf_icm):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            cls(R, M, 257, PRI, verbose=False, layout='observed')
        assert "K = 257" in str(e.value) and "K <= 256" in str(e.value) and "layout='observed'" in str(e.value)
        m = cls(R, M, 256, PRI, verbose=False, layout='observed')
        assert m._blocks is None                   # no column blocks: nothing ties a rank to a lane
        assert cls(R, M, 256, PRI, verbose=False)._blocks is not None


def test_M_test_and_expectation_are_refused_before_any_device_call(no_device):
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    g, icm = _models()
    for m in (g, icm):
        m.U = np.ones((I, 2)); m.V = np.ones((J, 2)); m.tau = 1.0
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Mt)
        assert "M_test" in str(e.value) and "layout='observed'" in str(e.value)
        assert not hasattr(m, "all_performances_test")
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        g.run(4, expectation=(1, 1))
    assert "expectation" in str(e.value) and "layout='observed'" in str(e.value)


def test_the_dense_layouts_switches_are_refused(no_device):
    for m in _models():
        for call, name in ((lambda: m.set_sweep_path(False), "set_sweep_path"), (lambda: m.set_small_path(False), "set_small_path"),
                           (lambda: m.set_profiling(True), "set_profiling")):
            with pytest.raises(bnmtf_amd.BnmtfError) as e:
                call()
            assert name in str(e.value) and "layout='observed'" in str(e.value)
        assert m.is_small() is False


def test_run_many_refuses_an_observed_model(no_device):
    g = _models()[0]
    g.U = np.ones((I, 2)); g.V = np.ones((J, 2)); g.tau = 1.0
    d = bnmf_gibbs_optimised(g.R, g.M, 2, PRI, verbose=False)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([d, g], 3)
    assert "layout='observed'" in str(e.value) and "model 1" in str(e.value)
    # (what the batched pools call for each of their models)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        g._run_prepare(3, True, None)
    assert "run_many" in str(e.value)


def test_header_exports_map_and_binding_list_the_same_new_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmt?f_obs_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(NEW)
    assert {n for n in _lib.EXPORTS if "_obs_" in n} == set(NEW)
    emap = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    for n in NEW:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    assert re.search(r"^#define BNMTF_OBS_MAX_RANK 256$", hdr, flags=re.M) and _observed.MAX_RANK == 256
    # a null handle or null argument is an error code, not a crash (function-try-block guard and argument checks)
    assert lib.bnmtf_obs_create(3, 3, 2, 1, None, None, None, None, None, 1.0, 1.0, 0, 0, None) == -1
    assert lib.bnmf_obs_set_state(None, None, None, 1.0) == -1
    assert lib.bnmf_obs_get_state(None, None, None, None) == -1
    assert lib.bnmf_obs_run(None, 1, 0, None, None, None, None, None) == -1
    assert lib.bnmf_obs_cond_params(None, 0, 0, None, None) == -1
    assert lib.bnmf_obs_metric_sums(None, 1, None, None, None, None, None, None) == -1
    assert b"bnmtf_obs_create" in lib.bnmtf_last_error()


def _entries(M, R=None, seed=0):
    """The entries of the mask M in a seeded random order (the library sorts), with values that tell them apart."""
    M = np.asarray(M)
    rows, cols = np.nonzero(M)
    R = (np.arange(M.size, dtype=np.float32).reshape(M.shape) + 0.5) if R is None else R
    order = np.random.RandomState(seed).permutation(len(rows))
    return rows[order].astype(np.int32), cols[order].astype(np.int32), R[rows, cols][order].astype(np.float32), R


def _check_lists(M, seed=0):
    """bnmtf_obs_build_lists -- the host half of bnmtf_obs_create -- on the entries of M handed over in random order: pointers,
    ascending inner indices and the values beside them, for the row list and for the column list."""
    M = np.asarray(M)
    n_i, n_j = M.shape
    rows, cols, vals, R = _entries(M, seed=seed)
    L = _observed.build_lists(n_i, n_j, rows, cols, vals)
    assert L["row_ptr"].dtype == np.uint32 and L["col_ptr"].dtype == np.uint32
    assert L["row_ptr"][0] == 0 and L["col_ptr"][0] == 0 and L["row_ptr"][-1] == L["col_ptr"][-1] == int((M != 0).sum())
    assert np.array_equal(np.diff(L["row_ptr"].astype(np.int64)), (M != 0).sum(axis=1)) and np.array_equal(np.diff(L["col_ptr"].astype(np.int64)), (M != 0).sum(axis=0))
    for i in range(n_i):
        sl = slice(L["row_ptr"][i], L["row_ptr"][i + 1])
        assert np.array_equal(L["row_col"][sl], np.flatnonzero(M[i])) and np.array_equal(L["row_val"][sl], R[i, np.flatnonzero(M[i])])
    for j in range(n_j):
        sl = slice(L["col_ptr"][j], L["col_ptr"][j + 1])
        assert np.array_equal(L["col_row"][sl], np.flatnonzero(M[:, j])) and np.array_equal(L["col_val"][sl], R[np.flatnonzero(M[:, j]), j])
    return L


def test_the_list_builder_on_a_ragged_mask_a_single_entry_and_a_full_matrix():
    ragged = np.array([[1, 0, 0, 1, 1], [0, 1, 0, 0, 0], [0, 1, 1, 0, 0], [1, 1, 0, 1, 1]])      # rows of 3, 1, 2, 4 entries, columns of 2, 3, 1, 2, 2
    for seed in range(4):
        L = _check_lists(ragged, seed)
        assert list(L["row_ptr"]) == [0, 3, 4, 6, 10] and list(L["col_ptr"]) == [0, 2, 5, 6, 8, 10]
        assert list(L["row_col"]) == [0, 3, 4, 1, 1, 2, 0, 1, 3, 4] and list(L["col_row"]) == [0, 3, 1, 2, 3, 2, 0, 3, 0, 3]
    L = _check_lists(np.ones((1, 1)))
    assert list(L["row_ptr"]) == [0, 1] and list(L["col_ptr"]) == [0, 1] and list(L["row_col"]) == [0] and list(L["col_row"]) == [0] and list(L["row_val"]) == [0.5]
    L = _check_lists(np.ones((4, 3)))
    assert list(L["row_ptr"]) == [0, 3, 6, 9, 12] and list(L["col_ptr"]) == [0, 4, 8, 12]
    assert list(L["row_col"]) == [0, 1, 2] * 4 and list(L["col_row"]) == [0, 1, 2, 3] * 3
    rs = np.random.RandomState(3)
    M = rs.rand(37, 29) < 0.15
    M[np.arange(37), rs.randint(0, 29, 37)] = True; M[rs.randint(0, 37, 29), np.arange(29)] = True
    _check_lists(M, 5)


def _refused(call):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        _lib.check(call())
    return str(e.value)


def test_what_the_builder_and_create_refuse_before_any_device_call():
    """An entry outside the matrix, an entry twice, a row or a column without entries, no entries at all: refused by
    bnmtf_obs_build_lists and -- with the same message, ahead of its first device call -- by bnmtf_obs_create."""
    lib = bnmtf_amd.lib()
    M = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 1]])
    rows, cols, vals, _ = _entries(M, seed=1)
    I, J, K = M.shape[0], M.shape[1], 2
    lam_r, lam_c = np.ones((I, K)), np.ones((J, K))
    h = C.c_void_p()

    def both(r, c, v, n=None):
        n = len(r) if n is None else n
        r, c, v = np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float32)
        a = _refused(lambda: lib.bnmtf_obs_build_lists(I, J, n, _lib.ptr(r), _lib.ptr(c), _lib.ptr(v), None, None, None, None, None, None))
        b = _refused(lambda: lib.bnmtf_obs_create(I, J, K, n, _lib.ptr(r), _lib.ptr(c), _lib.ptr(v), _lib.ptr(lam_r), _lib.ptr(lam_c), 1.0, 1.0, 7, 0, C.byref(h)))
        assert a == b and h.value is None and "error -1" in a
        return a

    assert lib.bnmtf_obs_build_lists(I, J, len(rows), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), None, None, None, None, None, None) == 0
    for bad_r, bad_c in ((I, 0), (-1, 0), (0, J), (0, -1)):
        r, c = rows.copy(), cols.copy(); r[2], c[2] = bad_r, bad_c
        assert "entry 2 (%d, %d) lies outside the 4 x 3 matrix" % (bad_r, bad_c) in both(r, c, vals)
    r, c = np.append(rows, rows[4]), np.append(cols, cols[4])
    assert "the entry (%d, %d) occurs twice" % (rows[4], cols[4]) in both(r, c, np.append(vals, 9.0))
    keep = rows != 1
    assert "Fully unobserved row in R, row 1." in both(rows[keep], cols[keep], vals[keep])
    keep = cols != 0
    assert "Fully unobserved column in R, column 0." in both(rows[keep], cols[keep], vals[keep])
    assert "between 1 and 2^31 - 1 entries (n=0)" in both(rows, cols, vals, n=0)
    # K beyond one handle's ranks, null lists: create's own checks
    assert "K=257" in _refused(lambda: lib.bnmtf_obs_create(I, J, 257, len(rows), _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(np.ones((I, 257))), _lib.ptr(np.ones((J, 257))), 1.0, 1.0, 7, 0, C.byref(h)))
    assert "null argument" in _refused(lambda: lib.bnmtf_obs_build_lists(I, J, 3, None, None, None, None, None, None, None, None, None))


def test_entry_list_is_row_major_with_fp32_values():
    R = np.arange(12.0).reshape(3, 4) + 0.5
    Mk = np.array([[0, 1, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0]])
    rows, cols, vals = _observed.entry_list(R, Mk)
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and vals.dtype == np.float32
    assert list(rows) == [0, 0, 2] and list(cols) == [1, 3, 0] and list(vals) == [1.5, 3.5, 8.5]
    assert all(a.flags["C_CONTIGUOUS"] for a in (rows, cols, vals))
