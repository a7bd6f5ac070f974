"""Host side of layout='observed' on the tri-factorisation classes: the keyword's place on
bnmtf_gibbs_optimised and nmtf_icm, what the layout refuses -- before any device call --, the new entry points in the header, the
exports map and the binding, and the resources of the new kernels.  No GPU needed."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, _observed, bnmtf_gibbs_optimised, nmtf_icm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = ("bnmtf_otri_create", "bnmtf_otri_set_state", "bnmtf_otri_get_state", "bnmtf_otri_run", "bnmtf_otri_cond_params", "bnmtf_otri_metric_sums")
CLASSES = (bnmtf_gibbs_optimised, nmtf_icm)


def _models(K=2, L=3, **kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    return [cls(R, M, K, L, PRI, verbose=False, layout='observed', **kw) for cls in CLASSES]


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def _state(m):
    m.F = np.ones((I, m.K)); m.S = np.ones((m.K, m.L)); m.G = np.ones((J, m.L)); m.tau = 1.0


def test_layout_is_keyword_only_with_dense_as_default():
    for cls in CLASSES:
        p = inspect.signature(cls.__init__).parameters["layout"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 'dense', cls.__name__
    R = np.ones((I, J)); M = np.ones((I, J))
    for cls in CLASSES:
        assert cls(R, M, 2, 3, PRI, verbose=False)._layout == 'dense'
        assert cls(R, M, 2, 3, PRI, verbose=False, layout='observed')._layout == 'observed'
    with pytest.raises(TypeError):
        bnmtf_gibbs_optimised(R, M, 2, 3, PRI, None, 0, True, 0, 1, None, 'observed')


def test_an_unknown_layout_is_rejected(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for cls in CLASSES:
        with pytest.raises(AssertionError) as e:
            cls(R, M, 2, 3, PRI, verbose=False, layout='bogus')
        assert str(e.value) == "Unknown layout: bogus. Should be 'dense' or 'observed'."


def test_ranks_above_32_are_refused_and_32_is_taken(no_device):
    R = np.ones((40, 41)); M = np.ones((40, 41))
    for cls in CLASSES:
        for K, L, name in ((33, 4, "K = 33"), (4, 33, "L = 33"), (64, 64, "K = 64"), (0, 3, "K = 0")):
            with pytest.raises(bnmtf_amd.BnmtfError) as e:
                cls(R, M, K, L, PRI, verbose=False, layout='observed')
            assert name in str(e.value) and "K, L <= 32" in str(e.value) and "layout='observed'" in str(e.value)
        m = cls(R, M, 32, 32, PRI, verbose=False, layout='observed')
        assert m._blocks is None and m._layout == 'observed'
        assert cls(R, M, 33, 4, PRI, verbose=False)._layout == 'dense'            # (the dense layout keeps its own limits)
    assert _observed.MAX_RANK_TRI == 32


def test_a_sharded_model_is_refused_at_construction(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for cls in CLASSES:
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            cls(R, M, 2, 3, PRI, verbose=False, layout='observed', rank=0, world=2, comm_id=bytes(128))
        assert "layout='observed'" in str(e.value) and "world = 1" in str(e.value)


def test_M_test_and_expectation_are_refused_before_any_device_call(no_device):
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    g, icm = _models()
    for m in (g, icm):
        _state(m)
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
        tot, row, col = m.omega_counts()
        assert tot == I * J and list(row) == [J] * I and list(col) == [I] * J


def test_run_many_and_the_pools_refuse_an_observed_model(no_device):
    g = _models()[0]
    _state(g)
    d = bnmtf_gibbs_optimised(g.R, g.M, 2, 3, PRI, verbose=False)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([d, g], 3)
    assert "layout='observed'" in str(e.value) and "model 1" in str(e.value)
    # (what the batched pools call for each of their models)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        g._run_prepare(3, True, None)
    assert "run_many" in str(e.value) and "layout='observed'" in str(e.value)


def test_header_exports_map_and_binding_list_the_same_new_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmt?f_otri_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(NEW)
    assert {n for n in _lib.EXPORTS if "_otri_" in n} == set(NEW)
    assert not [n for n in NEW if "_obs_" in n or "_vbo_" in n]
    every = re.findall(r"^BNMTF_API\s+[\w\s\*]+?\b(bnmt?f_\w+)\s*\(", hdr, flags=re.M)
    assert len(_lib.EXPORTS) == len(every) == len(set(every)), (len(_lib.EXPORTS), len(every))
    emap = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    for n in NEW:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    assert re.search(r"^#define BNMTF_OTRI_MAX_RANK 32$", hdr, flags=re.M)
    # every one is a function-try-block ending in the guard
    src = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "api_obs_tri.inc")).read()
    for n in NEW:
        assert re.search(r"^int %s\([^{]*?\) try \{" % n, src, flags=re.M | re.S), n
    assert src.count("} BNMTF_ABI_GUARD") == len(NEW)
    # a null handle or null argument is an error code, not a crash
    assert lib.bnmtf_otri_create(3, 3, 2, 2, 1, None, None, None, None, None, None, 1.0, 1.0, 0, 0, None) == -1
    assert b"bnmtf_otri_create" in lib.bnmtf_last_error()
    h = C.c_void_p()
    assert lib.bnmtf_otri_create(3, 3, 2, 2, 1, None, None, None, None, None, None, 1.0, 1.0, 0, 0, C.byref(h)) == -1 and h.value is None
    assert lib.bnmtf_otri_set_state(None, None, None, None, 1.0) == -1
    assert lib.bnmtf_otri_get_state(None, None, None, None, None) == -1
    assert lib.bnmtf_otri_run(None, 1, 0, None, None, None, None, None, None) == -1
    assert lib.bnmtf_otri_cond_params(None, 0, 0, 0, None, None) == -1
    assert lib.bnmtf_otri_metric_sums(None, 1, None, None, None, None, None, None, None) == -1
    assert b"bnmtf_otri_create" in lib.bnmtf_last_error()


def test_create_refuses_ranks_and_lists_before_any_device_call():
    """K or L outside 1 .. 32 and what bnmtf_obs_create refuses of the entries, with its messages: ahead of the first device call."""
    lib = bnmtf_amd.lib()
    M = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 1]])
    rows, cols, vals = _observed.entry_list(np.arange(12.0).reshape(4, 3), M)
    h = C.c_void_p()

    def refused(K, L, r, c, v, n=None):
        lam = np.ones(4 * 33 * 33)
        rc = lib.bnmtf_otri_create(4, 3, K, L, len(r) if n is None else n, _lib.ptr(r), _lib.ptr(c), _lib.ptr(v), _lib.ptr(lam), _lib.ptr(lam),
                                   _lib.ptr(lam), 1.0, 1.0, 7, 0, C.byref(h))
        assert rc == -1 and h.value is None
        return lib.bnmtf_last_error().decode()

    assert "K=33" in refused(33, 2, rows, cols, vals) and "L=33" in refused(2, 33, rows, cols, vals) and "L=0" in refused(2, 0, rows, cols, vals)
    keep = rows != 1
    assert "Fully unobserved row in R, row 1." in refused(2, 2, rows[keep].copy(), cols[keep].copy(), vals[keep].copy())
    r2 = rows.copy(); r2[2] = 4
    assert "lies outside the 4 x 3 matrix" in refused(2, 2, r2, cols, vals)
    assert "occurs twice" in refused(2, 2, np.append(rows, rows[3]).astype(np.int32), np.append(cols, cols[3]).astype(np.int32), np.append(vals, 1).astype(np.float32))
    assert "between 1 and 2^31 - 1 entries (n=0)" in refused(2, 2, rows, cols, vals, n=0)


def test_the_new_kernels_compile_for_gfx950_without_spills_or_scratch():
    """kernel_obs_tri.hip: the column-Gram kernel holds its 32 x 32 tile in two sets of 16 accumulators, two trips of rows and
    indices in flight and no LDS (95 VGPRs measured, four waves per SIMD), the effective-factor kernel
    three LDS tiles; neither spills or uses scratch."""
    csrc = os.path.join(ROOT, "bnmtf_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "kernel_obs_tri.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=900)
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
    for kernel in ("obs_tri_gram_kernel", "obs_tri_eff_kernel"):
        hits = [r for n, r in found.items() if kernel in n]
        assert len(hits) == 1, sorted(found)
        r = hits[0]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (kernel, r)
    assert [r for n, r in found.items() if "obs_tri_gram_kernel" in n][0]["LDS Size [bytes/block]"] == 0
