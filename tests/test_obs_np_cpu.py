"""Host side of layout='observed' on nmf_np.NMF and nmtf_np.NMTF: the keyword's place on the two classes,
what the layout refuses -- before any device call --, the six bnmtf_onp_* entry points in the header, the exports map and the
binding, what bnmtf_onp_create refuses, the resources of the new kernels and a sanitizer run of the new host code through a
stand-alone program.  No GPU needed."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import NMF, NMTF, _lib, _observed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
I, J = 6, 5
NEW = ("bnmtf_onp_create", "bnmtf_onp_set_state", "bnmtf_onp_get_state", "bnmtf_onp_run", "bnmtf_onp_update", "bnmtf_onp_metrics")
MAKERS = ((lambda R, M, **kw: NMF(R, M, 2, verbose=False, **kw)), (lambda R, M, **kw: NMTF(R, M, 2, 3, verbose=False, **kw)))


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def _models(**kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    out = [make(R, M, layout='observed', **kw) for make in MAKERS]
    out[0].initialise('ones'); out[1].initialise('ones', 'ones')
    return out


def test_layout_is_keyword_only_with_dense_as_default(no_device):
    for cls in (NMF, NMTF):
        p = inspect.signature(cls.__init__).parameters["layout"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 'dense', cls.__name__
    R = np.ones((I, J)); M = np.ones((I, J))
    for make in MAKERS:
        assert make(R, M)._layout == 'dense'
        assert make(R, M, layout='dense')._layout == 'dense'
        assert make(R, M, layout='observed')._layout == 'observed'


def test_an_unknown_layout_is_rejected(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for make in MAKERS:
        with pytest.raises(AssertionError) as e:
            make(R, M, layout='bogus')
        assert str(e.value) == "Unknown layout: bogus. Should be 'dense' or 'observed'."


def test_a_row_longer_than_the_dense_limit_is_constructed_and_fails_only_at_the_device(monkeypatch):
    """16 385 x 3: the dense layout's create refuses it ("at most 16384 entries"); the observed one has no such limit, so its run()
    gets as far as the library -- which this test takes away."""
    R = np.ones((16385, 3)); M = np.ones((16385, 3))
    for make, init in zip(MAKERS, (("ones",), ("ones", "ones"))):
        m = make(R, M, layout='observed')
        m.initialise(*init)

        def gone():
            raise bnmtf_amd.BnmtfError("no device in this test")
        monkeypatch.setattr(_lib, "lib", gone)
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(1)
        monkeypatch.undo()
        assert "at most" not in str(e.value) and "no device in this test" in str(e.value)
    # (the dense layout keeps its limit, said by its own create before any device call)
    d = MAKERS[0](R.T.copy(), M.T.copy())
    d.initialise('ones')
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        d.run(1)
    assert "at most 16384 entries" in str(e.value)


def test_M_test_is_refused_before_any_device_call(no_device):
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    for m in _models():
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Mt)
        assert "M_test" in str(e.value) and "layout='observed'" in str(e.value) and type(m).__name__ in str(e.value)
        assert not hasattr(m, "all_performances_test")


def test_run_many_refuses_an_observed_model_alone_and_in_a_mixed_list(no_device):
    for m, dense in zip(_models(), (MAKERS[0], MAKERS[1])):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            bnmtf_amd.run_many([m], 3)
        assert "layout='observed'" in str(e.value) and "model 0" in str(e.value)
        d = dense(m.R, m.M)
        d.initialise('ones') if isinstance(d, NMF) else d.initialise('ones', 'ones')
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            bnmtf_amd.run_many([d, m], 3)
        assert "layout='observed'" in str(e.value) and "model 1" in str(e.value)
    assert "run_many" in _observed.REFUSALS


def test_a_sharded_model_is_refused_at_construction(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    for make, name in zip(MAKERS, ("NMF", "NMTF")):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            make(R, M, layout='observed', rank=0, world=2, comm_id=bytes(128))
        assert "layout='observed'" in str(e.value) and "world = 1" in str(e.value) and str(e.value).startswith(name + ":")
        with pytest.raises(bnmtf_amd.BnmtfError) as e:                     # (the dense layout's own message, as before)
            make(R, M, rank=0, world=2, comm_id=bytes(128))
        assert "layout='observed'" not in str(e.value) and "runs on one GPU" in str(e.value)


def test_ranks_256_are_taken_and_257_refused(no_device):
    R = np.ones((8, 9)); M = np.ones((8, 9))
    assert NMF(R, M, 256, verbose=False, layout='observed').K == 256
    m = NMTF(R, M, 256, 256, verbose=False, layout='observed')
    assert (m.K, m.L) == (256, 256)
    for make, name in ((lambda: NMF(R, M, 257, verbose=False, layout='observed'), "K = 257"),
                       (lambda: NMTF(R, M, 257, 2, verbose=False, layout='observed'), "K = 257"),
                       (lambda: NMTF(R, M, 2, 257, verbose=False, layout='observed'), "L = 257"),
                       (lambda: NMTF(R, M, 2, 0, verbose=False, layout='observed'), "L = 0")):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            make()
        assert name in str(e.value) and "layout='observed'" in str(e.value) and "<= 256" in str(e.value)
    assert _observed.MAX_RANK == 256


def test_header_exports_map_and_binding_list_the_same_new_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmt?f_onp_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(NEW)
    assert {n for n in _lib.EXPORTS if "_onp_" in n} == set(NEW)
    every = re.findall(r"^BNMTF_API\s+[\w\s\*]+?\b(bnmt?f_\w+)\s*\(", hdr, flags=re.M)
    assert len(_lib.EXPORTS) == len(every) == len(set(every)), (len(_lib.EXPORTS), len(every))
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    for n in NEW:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    assert re.search(r"^#define BNMTF_ONP_MAX_RANK 256$", hdr, flags=re.M)
    # every one is a function-try-block ending in the guard
    src = open(os.path.join(CSRC, "api_obs_np.inc")).read()
    for n in NEW:
        assert re.search(r"^int %s\([^{]*?\) try \{" % n, src, flags=re.M | re.S), n
    assert src.count("} BNMTF_ABI_GUARD") == len(NEW)
    # a null handle or null argument is an error code, not a crash
    assert lib.bnmtf_onp_create(3, 3, 2, 0, 1, None, None, None, 0, None) == -1
    h = C.c_void_p()
    assert lib.bnmtf_onp_create(3, 3, 2, 0, 1, None, None, None, 0, C.byref(h)) == -1 and h.value is None
    assert b"bnmtf_onp_create" in lib.bnmtf_last_error()
    assert lib.bnmtf_onp_set_state(None, None, None, None) == -1
    assert lib.bnmtf_onp_get_state(None, None, None, None) == -1
    assert lib.bnmtf_onp_run(None, 1, None, None, None) == -1
    assert lib.bnmtf_onp_update(None, 0, 0, 0) == -1
    assert lib.bnmtf_onp_metrics(None, 0, None, None, None, None) == -1
    assert b"bnmtf_onp_create" in lib.bnmtf_last_error()


def test_create_refuses_ranks_and_lists_before_any_device_call():
    """K or L out of range and what bnmtf_obs_create refuses of the entries, with its messages: ahead of the first device call
    (this machine has no GPU: a create that reached the device would fail with a HIP error instead)."""
    lib = bnmtf_amd.lib()
    M = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 1]])
    rows, cols, vals = _observed.entry_list(np.arange(12.0).reshape(4, 3), M)
    h = C.c_void_p()

    def refused(K, L, r, c, v, n=None):
        rc = lib.bnmtf_onp_create(4, 3, K, L, len(r) if n is None else n, _lib.ptr(r), _lib.ptr(c), _lib.ptr(v), 0, C.byref(h))
        assert rc == -1 and h.value is None
        return lib.bnmtf_last_error().decode()

    for L in (0, 2):
        assert "K=257" in refused(257, L, rows, cols, vals) and "K=0" in refused(0, L, rows, cols, vals)
        keep = rows != 1
        assert "Fully unobserved row in R, row 1." in refused(2, L, rows[keep].copy(), cols[keep].copy(), vals[keep].copy())
        keep = cols != 0
        assert "Fully unobserved column in R, column 0." in refused(2, L, rows[keep].copy(), cols[keep].copy(), vals[keep].copy())
        r2 = rows.copy(); r2[2] = 4
        assert "entry 2 (4, 1) lies outside the 4 x 3 matrix" in refused(2, L, r2, cols, vals)
        assert "occurs twice" in refused(2, L, np.append(rows, rows[3]).astype(np.int32), np.append(cols, cols[3]).astype(np.int32), np.append(vals, 1).astype(np.float32))
        assert "between 1 and 2^31 - 1 entries (n=0)" in refused(2, L, rows, cols, vals, n=0)
    assert "L=257" in refused(2, 257, rows, cols, vals) and "L=-1" in refused(2, -1, rows, cols, vals)


def test_the_new_kernels_compile_for_gfx950_without_spills_or_scratch():
    """kernel_obs_np.hip: every kernel without spills and without scratch; the half sweep -- eight slots of p, r, j and v per lane
    in its widest instantiation -- within 128 VGPRs, four waves per SIMD, with the four waves' rows and fold in LDS."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_obs_np.hip"), "-o", os.devnull]
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
    kernels = {"onp_sweep_kernel": 1, "obs_fold_kernel": 1, "onp_eff_kernel": 1, "onp_s_pass_kernel": 2, "onp_metric_kernel": 1}
    assert len(found) == sum(kernels.values()), sorted(found)
    for kernel, count in kernels.items():
        hits = [r for n, r in found.items() if kernel in n]
        assert len(hits) == count, (kernel, sorted(found))
        for r in hits:
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
            assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (kernel, r)
    assert [r for n, r in found.items() if "onp_sweep_kernel" in n][0]["LDS Size [bytes/block]"] <= 4 * 256 * 4 + 4 * 8 * 8


def test_the_six_entry_points_run_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_onp.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_onp` and started as an ordinary child process."""
    exe = os.path.join(CSRC, "build", "san", "driver_onp_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_onp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver onp: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
