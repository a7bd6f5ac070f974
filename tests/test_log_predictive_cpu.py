"""Host side of bnmtf_amd.log_predictive: everything it refuses -- before any device call --, the export,
the entry points bnmtf_log_predictive_samples / _times in the header, the exports map and the binding, what the C call refuses, the
resources of the new kernel and a sanitizer run of the new host code through a stand-alone program.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, Entries, _lib, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, bnmtf_vb_optimised, nmf_icm, nmtf_icm)
from bnmtf_amd import log_predictive

module = sys.modules["bnmtf_amd.log_predictive"]          # (the package's attribute of that name is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW, TIMES = "bnmtf_log_predictive_samples", "bnmtf_log_predictive_times"
EINVAL = -1


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def _dense(seed=0):
    rs = np.random.RandomState(seed)
    M = (rs.rand(I, J) < 0.5).astype(float)
    M[np.arange(I), np.arange(I) % J] = 1; M[np.arange(J) % I, np.arange(J)] = 1
    return rs.rand(I, J) * 3 + 0.1, M


def _samplers(stored=4):
    """a two-factor and a tri-factorisation sampler of either layout, with `stored` samples put there by hand (None: never run)"""
    R, M = _dense()
    out = []
    for layout in ('dense', 'observed'):
        a = bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False, layout=layout)
        b = bnmtf_gibbs_optimised(R, M, 2, 3, PRI3, verbose=False, layout=layout)
        if stored is not None:
            a.all_U, a.all_V = np.ones((stored, I, 2), dtype=np.float32), np.ones((stored, J, 2), dtype=np.float32)
            b.all_F, b.all_S, b.all_G = (np.ones((stored, I, 2), dtype=np.float32), np.ones((stored, 2, 3), dtype=np.float32),
                                         np.ones((stored, J, 3), dtype=np.float32))
            a.all_tau = b.all_tau = np.ones(max(stored, 3))
        out += [a, b]
    return out


AT = Entries((I, J), [0, 5, 2], [4, 0, 2], [1., 2., 3.])


def _refused(model, at, burn_in, thinning, *texts, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        log_predictive(model, at, burn_in, thinning, **kw)
    assert str(e.value).startswith(type(model).__name__ + ": log_predictive: "), str(e.value)
    for text in texts:
        assert text in str(e.value), (text, str(e.value))


def test_log_predictive_is_exported():
    assert "log_predictive" in bnmtf_amd.__all__ and callable(bnmtf_amd.log_predictive) and log_predictive is module.log_predictive
    assert bnmtf_amd.log_predictive.from_samples is module.from_samples and hasattr(module, "LogPredictive")


def test_a_model_without_stored_samples_is_refused(no_device):
    for at in (AT, None):
        for m in _samplers(None):
            _refused(m, at, 0, 1, "no stored samples", "run() has not been called")
        for m in _samplers(0):
            _refused(m, at, 0, 1, "no stored samples", "store_samples=False")


def test_burn_in_and_thinning_outside_the_stored_samples_are_refused(no_device):
    for m in _samplers(4):
        _refused(m, AT, 4, 1, "burn_in", "4 stored")
        _refused(m, None, 9, 2, "burn_in", "4 stored")
        _refused(m, AT, -1, 1, "burn_in")
        _refused(m, AT, 0, 0, "thinning >= 1")
        _refused(m, None, 1, -2, "thinning >= 1")


def test_a_list_without_values_or_of_another_shape_is_refused(no_device):
    for m in _samplers(4):
        _refused(m, (np.array([0, 1]), np.array([0, 1])), 0, 1, "a density needs values", "a pair (rows, cols)", "None for the training entries")
        _refused(m, [np.array([0, 1]), np.array([0, 1])], 0, 1, "a density needs values", "a pair (rows, cols)")
        _refused(m, 3, 0, 1, "a density needs values", "int")
        _refused(m, Entries((I, J + 1), [0], [0], [1.]), 0, 1, "different shapes", "(6, 6) and (6, 5)")
        _refused(m, Entries((I + 1, J), [0], [0], [1.]), 0, 1, "different shapes", "(7, 5) and (6, 5)")
        _refused(m, Entries((I, J), [], [], []), 0, 1, "empty")


def test_point_estimates_and_variational_models_are_refused(no_device):
    R, M = _dense()
    points = [nmf_icm(R, M, 2, PRI, verbose=False), nmtf_icm(R, M, 2, 2, PRI3, verbose=False), NMF(R, M, 2, verbose=False),
              NMTF(R, M, 2, 2, verbose=False), nmf_icm(R, M, 2, PRI, verbose=False, layout='observed'), NMF(R, M, 2, verbose=False, layout='observed')]
    for m in points:
        for at in (AT, None):
            _refused(m, at, 0, 1, "point estimate", "no posterior samples")
    vb = [bnmf_vb_optimised(R, M, 2, PRI, verbose=False), bnmf_vb_observed(R, M, 2, PRI, verbose=False),
          bnmtf_vb_optimised(R, M, 2, 2, PRI3, verbose=False), bnmtf_vb_observed(R, M, 2, 2, PRI3, verbose=False)]
    for m in vb:
        for at in (AT, None):
            _refused(m, at, 0, 1, "variational", "no posterior samples", "it has variational_predictive")
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        log_predictive(object(), AT, 0, 1)
    assert str(e.value).startswith("object: log_predictive: ") and "bnmf_gibbs_optimised" in str(e.value)


def test_from_samples_refuses_before_any_device_call(no_device):
    A, B = np.ones((6, I, 2), dtype=np.float32), np.ones((6, J, 2), dtype=np.float32)
    S = np.ones((6, 2, 3), dtype=np.float32)
    taus = np.ones(6)
    at = (np.array([0, 5, 2]), np.array([4, 0, 2]))
    vals = np.array([1., 2., 3.])

    def refused(text, factors=(A, B), taus=taus, shape=(I, J), at=at, values=vals, indices=range(1, 6, 2), **kw):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            log_predictive.from_samples(factors, taus, shape, at[0], at[1], values, indices, **kw)
        assert str(e.value).startswith("log_predictive.from_samples: ") and text in str(e.value), (text, str(e.value))

    refused("arithmetic progression", indices=[0, 1, 3])
    refused("arithmetic progression", indices=[3, 2, 1])
    refused("arithmetic progression", indices=[2, 2])
    refused("no sample selected", indices=[])
    refused("the sample indices are integers", indices=[0.5, 1.5])
    refused("lie outside the 6 stored samples", indices=[4, 6])
    refused("lie outside the 6 stored samples", indices=[-1, 0])
    refused("(all_A, all_B) or (all_A, all_S, all_B)", factors=(A,))
    refused("different numbers of samples", factors=(A, B[:5]))
    refused("do not belong to a 6 x 5 matrix", factors=(A, S, B))          # (B's width is K, not L)
    refused("do not belong to a 7 x 5 matrix", shape=(7, 5))
    refused("ranks 1 .. 256", factors=(np.ones((6, I, 257), dtype=np.float32), np.ones((6, J, 257), dtype=np.float32)))
    refused("three-dimensional", factors=(A[:, 0], B[:, 0]))
    refused("taus holds a value per stored sample", taus=np.ones(3))
    refused("chunk_samples >= 0", chunk_samples=-1)
    refused("entry 1 (5, 5) lies outside", at=(np.array([0, 5, 1]), np.array([0, 5, 1])))
    refused("values holds the true value of every entry: 3 entries", values=np.ones(2))
    refused("values holds the true value of every entry", values=np.ones((3, 1)))
    refused("the value of entry 1 (5, 0) is not finite: nan", values=np.array([1., np.nan, 3.]))
    refused("the value of entry 2 (2, 2) is not finite: inf", values=np.array([1., 2., np.inf]))
    refused("every selected tau is finite and positive", taus=np.array([1., 1., 1., 0., 1., 1.]))
    refused("every selected tau is finite and positive", taus=np.array([1., np.inf, 1., 1., 1., 1.]))
    refused("every selected tau is finite and positive", taus=np.array([1., 1., 1., 1., 1., np.nan]))


def test_waic_needs_two_samples_and_its_formulas_are_the_usual_ones():
    LP = module.LogPredictive
    n = 4
    rows = cols = np.arange(n, dtype=np.int32)
    one = LP(rows, cols, np.ones(n), np.array([-1., -2., -3., -4.]), np.array([-1., -2., -3., -4.]), np.full(n, np.nan), 1)
    assert one.lppd() == -10.0 and len(one) == n and one.count == 1 and "4 entries, 1 samples" in repr(one)
    for f in (one.waic, one.p_waic, one.pointwise, one.se):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            f()
        assert str(e.value).startswith("LogPredictive: " + f.__name__ + ": ") and "at least two" in str(e.value) and "1 selected" in str(e.value)
    lpd, var = np.array([-1., -2.5, -3., -4.]), np.array([0.25, 0.5, 0.125, 1.])
    two = LP(rows, cols, np.ones(n), lpd, lpd - 0.5, var, 2)
    assert two.lppd() == lpd.sum() and two.p_waic() == var.sum() and two.waic() == -2.0 * (lpd.sum() - var.sum())
    assert np.array_equal(two.pointwise(), lpd - var)
    assert two.se() == float(np.sqrt(n * np.var(-2.0 * (lpd - var), ddof=1)))
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        LP(rows[:1], cols[:1], np.ones(1), lpd[:1], lpd[:1], var[:1], 2).se()
    assert "at least two" in str(e.value)


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    sig = (r"int device, int I, int J, int K, int L, uint64_t n,\s*const int32_t\* rows, const int32_t\* cols, const double\* values, "
           r"const float\* A, const float\* S, const float\* B,\s*uint64_t first, uint64_t step, int T, int chunk_samples, "
           r"const double\* c, const double\* h,\s*double\* l_first, double\* sum_d, double\* sum_d2, double\* l_max, double\* sum_exp")
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(%s\);" % (NEW, sig), hdr, flags=re.M)
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(double\* upload_ms, double\* kernel_ms\);" % TIMES, hdr, flags=re.M)
    P, D = C.c_void_p, C.POINTER(C.c_double)
    assert _lib._SIGS[NEW] == ([C.c_int] * 5 + [C.c_uint64] + [P] * 6 + [C.c_uint64, C.c_uint64, C.c_int, C.c_int] + [P] * 7, C.c_int)
    assert _lib._SIGS[TIMES] == ([D, D], C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d entry points" % len(_lib.EXPORTS) in readme
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    src = open(os.path.join(CSRC, "api_log_predictive.inc")).read()
    for name in (NEW, TIMES):
        assert name in _lib.EXPORTS and any(fnmatch.fnmatchcase(name, g) for g in globs)
        assert hasattr(bnmtf_amd.lib(), name), "libbnmtf_hip.so does not export %s" % name
        assert re.search(r"^int %s\([^{]*?\) try \{" % name, src, flags=re.M | re.S)
    assert src.count("} BNMTF_ABI_GUARD") == 2 and "CallScope cs;" in src and "kCallLogPredictive" in src
    # the row sort and the upload of a chunk are shared with api_predictive.inc, not copied: both call api.hip's
    api = open(os.path.join(CSRC, "api.hip")).read()
    old = open(os.path.join(CSRC, "api_predictive.inc")).read()
    assert api.count('#include "api_log_predictive.inc"') == 1
    for helper in ("sort_entries_by_row", "upload_samples", "sample_chunk"):
        assert len(re.findall(r"^static \w+ %s\(" % helper, api, flags=re.M)) == 1, helper
        assert helper + "(" in src and helper + "(" in old and not re.search(r"^static .*\b%s\(" % helper, src + old, flags=re.M), helper
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernel_log_predictive\.hip\b", mk, flags=re.M) and re.search(r"^asan_log_predictive:", mk, flags=re.M)
    assert re.search(r"^APIDEPS = .*\bapi_log_predictive\.inc\b", mk, flags=re.M)
    kh = open(os.path.join(CSRC, "kernels.h")).read()
    assert "struct LogPredictiveArgs {" in kh and "void launch_log_predictive(const LogPredictiveArgs& a, hipStream_t st);" in kh


def test_the_c_call_answers_null_pointers_bad_limits_and_values_that_are_not_finite_with_an_error_code():
    """with a device that does not exist (-1): every refusal comes before the first device call"""
    lib = bnmtf_amd.lib()
    rows = np.zeros(2, dtype=np.int32); A = np.ones((2, 3, 2), dtype=np.float32); S = np.ones((2, 2, 2), dtype=np.float32)
    vals, cc, hh = np.ones(2), np.zeros(2), np.ones(2)
    out = np.zeros(2)
    p = _lib.ptr

    def call(n_i=3, n_j=3, K=2, L=0, n=2, r=rows, c=rows, v=vals, a=A, s=None, b=A, first=0, step=1, T=2, chunk=0, cc=cc, hh=hh, o0=out, o1=out,
             o2=out, o3=out, o4=out):
        return lib.bnmtf_log_predictive_samples(-1, n_i, n_j, K, L, C.c_uint64(n), p(r), p(c), p(v), p(a), p(s), p(b), C.c_uint64(first), C.c_uint64(step),
                                                T, chunk, p(cc), p(hh), p(o0), p(o1), p(o2), p(o3), p(o4))

    def but(a, at, v):
        a = a.copy(); a[at] = v
        return a

    cases = [({k: None}, "null argument") for k in ("r", "c", "v", "a", "b", "cc", "hh", "o0", "o1", "o2", "o3", "o4")]
    cases += [({"n_i": 0}, "unsupported shape"), ({"n_j": -1}, "unsupported shape"), ({"K": 0}, "unsupported shape"), ({"K": 257}, "unsupported shape"),
              ({"L": -1}, "unsupported shape"), ({"L": 257, "s": S}, "unsupported shape"),
              ({"L": 2}, "S is required when L >= 1"), ({"s": S}, "null when L = 0"),
              ({"n": 0}, "1 <= n < 2^31"), ({"n": 2 ** 31}, "1 <= n < 2^31"),
              ({"T": 0}, "T >= 1"), ({"step": 0}, "step >= 1"), ({"chunk": -1}, "chunk_samples >= 0"),
              ({"r": np.array([0, 3], dtype=np.int32)}, "entry 1 (3, 0) lies outside the 3 x 3 matrix"),
              ({"c": np.array([-1, 0], dtype=np.int32)}, "entry 0 (0, -1) lies outside the 3 x 3 matrix"),
              ({"v": but(vals, 1, np.nan)}, "values: the value of entry 1 (0, 0) is not finite"),
              ({"v": but(vals, 0, -np.inf)}, "values: the value of entry 0 (0, 0) is not finite"),
              ({"cc": but(cc, 1, np.inf)}, "c[1] is not finite"), ({"cc": but(cc, 0, np.nan)}, "c[0] is not finite"),
              ({"hh": but(hh, 1, 0.0)}, "h[1] is not finite and positive"), ({"hh": but(hh, 0, -1.0)}, "h[0] is not finite and positive"),
              ({"hh": but(hh, 0, np.inf)}, "h[0] is not finite and positive"), ({"hh": but(hh, 1, np.nan)}, "h[1] is not finite and positive")]
    for kw, text in cases:
        assert call(**kw) == EINVAL, kw
        msg = lib.bnmtf_last_error().decode()
        assert msg.startswith(NEW + ": ") and text in msg, (kw, msg)
    assert lib.bnmtf_log_predictive_times(None, None) == EINVAL and lib.bnmtf_last_error().decode().startswith(TIMES + ": null argument")
    up, kn = C.c_double(-1), C.c_double(-1)
    assert lib.bnmtf_log_predictive_times(C.byref(up), C.byref(kn)) == 0 and up.value >= 0.0 and kn.value >= 0.0


# ---------------------------------------------------------------- the kernel and the host code
def test_the_new_kernel_compiles_for_gfx950_without_spills_or_scratch_at_the_stated_resources():
    """kernel_log_predictive.hip: one kernel in two instantiations (16-byte and 4-byte loads of the gathered rows), no spills, no
    scratch, the four waves' staged rows as doubles in LDS and nothing else (4 x 256 x 8 bytes), and the VGPR counts its header and
    DESIGN.md section 2.8b state."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_log_predictive.hip"), "-o", os.devnull]
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
    assert len(found) == 2 and all("log_predictive_kernel" in n for n in found), sorted(found)
    src = open(os.path.join(CSRC, "kernel_log_predictive.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 2.8b"):]
    for n, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (n, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (n, r)
        assert r["LDS Size [bytes/block]"] == 4 * 256 * 8, (n, r)
        stated = "%s loads %d VGPRs" % ("16-byte" if "ILb1E" in n else "4-byte", r["VGPRs"])
        assert stated in src and stated in section, (n, r, stated)
    assert "8 192 bytes of" in src and "8 192 bytes of" in section


def test_the_entry_point_runs_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_log_predictive.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_log_predictive` and started as an ordinary child process: both forms, chunk sizes
    from one sample to more than there are, strided and consecutive samples, duplicates, a call that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_log_predictive_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_log_predictive"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver log_predictive: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
