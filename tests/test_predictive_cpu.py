"""Host side of bnmtf_amd.posterior_predictive: everything it refuses -- before any device call --, the
export, the entry point bnmtf_predictive_samples in the header, the exports map and the binding, what the C call refuses, the
resources of the new kernel and a sanitizer run of the new host code through a stand-alone program.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, Entries, _lib, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, bnmtf_vb_optimised, nmf_icm, nmtf_icm, posterior_predictive, predictive)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = "bnmtf_predictive_samples"
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


AT = (np.array([0, 5, 2]), np.array([4, 0, 2]))


def _refused(model, at, burn_in, thinning, *texts, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        posterior_predictive(model, at, burn_in, thinning, **kw)
    for text in (type(model).__name__,) + texts:
        assert text in str(e.value), (text, str(e.value))


def test_posterior_predictive_is_exported():
    assert "posterior_predictive" in bnmtf_amd.__all__ and bnmtf_amd.posterior_predictive is predictive.posterior_predictive
    assert bnmtf_amd.predictive is predictive and callable(predictive.from_samples)


def test_a_model_without_stored_samples_is_refused(no_device):
    for m in _samplers(None):
        _refused(m, AT, 0, 1, "no stored samples", "run() has not been called")
    for m in _samplers(0):
        _refused(m, AT, 0, 1, "no stored samples", "store_samples=False")


def test_burn_in_and_thinning_outside_the_stored_samples_are_refused(no_device):
    for m in _samplers(4):
        _refused(m, AT, 4, 1, "burn_in", "4 stored")
        _refused(m, AT, 9, 2, "burn_in", "4 stored")
        _refused(m, AT, -1, 1, "burn_in")
        _refused(m, AT, 0, 0, "thinning >= 1")
        _refused(m, AT, 1, -2, "thinning >= 1")


def test_a_list_that_is_no_list_of_the_models_entries_is_refused(no_device):
    for m in _samplers(4):
        _refused(m, (np.array([0, I]), np.array([0, 1])), 0, 1, "entry 1 (6, 1) lies outside the 6 x 5 matrix")
        _refused(m, (np.array([0, 1]), np.array([-1, 1])), 0, 1, "entry 0 (0, -1) lies outside the 6 x 5 matrix")
        _refused(m, (np.array([0, 1]), np.array([J, 1])), 0, 1, "entry 0 (0, 5) lies outside")
        _refused(m, Entries((I, J + 1), [0], [0], [1.]), 0, 1, "different shapes", "(6, 6) and (6, 5)")
        _refused(m, Entries((I, J), [], [], []), 0, 1, "empty")
        _refused(m, (np.zeros(0, dtype=int), np.zeros(0, dtype=int)), 0, 1, "empty")
        _refused(m, (np.array([0, 1]), np.array([0])), 0, 1, "different lengths: 2 and 1")
        _refused(m, (np.array([0.5, 1]), np.array([0, 1])), 0, 1, "rows holds integers")
        _refused(m, 3, 0, 1, "an Entries or a pair (rows, cols)")


def test_point_estimates_and_variational_models_are_refused(no_device):
    R, M = _dense()
    points = [nmf_icm(R, M, 2, PRI, verbose=False), nmtf_icm(R, M, 2, 2, PRI3, verbose=False), NMF(R, M, 2, verbose=False),
              NMTF(R, M, 2, 2, verbose=False), nmf_icm(R, M, 2, PRI, verbose=False, layout='observed'), NMF(R, M, 2, verbose=False, layout='observed')]
    for m in points:
        _refused(m, AT, 0, 1, "point estimate", "no posterior samples")
    vb = [bnmf_vb_optimised(R, M, 2, PRI, verbose=False), bnmf_vb_observed(R, M, 2, PRI, verbose=False),
          bnmtf_vb_optimised(R, M, 2, 2, PRI3, verbose=False), bnmtf_vb_observed(R, M, 2, 2, PRI3, verbose=False)]
    for m in vb:
        _refused(m, AT, 0, 1, "variational", "closed form of q", "out of scope")
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        posterior_predictive(object(), AT, 0, 1)
    assert "object" in str(e.value) and "bnmf_gibbs_optimised" in str(e.value)


def test_from_samples_refuses_before_any_device_call(no_device):
    A, B = np.ones((6, I, 2), dtype=np.float32), np.ones((6, J, 2), dtype=np.float32)
    S = np.ones((6, 2, 3), dtype=np.float32)
    taus = np.ones(6)

    def refused(text, factors=(A, B), taus=taus, shape=(I, J), at=AT, indices=range(1, 6, 2), **kw):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            predictive.from_samples(factors, taus, shape, at[0], at[1], indices, **kw)
        assert text in str(e.value), (text, str(e.value))

    refused("arithmetic progression", indices=[0, 1, 3])
    refused("arithmetic progression", indices=[3, 2, 1])
    refused("arithmetic progression", indices=[2, 2])
    refused("no sample selected", indices=[])
    refused("lie outside the 6 stored samples", indices=[4, 6])
    refused("lie outside the 6 stored samples", indices=[-1, 0])
    refused("(all_A, all_B) or (all_A, all_S, all_B)", factors=(A,))
    refused("different numbers of samples", factors=(A, B[:5]))
    refused("do not belong to a 6 x 5 matrix", factors=(A, S, B))          # (B's width is K, not L)
    refused("do not belong to a 6 x 5 matrix", factors=(B, A))
    refused("do not belong to a 7 x 5 matrix", shape=(7, 5))
    refused("ranks 1 .. 256", factors=(np.ones((6, I, 257), dtype=np.float32), np.ones((6, J, 257), dtype=np.float32)))
    refused("three-dimensional", factors=(A[:, 0], B[:, 0]))
    refused("taus holds a value per stored sample", taus=np.ones(3))
    refused("chunk_samples >= 0", chunk_samples=-1)
    refused("entry 1 (5, 5) lies outside", at=(np.array([0, 5]), np.array([0, 5])))


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_point():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    sig = (r"int device, int I, int J, int K, int L, uint64_t n,\s*const int32_t\* rows, const int32_t\* cols, const float\* A, "
           r"const float\* S, const float\* B,\s*uint64_t first, uint64_t step, int T, int chunk_samples,\s*double\* p_first, double\* sum_d, "
           r"double\* sum_d2")
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(%s\);" % (NEW, sig), hdr, flags=re.M)
    P = C.c_void_p
    assert NEW in _lib.EXPORTS and _lib._SIGS[NEW] == ([C.c_int] * 5 + [C.c_uint64, P, P, P, P, P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, P, P, P], C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    assert not any(t in NEW for t in ("_obs_", "_otri_", "_otvb_", "_onp_"))
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    assert any(fnmatch.fnmatchcase(NEW, g) for g in globs)
    assert hasattr(bnmtf_amd.lib(), NEW), "libbnmtf_hip.so does not export %s" % NEW
    src = open(os.path.join(CSRC, "api_predictive.inc")).read()
    assert re.search(r"^int %s\([^{]*?\) try \{" % NEW, src, flags=re.M | re.S) and "BNMTF_ABI_GUARD" in src
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert api.rstrip().endswith('#include "api_predictive.inc"')
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernel_predictive\.hip\b", mk, flags=re.M) and re.search(r"^asan_predictive:", mk, flags=re.M)


def test_the_c_call_answers_null_pointers_and_bad_limits_with_an_error_code():
    lib = bnmtf_amd.lib()
    rows = np.zeros(2, dtype=np.int32); A = np.ones((1, 3, 2), dtype=np.float32); S = np.ones((1, 2, 2), dtype=np.float32)
    out = np.zeros(2)
    p = _lib.ptr

    def call(device=0, n_i=3, n_j=3, K=2, L=0, n=2, r=rows, c=rows, a=A, s=None, b=A, first=0, step=1, T=1, chunk=0, o0=out, o1=out, o2=out):
        return lib.bnmtf_predictive_samples(device, n_i, n_j, K, L, C.c_uint64(n), p(r), p(c), p(a), p(s), p(b), C.c_uint64(first), C.c_uint64(step), T, chunk,
                                            p(o0), p(o1), p(o2))

    for kw, text in (({"r": None}, "null argument"), ({"c": None}, "null argument"), ({"a": None}, "null argument"), ({"b": None}, "null argument"),
                     ({"o0": None}, "null argument"), ({"o1": None}, "null argument"), ({"o2": None}, "null argument"),
                     ({"n_i": 0}, "unsupported shape"), ({"n_j": -1}, "unsupported shape"), ({"K": 0}, "unsupported shape"), ({"K": 257}, "unsupported shape"),
                     ({"L": -1}, "unsupported shape"), ({"L": 257, "s": S}, "unsupported shape"),
                     ({"L": 2}, "S is required when L >= 1"), ({"s": S}, "null when L = 0"),
                     ({"n": 0}, "1 <= n < 2^31"), ({"n": 2 ** 31}, "1 <= n < 2^31"),
                     ({"T": 0}, "T >= 1"), ({"step": 0}, "step >= 1"), ({"chunk": -1}, "chunk_samples >= 0"),
                     ({"r": np.array([0, 3], dtype=np.int32)}, "entry 1 (3, 0) lies outside the 3 x 3 matrix"),
                     ({"c": np.array([-1, 0], dtype=np.int32)}, "entry 0 (0, -1) lies outside the 3 x 3 matrix")):
        assert call(**kw) == EINVAL, kw
        msg = lib.bnmtf_last_error().decode()
        assert msg.startswith(NEW + ": ") and text in msg, (kw, msg)


# ---------------------------------------------------------------- the kernel and the host code
def test_the_new_kernel_compiles_for_gfx950_without_spills_or_scratch():
    """kernel_predictive.hip: one kernel in two instantiations (16-byte and 4-byte loads of the gathered rows), no spills, no
    scratch, the four waves' staged rows as doubles in LDS and nothing else (4 x 256 x 8 bytes: DESIGN.md section 2.8), within 128
    VGPRs: at least four waves per SIMD."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_predictive.hip"), "-o", os.devnull]
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
    assert len(found) == 2 and all("predictive_kernel" in n for n in found), sorted(found)
    for n, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (n, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (n, r)
        assert r["LDS Size [bytes/block]"] <= 4 * 256 * 8, (n, r)


def test_the_entry_point_runs_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_predictive.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_predictive` and started as an ordinary child process: both forms, chunk sizes from
    one sample to more than there are, strided and consecutive samples, duplicates, a call that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_predictive_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_predictive"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver predictive: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
