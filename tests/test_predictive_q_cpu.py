"""Host side of bnmtf_amd.variational_predictive: the closed form against the brute-force definition,
exactly, on integer moments; that the integer cases of tests/_predictive_q_cases.py stay exact in fp64 at every rank; everything
the call refuses -- before any device call --; the export, the entry points in the header, the exports map and the binding; what
the C call refuses; the resources of the new kernels; and a sanitizer run of the new host code through a stand-alone program.  No
GPU needed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, Entries, _lib, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, bnmtf_vb_optimised, nmf_icm, nmtf_icm, posterior_predictive, predictive, predictive_q,
                       variational_predictive)

import _predictive_q_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = "bnmtf_predictive_moments"
TIMES = "bnmtf_predictive_moments_times"
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


def _variational(q=True, tau=True):
    """the four variational classes, never initialised on a device: q (exp*, var*) and q(tau) put there by hand"""
    R, M = _dense()
    out = [bnmf_vb_optimised(R, M, 2, PRI, verbose=False), bnmf_vb_observed(R, M, 2, PRI, verbose=False),
           bnmtf_vb_optimised(R, M, 2, 3, PRI3, verbose=False), bnmtf_vb_observed(R, M, 2, 3, PRI3, verbose=False)]
    for m in out:
        if q:
            for f, shape in zip(m._FACTORS, m._factor_shapes()):
                setattr(m, "exp" + f, np.ones(shape)); setattr(m, "var" + f, np.ones(shape))
        if tau:
            m.alpha_s, m.beta_s = 3.0, 4.0
    return out


AT = (np.array([0, 5, 2]), np.array([4, 0, 2]))


def _refused(model, at, *texts, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        variational_predictive(model, at, **kw)
    msg = str(e.value)
    assert msg.startswith(type(model).__name__ + ": variational_predictive: "), msg
    for text in texts:
        assert text in msg, (text, msg)


# ---------------------------------------------------------------- the closed form
@pytest.mark.parametrize("K, L", [(1, 0), (2, 0), (5, 0), (6, 0), (1, 1), (2, 3), (3, 2), (4, 4), (6, 5), (5, 6), (6, 6)])
def test_the_closed_form_is_the_definition_exactly_on_integer_moments(K, L):
    """moments in {0, 1, 2, 3}: both sides are sums of integers far below 2^63, so equality is exact -- each of the seven terms and
    the collapse from K^2 L^2 to K + L work per entry stand or fall here"""
    rows, cols, _ = cases.entry_list(7, 9, 'last', seed=K + 10 * L)
    rows = np.concatenate([rows, np.arange(7, dtype=np.int32)]); cols = np.concatenate([cols, np.arange(7, dtype=np.int32)])
    for seed in range(3):
        m = cases.moments(7, 9, K, L, True, seed)
        for drop in ((), (0,), (2,), (0, 2)) + (((1,), (0, 1, 2)) if L else ()):
            use = tuple(None if (q % 2 == 1 and q // 2 in drop) else a for q, a in enumerate(m))
            mean, var = cases.closed_form(rows, cols, *use)
            dmean, dvar = cases.definition(rows, cols, *use)
            assert mean.dtype == np.int64 and var.dtype == np.int64
            assert np.array_equal(mean, dmean) and np.array_equal(var, dvar), (K, L, seed, drop)
            assert (var >= 0).all()
            if set(drop) >= ({0, 1, 2} if L else {0, 2}):          # every factor fixed: no variance
                assert not var.any()
    # S = I without a variance: the tri-factorisation's form is the two-factor form
    if L == 0:
        EA, VA, _, _, EB, VB = m
        two = cases.closed_form(rows, cols, EA, VA, None, None, EB, VB)
        tri = cases.closed_form(rows, cols, EA, VA, np.eye(K, dtype=np.int64), np.zeros((K, K), dtype=np.int64), EB, VB)
        assert np.array_equal(two[0], tri[0]) and np.array_equal(two[1], tri[1])


def test_the_integer_cases_stay_exact_in_fp64_at_every_rank():
    """every mean, variance and -- all terms being non-negative -- partial sum of the integer cases is an integer below
    (K L)^2 12^3 (7.42e12 at K = L = 256) < 2^53: fp64 holds them exactly in any order of summation"""
    assert cases.integer_limit(256, 256) == 256 ** 4 * 12 ** 3 < 7.43e12 < 2 ** 53
    for shape in cases.SHAPES:
        c = cases.case(shape, True)
        K, L = shape[2], shape[3]
        assert all(a is None or (a.dtype == np.int64 and a.min() >= 0 and a.max() <= 3) for a in c["m"])
        assert c["mean"].dtype == np.int64 and 0 <= c["mean"].min() and c["mean"].max() <= cases.integer_limit(K, L)
        assert c["var"].dtype == np.int64 and 0 <= c["var"].min() and c["var"].max() <= cases.integer_limit(K, L)
        assert cases.integer_limit(K, L) < 2 ** 53


def test_the_case_file_holds_the_shapes_it_names():
    per_row = np.bincount(cases.case((cases.I, cases.J, 4, 0, 'mixed'), True)["rows"], minlength=cases.I)
    assert per_row[0] == 0 and per_row[:7].tolist() == [0, 1, 63, 64, 65, 128, 129]
    assert (cases.I + 3) // 4 == 3 and cases.I % 4 != 0 and cases.J <= 140
    last = cases.case((cases.I, cases.J, 5, 0, 'last'), True)
    assert (last["rows"] == cases.I - 1).all() and len(last["rows"]) > 129
    assert {s[0] for s in cases.SHAPES if s[4] == 'one'} == {1, 3, 4, 5} and all(s[1] == 1 for s in cases.SHAPES if s[4] == 'one')
    assert {s[2] for s in cases.SHAPES if s[3] == 0} >= set(cases.RANKS) == {1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130, 256}
    assert {(3, 11), (33, 5), (5, 130)} <= {(s[2], s[3]) for s in cases.SHAPES}
    assert all(c["twins"] for c in [cases.case(s, True) for s in cases.SHAPES if s[4] != 'one'])


# ---------------------------------------------------------------- what the Python call refuses
def test_variational_predictive_is_exported():
    assert "variational_predictive" in bnmtf_amd.__all__ and bnmtf_amd.variational_predictive is predictive_q.variational_predictive
    assert variational_predictive.from_moments is predictive_q.from_moments
    assert issubclass(predictive_q.VariationalPredictive, predictive.Predictive) and predictive_q.MAX_RANK == 256
    P = predictive_q.VariationalPredictive(AT[0], AT[1], np.ones(3), np.full(3, 3.0), 1.0)
    assert "closed form of q" in repr(P) and P.count == 0 and len(P) == 3
    assert np.array_equal(P.std(), np.full(3, 2.0)) and np.array_equal(P.std(noise=False), np.sqrt(np.full(3, 3.0)))
    # Predictive itself is what it was
    assert repr(predictive.Predictive(AT[0], AT[1], np.ones(3), np.ones(3), 1.0, 4)) == "Predictive(3 entries, 4 samples)"


def test_models_that_are_not_variational_are_refused(no_device):
    R, M = _dense()
    for layout in ('dense', 'observed'):
        for m in (bnmf_gibbs_optimised(R, M, 2, PRI, verbose=False, layout=layout), bnmtf_gibbs_optimised(R, M, 2, 3, PRI3, verbose=False, layout=layout)):
            _refused(m, AT, "posterior_predictive", "samples")
    points = [nmf_icm(R, M, 2, PRI, verbose=False), nmtf_icm(R, M, 2, 2, PRI3, verbose=False), NMF(R, M, 2, verbose=False),
              NMTF(R, M, 2, 2, verbose=False), nmf_icm(R, M, 2, PRI, verbose=False, layout='observed'), NMF(R, M, 2, verbose=False, layout='observed')]
    for m in points:
        _refused(m, AT, "point estimate")
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        variational_predictive(object(), AT)
    assert str(e.value).startswith("object: variational_predictive: ") and "bnmf_vb_optimised" in str(e.value)


def test_a_model_without_q_or_without_q_of_tau_is_refused(no_device):
    for m in _variational(q=False):
        _refused(m, AT, "initialise() has not been called")
    for m in _variational():
        delattr(m, "var" + m._FACTORS[-1])
        _refused(m, AT, "var" + m._FACTORS[-1], "initialise() has not been called")
    for m in _variational(tau=False):
        _refused(m, AT, "alpha_s / beta_s")
    for m in _variational():
        m.alpha_s = 1.0
        _refused(m, AT, "alpha_s > 1", "alpha_s=1.0")
        m.alpha_s = 0.5
        _refused(m, AT, "alpha_s > 1")


def test_a_list_that_is_no_list_of_the_models_entries_is_refused(no_device):
    for m in _variational():
        _refused(m, (np.array([0, I]), np.array([0, 1])), "entry 1 (6, 1) lies outside the 6 x 5 matrix")
        _refused(m, (np.array([0, 1]), np.array([-1, 1])), "entry 0 (0, -1) lies outside the 6 x 5 matrix")
        _refused(m, (np.array([0, 1]), np.array([J, 1])), "entry 0 (0, 5) lies outside")
        _refused(m, Entries((I, J + 1), [0], [0], [1.]), "different shapes", "(6, 6) and (6, 5)")
        _refused(m, Entries((I, J), [], [], []), "empty")
        _refused(m, (np.zeros(0, dtype=int), np.zeros(0, dtype=int)), "empty")
        _refused(m, (np.array([0, 1]), np.array([0])), "different lengths: 2 and 1")
        _refused(m, (np.array([0.5, 1]), np.array([0, 1])), "rows holds integers")
        _refused(m, 3, "an Entries or a pair (rows, cols)")
        bad = np.ones((I, 2)); bad[3, 1] = -1e-9
        setattr(m, "var" + m._FACTORS[0], bad)
        _refused(m, AT, "variance that is negative or not finite")
        setattr(m, "var" + m._FACTORS[0], np.ones((I, 2)))
        bad = np.ones((I, 2)); bad[0, 0] = np.inf
        setattr(m, "exp" + m._FACTORS[0], bad)
        _refused(m, AT, "mean that is not finite")


def test_from_moments_refuses_before_any_device_call(no_device):
    EA, VA = np.ones((I, 2)), np.ones((I, 2))
    ES, VS = np.ones((2, 3)), np.ones((2, 3))
    EB, VB = np.ones((J, 2)), np.ones((J, 2))
    EG, VG = np.ones((J, 3)), np.ones((J, 3))

    def refused(text, factors=((EA, VA), (EB, VB)), shape=(I, J), at=AT, **kw):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            variational_predictive.from_moments(factors, shape, at[0], at[1], **kw)
        assert str(e.value).startswith("variational_predictive.from_moments: ") and text in str(e.value), (text, str(e.value))

    refused("a (mean, variance) pair per factor", factors=((EA, VA),))
    refused("a (mean, variance) pair per factor", factors=(EA, VA, EB, VB))
    refused("a (mean, variance) pair per factor", factors=((EA, VA), (EB,)))
    refused("a (mean, variance) pair per factor", factors=3)
    refused("do not fit each other and the 6 x 5 matrix", factors=((EA, VA), (ES, VS), (EB, VB)))      # (B's width is K, not L)
    refused("do not fit each other and the 6 x 5 matrix", factors=((EB, VB), (EA, VA)))
    refused("do not fit each other and the 7 x 5 matrix", shape=(7, 5))
    refused("different shapes", factors=((EA, VA[:, :1]), (EB, VB)))
    refused("two-dimensional", factors=((EA[0], VA[0]), (EB, VB)))
    refused("ranks 1 .. 256", factors=((np.ones((I, 257)), None), (np.ones((J, 257)), None)))
    refused("ranks 1 .. 256", factors=((EA, VA), (np.ones((2, 257)), None), (np.ones((J, 257)), None)))
    refused("variance that is negative", factors=((EA, VA), (ES, -VS), (EG, VG)))
    refused("variance that is negative or not finite", factors=((EA, VA), (EB, VB * np.nan)))
    refused("mean that is not finite", factors=((EA, VA), (EB * np.nan, None)))
    refused("entry 1 (5, 5) lies outside", at=(np.array([0, 5]), np.array([0, 5])))
    refused("the list of entries is empty", at=([], []))
    refused("come together", alpha_s=2.0)
    refused("alpha_s > 1", alpha_s=1.0, beta_s=2.0)
    refused("beta_s > 0", alpha_s=2.0, beta_s=0.0)


def test_posterior_predictive_keeps_its_refusal_of_variational_models(no_device):
    for m in _variational():
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            posterior_predictive(m, AT, 0, 1)
        assert all(t in str(e.value) for t in (type(m).__name__, "closed form of q", "out of scope here"))


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    sig = (r"int device, int I, int J, int K, int L, uint64_t n,\s*const int32_t\* rows, const int32_t\* cols,\s*const double\* EA, "
           r"const double\* VA, const double\* ES, const double\* VS, const double\* EB, const double\* VB,\s*double\* mean_out, double\* var_out")
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(%s\);" % (NEW, sig), hdr, flags=re.M)
    assert re.search(r"^BNMTF_API\s+int\s+%s\s*\(double\* upload_ms, double\* kernel_ms\);" % TIMES, hdr, flags=re.M)
    assert re.search(r"^#define BNMTF_PREDICTIVE_Q_MAX_RANK 256$", hdr, flags=re.M)
    P = C.c_void_p
    assert NEW in _lib.EXPORTS and _lib._SIGS[NEW] == ([C.c_int] * 5 + [C.c_uint64] + [P] * 10, C.c_int)
    assert TIMES in _lib.EXPORTS and _lib._SIGS[TIMES] == ([C.POINTER(C.c_double)] * 2, C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d entry points" % len(_lib.EXPORTS) in readme
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    lib = bnmtf_amd.lib()
    for name in (NEW, TIMES):
        assert any(fnmatch.fnmatchcase(name, g) for g in globs)
        assert hasattr(lib, name), "libbnmtf_hip.so does not export %s" % name
    src = open(os.path.join(CSRC, "api_predictive_q.inc")).read()
    for name in (NEW, TIMES):
        assert re.search(r"^int %s\([^{]*?\) try \{" % name, src, flags=re.M | re.S)
    assert src.count("} BNMTF_ABI_GUARD") == 2 and "CallScope cs;" in src
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert '#include "api_predictive_q.inc"' in api
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernel_predictive_q\.hip\b", mk, flags=re.M) and re.search(r"^asan_predictive_q:", mk, flags=re.M)
    assert re.search(r"^APIDEPS = .*\bapi_predictive_q\.inc\b", mk, flags=re.M)


def test_the_c_call_answers_null_pointers_and_bad_limits_with_an_error_code():
    lib = bnmtf_amd.lib()
    rows = np.zeros(2, dtype=np.int32)
    E, S = np.ones((3, 2)), np.ones((2, 2))
    out = np.zeros(2)
    p = _lib.ptr

    def call(device=0, n_i=3, n_j=3, K=2, L=0, n=2, r=rows, c=rows, ea=E, va=E, es=None, vs=None, eb=E, vb=E, o0=out, o1=out):
        return lib.bnmtf_predictive_moments(device, n_i, n_j, K, L, C.c_uint64(n), p(r), p(c), p(ea), p(va), p(es), p(vs), p(eb), p(vb), p(o0), p(o1))

    def with_value(v, at=(1, 1)):
        a = np.ones((3, 2)); a[at] = v
        return a

    for kw, text in (({"r": None}, "null argument"), ({"c": None}, "null argument"), ({"ea": None}, "null argument"), ({"eb": None}, "null argument"),
                     ({"o0": None}, "null argument"), ({"o1": None}, "null argument"),
                     ({"n_i": 0}, "unsupported shape"), ({"n_j": -1}, "unsupported shape"), ({"K": 0}, "unsupported shape"), ({"K": 257}, "unsupported shape"),
                     ({"L": -1}, "unsupported shape"), ({"L": 257, "es": S}, "unsupported shape"),
                     ({"L": 2}, "ES is required when L >= 1"), ({"es": S}, "null when L = 0"), ({"vs": S}, "null when L = 0"),
                     ({"n": 0}, "1 <= n < 2^31"), ({"n": 2 ** 31}, "1 <= n < 2^31"),
                     ({"r": np.array([0, 3], dtype=np.int32)}, "entry 1 (3, 0) lies outside the 3 x 3 matrix"),
                     ({"c": np.array([-1, 0], dtype=np.int32)}, "entry 0 (0, -1) lies outside the 3 x 3 matrix"),
                     ({"va": with_value(-1.0)}, "the rows factor holds a variance that is negative or not finite"),
                     ({"vb": with_value(np.inf)}, "the columns factor holds a variance that is negative or not finite"),
                     ({"vb": with_value(np.nan)}, "variance that is negative or not finite"),
                     ({"L": 2, "es": S, "vs": -S}, "the middle factor holds a variance that is negative"),
                     ({"ea": with_value(np.nan)}, "the rows factor holds a mean that is not finite"),
                     ({"L": 2, "es": S * np.inf}, "the middle factor holds a mean that is not finite"),
                     ({"eb": with_value(-np.inf)}, "the columns factor holds a mean that is not finite")):
        assert call(**kw) == EINVAL, kw
        msg = lib.bnmtf_last_error().decode()
        assert msg.startswith(NEW + ": ") and text in msg, (kw, msg)
    assert lib.bnmtf_predictive_moments_times(None, None) == EINVAL
    assert lib.bnmtf_last_error().decode() == TIMES + ": null argument"


# ---------------------------------------------------------------- the kernels and the host code
def test_the_new_kernels_compile_for_gfx950_without_spills_or_scratch():
    """kernel_predictive_q.hip: the table pass and the entry pass in its eight instantiations (two or three factors, 16-byte or
    8-byte loads of the gathered rows, with or without the columns factor's variance): no spills, no scratch, the four waves'
    staged rows as doubles in LDS and nothing else (4 x 4 x 256 x 8 bytes; the table pass a quarter of it: DESIGN.md section 2.8a),
    within 128 VGPRs: at least four waves per SIMD."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_predictive_q.hip"), "-o", os.devnull]
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
    assert len(found) == 9 and sum("predictive_q_table_kernel" in n for n in found) == 1, sorted(found)
    assert sum("predictive_q_kernel" in n for n in found) == 8, sorted(found)
    for n, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (n, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (n, r)
        assert r["LDS Size [bytes/block]"] <= (4 * 256 * 8 if "table" in n else 4 * 4 * 256 * 8), (n, r)
    src = open(os.path.join(CSRC, "kernel_predictive_q.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "atomic" not in code and code.count("#pragma clang fp contract(off)") >= 4


def test_the_entry_points_run_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_predictive_q.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_predictive_q` and started as an ordinary child process: both forms, every variance
    null in turn, duplicates, both entry points, a call that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_predictive_q_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_predictive_q"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver predictive_q: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
