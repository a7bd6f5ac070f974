"""Host side of bnmtf_amd.top_entries: the NumPy restatement against a brute-force loop, everything the
function refuses -- before any device call --, the export, the two entry points in the header, the exports map and the binding,
what the C call refuses, the resources of the new kernels, a sanitizer run of the new host code through a stand-alone program, and
the host memory of a call on a model too large for an I x J array.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
import sys
import tracemalloc

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, Entries, _lib, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, bnmtf_vb_optimised, nmf_icm, nmtf_icm, top_entries)
from bnmtf_amd import top_entries as _function
import _top_entries_cases as cases

top_module = sys.modules["bnmtf_amd.top_entries"]          # (the package's attribute of that name is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = ("bnmtf_top_entries", "bnmtf_top_entries_times")
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


def _others():
    """every class that is no Gibbs sampler, its factors put there by hand"""
    R, M = _dense()
    two = [nmf_icm(R, M, 2, PRI, verbose=False), nmf_icm(R, M, 2, PRI, verbose=False, layout='observed'), NMF(R, M, 2, verbose=False),
           NMF(R, M, 2, verbose=False, layout='observed')]
    tri = [nmtf_icm(R, M, 2, 3, PRI3, verbose=False), NMTF(R, M, 2, 3, verbose=False), NMTF(R, M, 2, 3, verbose=False, layout='observed')]
    for m in two:
        m.U, m.V = np.ones((I, 2)), np.ones((J, 2))
    for m in tri:
        m.F, m.S, m.G = np.ones((I, 2)), np.ones((2, 3)), np.ones((J, 3))
    vb2 = [bnmf_vb_optimised(R, M, 2, PRI, verbose=False), bnmf_vb_observed(R, M, 2, PRI, verbose=False)]
    vb3 = [bnmtf_vb_optimised(R, M, 2, 3, PRI3, verbose=False), bnmtf_vb_observed(R, M, 2, 3, PRI3, verbose=False)]
    for m in vb2:
        m.expU, m.expV = np.ones((I, 2)), np.ones((J, 2))
    for m in vb3:
        m.expF, m.expS, m.expG = np.ones((I, 2)), np.ones((2, 3)), np.ones((J, 3))
    return two + tri + vb2 + vb3


def _refused(model, n, *texts, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        top_entries(model, n, **kw)
    assert str(e.value).startswith(type(model).__name__ + ": top_entries: "), str(e.value)
    for text in texts:
        assert text in str(e.value), (text, str(e.value))


def test_top_entries_is_exported():
    assert "top_entries" in bnmtf_amd.__all__ and callable(bnmtf_amd.top_entries) and _function is top_module.top_entries
    assert callable(top_module.from_factors) and top_module.MAX_N == 128
    assert bnmtf_amd.top_entries.from_factors is top_module.from_factors


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("J_, n, K, L, largest", [(1, 1, 1, 0, True), (7, 3, 2, 0, True), (7, 3, 2, 0, False), (9, 12, 1, 1, True), (12, 4, 3, 2, False)])
def test_the_numpy_restatement_is_the_brute_force_selection(J_, n, K, L, largest):
    factors = cases.int_factors(J_, K, L, seed=J_ + n)
    ex = cases.exclusion(J_, n, seed=n)
    for rows in (None, [7, 0, 3]):
        for exclude in (None, ex):
            a = cases.restate(factors, n, rows, exclude, largest)
            b = cases.brute_force(factors, n, rows, exclude, largest)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
            cols, scores, counts = a
            assert ((cols >= 0).sum(axis=1) == counts).all() and (np.isnan(scores) == (cols < 0)).all()
    # the rows of the exclusion pattern: nothing, everything, all but one, the two ends, n left, n - 1 left
    cols, scores, counts = cases.restate(factors, n, None, ex, largest)
    assert counts[0] == min(n, J_) and counts[1] == 0 and counts[2] == min(n, 1) and counts[4] == min(n, J_) and counts[5] == min(n - 1, J_)
    assert len(ex[0]) > len(set(zip(ex[0].tolist(), ex[1].tolist())))           # (repeats in the list)
    # minus zero and zero tie: the lower column comes first either way
    Z = (np.array([[1.0]]), np.array([[0.0], [-0.0], [0.0]]))
    for lg in (True, False):
        assert cases.restate(Z, 3, largest=lg)[0].tolist() == [[0, 1, 2]] and cases.brute_force(Z, 3, largest=lg)[0].tolist() == [[0, 1, 2]]


def test_every_exact_case_has_its_tie_and_exact_scores():
    """what the GPU test relies on: integer scores below 2^53 whatever the summation order, and a tie where the order decides"""
    for seed, (J_, n, K, L) in enumerate(cases.EXACT + cases.SPLIT_CASES):
        factors = cases.int_factors(J_, K, L, seed)
        P = cases.dense_scores(factors)
        assert (P == np.round(P)).all() and P.max() < 2.0 ** 53 and P.shape == (cases.ROWS, J_)
        fsum = np.einsum('ik,jk->ij', factors[0] @ factors[1], factors[2]) if L else np.einsum('ik,jk->ij', *factors)
        assert (fsum == P).all()
        for largest in (True, False):
            tie = cases.has_boundary_tie(factors, n, cases.exclusion(J_, n, seed), largest)
            assert tie or (tie is None and J_ == 1), (J_, n, K, L, largest)
    assert any(J_ < n for J_, n, _, _ in cases.EXACT)
    assert {c[0] for c in cases.EXACT} == {1, 63, 64, 65, 200} and {c[1] for c in cases.EXACT} == {1, 5, 64, 128}
    assert {c[2] for c in cases.EXACT if not c[3]} == {1, 5, 32, 64, 65, 256}
    assert {c[2:] for c in cases.EXACT if c[3]} == {(1, 1), (5, 3), (32, 32), (33, 65), (256, 256)}


# ---------------------------------------------------------------- refusals, all before a device call
def test_n_outside_its_range_is_refused(no_device):
    for m in _samplers(4):
        for n in (0, -1, 129, 2.5, "3"):
            _refused(m, n, "1 .. 128", "BNMTF_TOP_MAX_N", burn_in=0, thinning=1)
    for m in _others():
        _refused(m, 0, "1 .. 128")
        _refused(m, 129, "1 .. 128")


def test_a_gibbs_model_without_its_samples_or_arguments_is_refused(no_device):
    for m in _samplers(None):
        _refused(m, 3, "no stored samples", "run() has not been called", burn_in=0, thinning=1)
    for m in _samplers(0):
        _refused(m, 3, "no stored samples", "store_samples=False", burn_in=0, thinning=1)
    for m in _samplers(4):
        _refused(m, 3, "burn_in", "4 stored", burn_in=4, thinning=1)
        _refused(m, 3, "burn_in", "4 stored", burn_in=9, thinning=2)
        _refused(m, 3, "burn_in", burn_in=-1, thinning=1)
        _refused(m, 3, "thinning >= 1", burn_in=0, thinning=0)
        _refused(m, 3, "thinning >= 1", burn_in=1, thinning=-2)
        _refused(m, 3, "burn_in and thinning are required")
        _refused(m, 3, "burn_in and thinning are required", burn_in=1)
        _refused(m, 3, "burn_in and thinning are required", thinning=1)


def test_burn_in_and_thinning_are_refused_for_every_other_class(no_device):
    for m in _others():
        _refused(m, 3, "burn_in and thinning select the samples of a Gibbs model", burn_in=0, thinning=1)
        _refused(m, 3, "takes neither", burn_in=0)
        _refused(m, 3, "takes neither", thinning=1)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        top_entries(object(), 3)
    assert str(e.value).startswith("object: top_entries: ") and "not a model of this package" in str(e.value)


def test_axis_rows_and_exclusions_are_checked(no_device):
    gibbs = dict(burn_in=0, thinning=1)
    for m, kw in [(m, gibbs) for m in _samplers(4)] + [(m, {}) for m in _others()]:
        _refused(m, 3, "axis is 0", "or 1", axis=2, **kw)
        _refused(m, 3, "axis is 0", axis=-1, **kw)
        _refused(m, 3, "axis is 0", axis=None, **kw)
        _refused(m, 3, "rows[1] = 6 lies outside the 6 rows", rows=[0, I], **kw)
        _refused(m, 3, "rows[0] = -1 lies outside", rows=[-1, 2], **kw)
        _refused(m, 3, "rows[1] = 5 lies outside the 5 rows", rows=[0, J], axis=1, **kw)           # (axis=1: rows index columns)
        _refused(m, 3, "distinct", "3 occurs twice", rows=[3, 1, 3], **kw)
        _refused(m, 3, "rows is one-dimensional", rows=[[0, 1]], **kw)
        _refused(m, 3, "rows holds integers", rows=[0.5, 1], **kw)
        _refused(m, 3, "rows is empty", rows=[], **kw)
        _refused(m, 3, "excluded entry 1 (6, 1) lies outside the 6 x 5 matrix", exclude=([0, I], [0, 1]), **kw)
        _refused(m, 3, "excluded entry 0 (0, -1) lies outside the 6 x 5 matrix", exclude=([0, 1], [-1, 1]), **kw)
        _refused(m, 3, "excluded entry 0 (0, 5) lies outside", exclude=([0, 1], [J, 1]), axis=1, **kw)
        _refused(m, 3, "different shapes", "(6, 6) and (6, 5)", exclude=Entries((I, J + 1), [0], [0], [1.]), **kw)
        _refused(m, 3, "different lengths: 2 and 1", exclude=([0, 1], [0]), **kw)
        _refused(m, 3, "the excluded rows holds integers", exclude=([0.5, 1], [0, 1]), **kw)
        _refused(m, 3, "exclude is 'observed'", "'training'", exclude='training', **kw)
        _refused(m, 3, "exclude is 'observed'", "int", exclude=3, **kw)


def test_factors_that_are_not_finite_or_do_not_fit_are_refused(no_device):
    for m in _others():
        names = [a for a in ("U", "V", "F", "S", "G", "expU", "expV", "expF", "expS", "expG") if isinstance(vars(m).get(a), np.ndarray)]
        assert len(names) in (2, 3)
        for bad in (np.nan, np.inf, -np.inf):
            for a in names:
                keep = getattr(m, a)
                broken = keep.copy(); broken[-1, -1] = bad
                setattr(m, a, broken)
                _refused(m, 3, "not finite", "finite scores")
                setattr(m, a, keep)
        first, last = names[0], names[-1]
        keep = getattr(m, last)
        setattr(m, last, np.ones((J, 4)))
        _refused(m, 3, "do not fit each other")
        setattr(m, last, np.ones((J + 1, keep.shape[1])))
        _refused(m, 3, "do not fit each other", "6 x 5 matrix")
        setattr(m, last, keep)
        keep = getattr(m, first)
        setattr(m, first, np.ones(I))
        _refused(m, 3, "do not fit each other")
        setattr(m, first, keep)
    for m in _samplers(4):
        getattr(m, "all_" + m._FACTORS[0])[2, 1, 1] = np.inf
        _refused(m, 3, "not finite", burn_in=0, thinning=1)


def test_from_factors_refuses_before_any_device_call(no_device):
    A, B, S = np.ones((I, 2)), np.ones((J, 2)), np.ones((2, 3))
    G = np.ones((J, 3))

    def refused(text, factors=(A, B), n=3, **kw):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            top_module.from_factors(factors, n, **kw)
        assert str(e.value).startswith("top_entries.from_factors: ") and text in str(e.value), (text, str(e.value))

    refused("(A, B) or (A, S, B), not 1 arrays", factors=(A,))
    refused("(A, B) or (A, S, B), not 4 arrays", factors=(A, S, G, G))
    refused("do not fit each other", factors=(A, S, B))            # (B's width is K, not L)
    refused("do not fit each other", factors=(A, G))
    refused("do not fit each other", factors=(A, np.ones((3, 2)), G))
    refused("two-dimensional", factors=(A[0], B))
    refused("ranks 1 .. 256", factors=(np.ones((I, 257)), np.ones((J, 257))))
    refused("ranks 1 .. 256", factors=(A, np.ones((2, 257)), np.ones((J, 257))))
    refused("ranks 1 .. 256", factors=(np.ones((I, 0)), np.ones((J, 0))))
    refused("1 .. 128", n=0)
    refused("1 .. 128", n=129)
    refused("not finite", factors=(A, np.full((J, 2), np.nan)))
    refused("factor S holds a value that is not finite", factors=(A, np.full((2, 3), np.inf), G))
    refused("rows[0] = 6 lies outside the 6 rows", rows=[I])
    refused("2 occurs twice", rows=[2, 2])
    refused("excluded entry 0 (6, 0) lies outside the 6 x 5 matrix", exclude=([I], [0]))
    refused("different shapes", exclude=Entries((I + 1, J), [0], [0], [1.]))
    refused("plain factors have no training entries", exclude='observed')
    refused("0 <= split <= 1024", split=-1)
    refused("0 <= split <= 1024", split=1025)


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    sig = (r"int device, int I, int J, int K, int L,\s*const double\* A, const double\* S, const double\* B,\s*uint64_t n_rows, const int32_t\* rows,\s*"
           r"uint64_t n_excl, const int32_t\* ex_rows, const int32_t\* ex_cols,\s*int n, int largest, int split,\s*"
           r"int32_t\* cols_out, double\* scores_out, int32_t\* counts_out")
    assert re.search(r"^BNMTF_API\s+int\s+bnmtf_top_entries\s*\(%s\);" % sig, hdr, flags=re.M)
    assert re.search(r"^BNMTF_API\s+int\s+bnmtf_top_entries_times\s*\(double\* upload_ms, double\* kernel_ms\);", hdr, flags=re.M)
    assert re.search(r"^#define BNMTF_TOP_MAX_N 128$", hdr, flags=re.M)
    P, D = C.c_void_p, C.POINTER(C.c_double)
    assert _lib._SIGS[NEW[0]] == ([C.c_int] * 5 + [P, P, P, C.c_uint64, P, C.c_uint64, P, P, C.c_int, C.c_int, C.c_int, P, P, P], C.c_int)
    assert _lib._SIGS[NEW[1]] == ([D, D], C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    src = open(os.path.join(CSRC, "api_top.inc")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and not any(t in name for t in ("_obs_", "_otri_", "_otvb_", "_onp_"))
        assert any(fnmatch.fnmatchcase(name, g) for g in globs)
        assert hasattr(bnmtf_amd.lib(), name), "libbnmtf_hip.so does not export %s" % name
        assert re.search(r"^int %s\([^{]*?\) try \{" % name, src, flags=re.M | re.S)
    assert src.count("} BNMTF_ABI_GUARD") == 2 and "bnmtf_model" not in src and "handle" not in src.replace("no handle", "")
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert api.count('#include "api_top.inc"') == 1 and api.index('#include "api_top.inc"') > api.index('#include "api_many.inc"')
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernel_top\.hip\b", mk, flags=re.M) and re.search(r"^asan_top:", mk, flags=re.M)
    deps = re.search(r"^APIDEPS = (.*)$", mk, flags=re.M).group(1).split()
    assert "api_predictive.inc" in deps and "api_top.inc" in deps                                    # every dependency list names it
    for rule in (r"build/%\.o", r"build/san/%_asan\.o", r"build/san/%_tsan\.o"):
        assert re.search(r"^%s: %%\.hip \$\(APIDEPS\)" % rule, mk, flags=re.M), rule


def test_the_c_call_answers_null_pointers_and_bad_limits_with_an_error_code():
    lib = bnmtf_amd.lib()
    A = np.ones((3, 2)); S = np.ones((2, 2)); rows = np.array([2, 0], dtype=np.int32); ex = np.zeros(2, dtype=np.int32)
    oc = np.zeros((3, 4), dtype=np.int32); osc = np.zeros((3, 4)); on = np.zeros(3, dtype=np.int32)
    p = _lib.ptr

    def call(device=0, n_i=3, n_j=3, K=2, L=0, a=A, s=None, b=A, nr=2, r=rows, ne=2, er=ex, ec=ex, n=4, largest=1, split=0, o0=oc, o1=osc, o2=on):
        return lib.bnmtf_top_entries(device, n_i, n_j, K, L, p(a), p(s), p(b), C.c_uint64(nr), p(r), C.c_uint64(ne), p(er), p(ec), n, largest, split,
                                     p(o0), p(o1), p(o2))

    nan = A.copy(); nan[1, 1] = np.nan
    for kw, text in (({"a": None}, "null argument"), ({"b": None}, "null argument"), ({"er": None}, "null argument"), ({"ec": None}, "null argument"),
                     ({"o0": None}, "null argument"), ({"o1": None}, "null argument"), ({"o2": None}, "null argument"),
                     ({"n_i": 0}, "unsupported shape"), ({"n_j": -1}, "unsupported shape"), ({"n_j": 2 ** 30 + 1}, "unsupported shape"),
                     ({"K": 0}, "unsupported shape"), ({"K": 257}, "unsupported shape"), ({"L": -1}, "unsupported shape"), ({"L": 257, "s": S}, "unsupported shape"),
                     ({"L": 2}, "S is required when L >= 1"), ({"s": S}, "null when L = 0"),
                     ({"n": 0}, "1 <= n <= 128 (BNMTF_TOP_MAX_N"), ({"n": 129}, "1 <= n <= 128"), ({"largest": 2}, "largest is 0 or 1"),
                     ({"split": -1}, "0 <= split <= 1024"), ({"split": 1025}, "0 <= split <= 1024"),
                     ({"nr": 0}, "1 <= n_rows <= I"), ({"nr": 4}, "1 <= n_rows <= I"), ({"ne": 2 ** 32}, "n_excl < 2^32"),
                     ({"r": np.array([0, 3], dtype=np.int32)}, "rows[1] = 3 lies outside the 3 rows"),
                     ({"r": np.array([1, 1], dtype=np.int32)}, "rows[1] = 1 occurs twice"),
                     ({"er": np.array([0, 3], dtype=np.int32)}, "excluded entry 1 (3, 0) lies outside the 3 x 3 matrix"),
                     ({"ec": np.array([-1, 0], dtype=np.int32)}, "excluded entry 0 (0, -1) lies outside the 3 x 3 matrix"),
                     ({"b": nan}, "not finite"), ({"a": nan, "r": np.array([1, 2], dtype=np.int32)}, "not finite")):
        assert call(**kw) == EINVAL, kw
        msg = lib.bnmtf_last_error().decode()
        assert msg.startswith(NEW[0] + ": ") and text in msg, (kw, msg)
    assert lib.bnmtf_top_entries_times(None, None) == EINVAL and lib.bnmtf_last_error().decode().startswith(NEW[1] + ": null argument")
    up, kn = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.bnmtf_top_entries_times(C.byref(up), C.byref(kn)) == 0 and up.value >= 0.0 and kn.value >= 0.0


# ---------------------------------------------------------------- the kernels and the host code
def test_the_new_kernels_compile_for_gfx950_within_the_stated_budget():
    """kernel_top.hip, the budget of DESIGN.md section 2.9: three kernels, no spills, no scratch.  top_kernel: the four waves'
    staged rows as doubles (4 x 256 x 8 bytes) and their lists (4 x 128 x 12 bytes) in LDS and nothing else -- 14 336 bytes --,
    within 80 VGPRs: six waves per SIMD.  top_merge_kernel: the lists alone (6 144 bytes), within 64 VGPRs: eight waves.
    top_fs_kernel: no LDS, within 64 VGPRs."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_top.hip"), "-o", os.devnull]
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
    budget = {"top_kernel": (80, 6, 4 * 256 * 8 + 4 * 128 * 12), "top_merge_kernel": (64, 8, 4 * 128 * 12), "top_fs_kernel": (64, 8, 0)}
    assert len(found) == 3, sorted(found)
    for kernel, (vgprs, waves, lds) in budget.items():
        hits = [r for n, r in found.items() if re.search(r"\d%sE" % kernel, n)]
        assert len(hits) == 1, (kernel, sorted(found))
        r = hits[0]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
        assert r["VGPRs"] <= vgprs and r["Occupancy [waves/SIMD]"] >= waves, (kernel, r)
        assert r["LDS Size [bytes/block]"] <= lds, (kernel, r)
    src = open(os.path.join(CSRC, "kernel_top.hip")).read()
    assert "atomic" not in src.replace("without atomics", "") and "mfma" not in src.lower()


def test_the_entry_point_runs_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_top.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_top` and started as an ordinary child process: both forms, rows null and given,
    duplicate exclusions, splits from 1 to more than there are column steps, a call that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_top_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_top"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver top: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]


# ---------------------------------------------------------------- host memory
class _StubLib(object):
    """bnmtf_top_entries as a no-op that fills its outputs: column 0 everywhere, one valid slot per row"""

    def __init__(self):
        self.calls = []

    def bnmtf_top_entries(self, device, n_i, n_j, K, L, A, S, B, n_rows, rows, n_excl, ex_rows, ex_cols, n, largest, split, cols, scores, counts):
        r = n_i if rows is None else n_rows.value
        C.memset(cols, 0, r * n * 4); C.memset(scores, 0, r * n * 8); C.memset(counts, 0, r * 4)
        self.calls.append((n_i, n_j, K, L, r, n_excl.value, n))
        return 0


def test_host_memory_stays_far_below_the_matrix(monkeypatch):
    """top_entries on an 8 192 x 8 192 Entries-built model: the peak of the call by tracemalloc stays under I J BYTES -- an
    eighth of one fp64 I x J array -- with the factors set by hand and the library's call stubbed."""
    n_i = n_j = 8192
    K = 4
    rs = np.random.RandomState(0)
    rows = np.concatenate([np.arange(n_i), rs.randint(n_i, size=9 * n_i)]).astype(np.int32)
    cols = np.concatenate([rs.permutation(n_j), rs.randint(n_j, size=9 * n_i)]).astype(np.int32)
    key = np.unique(rows.astype(np.int64) * n_j + cols)
    E = Entries((n_i, n_j), key // n_j, key % n_j, np.ones(len(key)))
    stub = _StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    m = bnmf_gibbs_optimised(E, None, K, PRI, verbose=False, layout='observed')
    m.all_U, m.all_V, m.all_tau = np.ones((3, n_i, K), dtype=np.float32), np.ones((3, n_j, K), dtype=np.float32), np.ones(3)
    tracemalloc.start()
    try:
        T = top_entries(m, 10, burn_in=1, thinning=1)
        T1 = top_entries(m, 10, burn_in=1, thinning=1, axis=1, rows=np.arange(100))
        rows_, cols_ = T.entries()
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    print("peak %.1f MB of %.1f MB" % (peak / 1e6, n_i * n_j / 1e6))
    assert peak < n_i * n_j
    assert stub.calls == [(n_i, n_j, K, 0, n_i, len(E), 10), (n_j, n_i, K, 0, 100, len(E), 10)]
    assert T.cols.shape == (n_i, 10) and T.scores.shape == (n_i, 10) and T.counts.shape == (n_i,) and T1.cols.shape == (100, 10)
    assert T.cols.dtype == np.int32 and T.scores.dtype == np.float64 and T.counts.dtype == np.int32 and T.rows.dtype == np.int32
    assert len(rows_) == len(cols_) == n_i * 10 and rows_.dtype == np.int32 and (rows_ == np.repeat(np.arange(n_i), 10)).all()
