"""Host side of bnmtf_amd.fold_in: the export, the two entry points in the header, the exports map, the
binding and the Makefile, everything the function refuses -- before any device call --, what the C call refuses, the resources of
the new kernel, a sanitizer run of the new host code through a stand-alone program, and the restatements the GPU tests rely on:
their inputs meet the ambiguity cap on the fp32 restatement's chain, and its mode chain agrees with the fp64 one.  No GPU needed."""
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
                       bnmtf_vb_observed, bnmtf_vb_optimised, fold_in, nmf_icm, nmtf_icm)
import _draw_cases
import _fold_in_cases as cases

fold_module = sys.modules["bnmtf_amd.fold_in"]            # (the package's attribute of that name is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = ("bnmtf_fold_in", "bnmtf_fold_in_times")
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
        a = bnmf_gibbs_optimised(R, M, 2, PRI, seed=3, verbose=False, layout=layout)
        b = bnmtf_gibbs_optimised(R, M, 2, 3, PRI3, seed=3, verbose=False, layout=layout)
        if stored is not None:
            a.all_U, a.all_V = np.ones((stored, I, 2), dtype=np.float32), np.ones((stored, J, 2), dtype=np.float32)
            b.all_F, b.all_S, b.all_G = (np.ones((stored, I, 2), dtype=np.float32), np.ones((stored, 2, 3), dtype=np.float32),
                                         np.ones((stored, J, 3), dtype=np.float32))
            a.all_tau = b.all_tau = np.ones(max(stored, 3))
        out += [a, b]
    return out


def _others():
    """the ICM and the variational classes, their factors and tau put there by hand"""
    R, M = _dense()
    two = [nmf_icm(R, M, 2, PRI, seed=3, verbose=False), nmf_icm(R, M, 2, PRI, seed=3, verbose=False, layout='observed')]
    tri = [nmtf_icm(R, M, 2, 3, PRI3, seed=3, verbose=False)]
    for m in two:
        m.U, m.V, m.tau = np.ones((I, 2)), np.ones((J, 2)), 1.5
    for m in tri:
        m.F, m.S, m.G, m.tau = np.ones((I, 2)), np.ones((2, 3)), np.ones((J, 3)), 1.5
    vb2 = [bnmf_vb_optimised(R, M, 2, PRI, verbose=False), bnmf_vb_observed(R, M, 2, PRI, verbose=False)]
    vb3 = [bnmtf_vb_optimised(R, M, 2, 3, PRI3, verbose=False), bnmtf_vb_observed(R, M, 2, 3, PRI3, verbose=False)]
    for m in vb2:
        m.expU, m.expV, m.exptau, m._seed = np.ones((I, 2)), np.ones((J, 2)), 1.5, 3          # (the key a handle would have drawn)
    for m in vb3:
        m.expF, m.expS, m.expG, m.exptau, m._seed = np.ones((I, 2)), np.ones((2, 3)), np.ones((J, 3)), 1.5, 3
    return two + tri + vb2 + vb3


def _new(axis=0, n=2):
    """n new rows over the J columns (axis=1: n new columns over the I rows), two entries each"""
    if axis == 0:
        return Entries((n, J), np.repeat(np.arange(n), 2), np.tile([0, 3], n), np.ones(2 * n))
    return Entries((I, n), np.tile([1, 4], n), np.repeat(np.arange(n), 2), np.ones(2 * n))


def _refused(model, new, *texts, iterations=3, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        fold_in(model, new, iterations, **kw)
    assert str(e.value).startswith(type(model).__name__ + ": fold_in: "), str(e.value)
    for text in texts:
        assert text in str(e.value), (text, str(e.value))


def _all_models():
    gibbs = dict(burn_in=0, thinning=1)
    return [(m, gibbs) for m in _samplers(4)] + [(m, {}) for m in _others()]


def test_fold_in_is_exported():
    assert "fold_in" in bnmtf_amd.__all__ and callable(bnmtf_amd.fold_in) and bnmtf_amd.fold_in is fold_module.fold_in
    assert callable(fold_module.from_factors) and fold_module.MAX_RANK == 256 and fold_module.STREAM == 4
    assert bnmtf_amd.fold_in.from_factors is fold_module.from_factors


# ---------------------------------------------------------------- refusals, all before a device call
def test_the_shape_of_new_follows_the_axis(no_device):
    for m, kw in _all_models():
        _refused(m, _new(1), "with axis=0 new has shape (n_new, 5)", "(6, 2)", **kw)
        _refused(m, _new(0), "with axis=1 new has shape (6, n_new)", "(2, 5)", axis=1, **kw)
        _refused(m, _new(0), "axis is 0 (new rows) or 1 (new columns)", axis=2, **kw)
        _refused(m, (np.zeros(2), np.zeros(2)), "new is an Entries, not tuple", **kw)


def test_an_empty_unit_and_a_duplicate_entry_are_refused(no_device):
    for m, kw in _all_models():
        _refused(m, Entries((3, J), [0, 2], [1, 1], [1., 1.]), "new row 1 has no entry", **kw)
        _refused(m, Entries((I, 3), [1, 1], [0, 1], [1., 1.]), "new column 2 has no entry", axis=1, **kw)
        _refused(m, Entries((2, J), [], [], []), "new holds no entry", **kw)
        _refused(m, Entries((2, J), [0, 1, 1, 0], [1, 2, 2, 3], [1., 1., 2., 1.]), "entry (1, 2) of new is given twice", **kw)
        _refused(m, Entries((I, 2), [2, 2, 0], [1, 1, 0], [1., 1., 2.]), "entry (2, 1) of new is given twice", axis=1, **kw)


def test_burn_in_and_thinning_missing_or_superfluous(no_device):
    for m in _samplers(4):
        _refused(m, _new(), "burn_in and thinning are required for a Gibbs model")
        _refused(m, _new(), "burn_in and thinning are required", burn_in=1)
        _refused(m, _new(), "burn_in", "4 stored", burn_in=4, thinning=1)
        _refused(m, _new(), "thinning >= 1", burn_in=0, thinning=0)
    for m in _samplers(None):
        _refused(m, _new(), "no stored samples", burn_in=0, thinning=1)
    for m in _others():
        _refused(m, _new(), "burn_in and thinning select the samples of a Gibbs model", "takes neither", burn_in=0, thinning=1)
        _refused(m, _new(), "takes neither", thinning=1)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        fold_in(object(), _new(), 3)
    assert str(e.value).startswith("object: fold_in: ") and "not a model of this package" in str(e.value)


def test_unequal_rate_rows_need_lambdas(no_device):
    for m, kw in _all_models():
        first, last = "lambda" + m._FACTORS[0], "lambda" + m._FACTORS[-1]
        keep = getattr(m, first)
        uneven = np.array(np.broadcast_to(keep, (I, 2)), dtype=float); uneven[3, 1] = 0.7
        setattr(m, first, uneven)
        _refused(m, _new(), "the rows of %s differ" % first, "lambdas=", **kw)
        setattr(m, first, keep)
        keep = getattr(m, last)
        uneven = np.array(np.broadcast_to(keep, (J, keep.shape[-1] if np.ndim(keep) else 2)), dtype=float); uneven[0, 0] = 0.7
        setattr(m, last, uneven)
        _refused(m, _new(1), "the rows of %s differ" % last, "lambdas=", axis=1, **kw)
        setattr(m, last, keep)
        _refused(m, _new(), "lambdas is a scalar, [W] or [n_new][W]", lambdas=np.ones(5), **kw)
        _refused(m, _new(), "lambdas is a scalar, [W] or [n_new][W]", lambdas=np.ones((3, 2)), **kw)
        _refused(m, _new(), "lambdas holds a value that is not finite or is negative", lambdas=-1.0, **kw)
        _refused(m, _new(), "lambdas holds a value that is not finite", lambdas=np.nan, **kw)


def test_the_non_probabilistic_classes_are_sent_to_from_factors(no_device):
    R, M = _dense()
    for m in (NMF(R, M, 2, verbose=False), NMF(R, M, 2, verbose=False, layout='observed'), NMTF(R, M, 2, 3, verbose=False),
              NMTF(R, M, 2, 3, verbose=False, layout='observed')):
        _refused(m, _new(), "neither prior rates nor tau", "fold_in.from_factors")


def test_the_chain_keywords_are_checked(no_device):
    for m, kw in _all_models():
        _refused(m, _new(), "discard must lie below iterations (discard=3, iterations=3)", discard=3, **kw)
        _refused(m, _new(), "discard must lie below iterations", discard=7, **kw)
        _refused(m, _new(), "discard is an integer >= 0", discard=-1, **kw)
        _refused(m, _new(), "keep_every is an integer >= 1", keep_every=0, **kw)
        _refused(m, _new(), "keep_every is an integer >= 1", keep_every=1.5, **kw)
        _refused(m, _new(), "iterations is an integer >= 1", iterations=0, **kw)
        _refused(m, _new(), "first_iteration is an integer >= 0", first_iteration=-1, **kw)
        _refused(m, _new(), "below 2^31", first_iteration=2 ** 31 - 2, **kw)
        _refused(m, _new(), "update is 'draw'", "'mode'", "variational fold-in is not offered", update='vb', **kw)
        _refused(m, _new(), "update='mode' has one answer", "neither discard nor keep_every", update='mode', discard=1, **kw)
        _refused(m, _new(), "update='mode' has one answer", update='mode', keep_every=2, **kw)
        _refused(m, _new(), "tau is finite and positive", tau=0.0, **kw)
        _refused(m, _new(), "tau is finite and positive", tau=np.inf, **kw)
        _refused(m, _new(), "init is 'exp'", "'zero'", init='zero', **kw)
        _refused(m, _new(), "init is 'exp' or an array [n_new][W] = (2, 2)", init=np.ones((2, 3)), **kw)
        _refused(m, _new(), "init holds a value that is not finite", init=np.full((2, 2), np.nan), **kw)
        _refused(m, _new(), "init='exp' is 1 / lambda and needs positive rates", lambdas=0.0, **kw)
        _refused(m, _new(), "ids is a uint32 [n_new] = [2]", ids=[1, 2, 3], **kw)
        _refused(m, _new(), "ids is a uint32", ids=[0.5, 1.0], **kw)
        _refused(m, _new(), "seed is an integer >= 0", seed=-1, **kw)


def test_factors_that_are_not_finite_or_too_wide_are_refused(no_device):
    for m in _others():
        name = [a for a in ("V", "G", "expV", "expG") if isinstance(vars(m).get(a), np.ndarray)][0]
        keep = getattr(m, name)
        for bad in (np.nan, np.inf):
            broken = keep.copy(); broken[-1, -1] = bad
            setattr(m, name, broken)
            _refused(m, _new(), "not finite")
        setattr(m, name, np.ones((J + 1, keep.shape[1])))
        _refused(m, _new(), "do not fit each other", "6 x 5 matrix")
        setattr(m, name, keep)
    new = Entries((2, J), [0, 1], [0, 1], [1., 1.])

    def refused(text, other=np.ones((J, 2)), new=new, lambdas=1.0, tau=1.0, iterations=3, **kw):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            fold_module.from_factors(other, new, lambdas, tau, iterations, **kw)
        assert str(e.value).startswith("fold_in.from_factors: ") and text in str(e.value), (text, str(e.value))

    refused("ranks 1 .. 256 (BNMTF_FOLDIN_MAX_RANK; W=257)", other=np.ones((J, 257)))
    refused("ranks 1 .. 256", other=np.ones((J, 0)))
    refused("the fixed factor is two-dimensional", other=np.ones(J))
    refused("the fixed factor holds a value that is not finite", other=np.full((J, 2), np.inf))
    refused("with axis=0 new has shape (n_new, 4)", other=np.ones((4, 2)))
    refused("minimum_TN belongs to update='mode'", minimum_TN=0.5)
    refused("minimum_TN is a finite number >= 0", minimum_TN=-1.0, update='mode')
    refused("form is 0", form=2)
    refused("discard must lie below iterations", discard=3)
    refused("keep_every is an integer >= 1", keep_every=0)
    with pytest.raises(ValueError):
        Entries((2, J), [0, 1], [0, 1], [1., np.nan])              # (a value that is not finite never becomes an Entries)


def test_the_fixed_side_of_a_tri_factorisation_is_summed_in_index_order():
    rs = np.random.RandomState(1)
    F, S, G = rs.rand(7, 3), rs.rand(3, 4), rs.rand(5, 4)
    a0, a1 = fold_module.fixed_side((F, S, G), 0), fold_module.fixed_side((F, S, G), 1)
    assert a0.shape == (5, 3) and a1.shape == (7, 4)
    for j in range(5):
        for k in range(3):
            acc = 0.0
            for l in range(4):
                acc += G[j, l] * S[k, l]
            assert a0[j, k] == acc
    for i in range(7):
        for l in range(4):
            acc = 0.0
            for k in range(3):
                acc += F[i, k] * S[k, l]
            assert a1[i, l] == acc
    assert fold_module.fixed_side((F, G[:, :3]), 0).tobytes() == G[:, :3].tobytes() and fold_module.fixed_side((F, G[:, :3]), 1).tobytes() == F.tobytes()


# ---------------------------------------------------------------- ABI
def test_header_exports_map_and_binding_list_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    sig = (r"int device, int n_units, int m, int W, const double\* other,\s*uint64_t n, const int32_t\* unit, const int32_t\* idx, const float\* values,\s*"
           r"const double\* lambda, double tau, const double\* init, const uint32_t\* ids, uint64_t seed,\s*"
           r"int iterations, int first_iteration, int discard, int keep_every, int update, double min_x, int form,\s*"
           r"double\* first_out, double\* sum_d_out, double\* sum_d2_out, float\* samples_out")
    assert re.search(r"^BNMTF_API\s+int\s+bnmtf_fold_in\s*\(%s\);" % sig, hdr, flags=re.M)
    assert re.search(r"^BNMTF_API\s+int\s+bnmtf_fold_in_times\s*\(double\* upload_ms, double\* kernel_ms\);", hdr, flags=re.M)
    assert re.search(r"^#define BNMTF_FOLDIN_MAX_RANK 256$", hdr, flags=re.M)
    P, D, i = C.c_void_p, C.POINTER(C.c_double), C.c_int
    assert _lib._SIGS[NEW[0]] == ([i, i, i, i, P, C.c_uint64, P, P, P, P, C.c_double, P, P, C.c_uint64, i, i, i, i, i, C.c_double, i, P, P, P, P], i)
    assert _lib._SIGS[NEW[1]] == ([D, D], C.c_int)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    emap = open(os.path.join(CSRC, "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    src = open(os.path.join(CSRC, "api_foldin.inc")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and not any(t in name for t in ("_obs_", "_otri_", "_otvb_", "_onp_", "_vbo_", "_kmeans_"))
        assert any(fnmatch.fnmatchcase(name, g) for g in globs)
        assert hasattr(bnmtf_amd.lib(), name), "libbnmtf_hip.so does not export %s" % name
        assert re.search(r"^int %s\([^{]*?\) try \{" % name, src, flags=re.M | re.S)
    assert src.count("} BNMTF_ABI_GUARD") == 2 and "bnmtf_model" not in src and "handle" not in src.replace("no handle", "")
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert api.count('#include "api_foldin.inc"') == 1 and api.index('#include "api_foldin.inc"') > api.index('#include "api_top.inc"')
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bkernel_foldin\.hip\b", mk, flags=re.M) and re.search(r"^asan_foldin:", mk, flags=re.M)
    deps = re.search(r"^APIDEPS = (.*)$", mk, flags=re.M).group(1).split()
    assert {"api_predictive.inc", "api_top.inc", "api_foldin.inc"} <= set(deps)                      # every dependency list names it
    for rule in (r"build/%\.o", r"build/san/%_asan\.o", r"build/san/%_tsan\.o"):
        assert re.search(r"^%s: %%\.hip \$\(APIDEPS\)" % rule, mk, flags=re.M), rule
    kh = open(os.path.join(CSRC, "kernels.h")).read()
    assert re.search(r"\bkStreamFoldIn = 4\b", kh) and re.search(r"constexpr int kFoldInMaxRank = 256;", kh)


def test_the_c_call_answers_null_pointers_and_bad_limits_with_an_error_code():
    lib = bnmtf_amd.lib()
    p = _lib.ptr
    other = np.ones((4, 2)); lam = np.ones((3, 2)); x0 = np.ones((3, 2))
    unit = np.array([0, 1, 1, 2], dtype=np.int32); idx = np.array([3, 0, 2, 1], dtype=np.int32); val = np.ones(4, dtype=np.float32)
    ids = np.arange(3, dtype=np.uint32)
    o0, o1, o2 = np.zeros((3, 2)), np.zeros((3, 2)), np.zeros((3, 2))

    def call(nu=3, m=4, W=2, o=other, n=4, un=unit, ix=idx, v=val, l=lam, tau=1.0, x=x0, T=3, it0=0, dis=0, ke=1, upd=0, mn=0.0, form=0, a=o0, b=o1, c=o2):
        return lib.bnmtf_fold_in(0, nu, m, W, p(o), C.c_uint64(n), p(un), p(ix), p(v), p(l), tau, p(x), p(ids), C.c_uint64(5), T, it0, dis, ke, upd, mn, form,
                                 p(a), p(b), p(c), None)

    nan = other.copy(); nan[1, 1] = np.nan
    for kw, text in (({"o": None}, "null argument"), ({"un": None}, "null argument"), ({"ix": None}, "null argument"), ({"v": None}, "null argument"),
                     ({"l": None}, "null argument"), ({"x": None}, "null argument"), ({"a": None}, "null argument"), ({"b": None}, "null argument"),
                     ({"c": None}, "null argument"),
                     ({"nu": 0}, "unsupported shape"), ({"m": 0}, "unsupported shape"), ({"m": 2 ** 30 + 1}, "unsupported shape"),
                     ({"W": 0}, "unsupported shape"), ({"W": 257}, "1 <= W <= 256: BNMTF_FOLDIN_MAX_RANK"),
                     ({"n": 0}, "1 <= n < 2^31"), ({"n": 2 ** 31}, "1 <= n < 2^31"), ({"n": 2}, "every unit needs an entry"),
                     ({"T": 0}, "iterations >= 1"), ({"it0": -1}, "first_iteration >= 0"), ({"it0": 2 ** 31 - 2}, "below 2^31"),
                     ({"upd": 2}, "update is 0 (draw) or 1 (mode)"), ({"ke": 0}, "keep_every >= 1"), ({"dis": 3}, "0 <= discard < iterations"),
                     ({"dis": -1}, "0 <= discard < iterations"), ({"upd": 1, "dis": 1}, "a mode chain has one answer"),
                     ({"upd": 1, "ke": 2}, "a mode chain has one answer"), ({"form": 2}, "form is 0"), ({"form": -1}, "form is 0"),
                     ({"tau": 0.0}, "tau is positive and finite"), ({"tau": np.nan}, "tau is positive and finite"), ({"mn": -0.5}, "min_x is finite and not negative"),
                     ({"un": np.array([0, 1, 1, 3], dtype=np.int32)}, "entry 3 (3, 1) lies outside the 3 units x 4 indices"),
                     ({"ix": np.array([4, 0, 2, 1], dtype=np.int32)}, "entry 0 (0, 4) lies outside"),
                     ({"ix": np.array([3, 2, 2, 1], dtype=np.int32)}, "entry 2 (1, 2) is given twice"),
                     ({"ix": np.array([3, 2, 0, 1], dtype=np.int32)}, "the list is sorted by (unit, index): entry 2 (1, 0) follows (1, 2)"),
                     ({"un": np.array([0, 0, 2, 2], dtype=np.int32), "ix": np.array([0, 3, 0, 1], dtype=np.int32)}, "unit 1 has no entry"),
                     ({"v": np.array([1, np.inf, 1, 1], dtype=np.float32)}, "the value of entry 1 (1, 0) is not finite"),
                     ({"o": nan}, "the fixed factor holds a value that is not finite in fp32 (row 1, column 1)"),
                     ({"l": -lam}, "the prior rates are finite and not negative"), ({"x": x0 * np.inf}, "the start holds a value that is not finite")):
        assert call(**kw) == EINVAL, kw
        msg = lib.bnmtf_last_error().decode()
        assert msg.startswith(NEW[0] + ": ") and text in msg, (kw, msg)
    assert lib.bnmtf_fold_in_times(None, None) == EINVAL and lib.bnmtf_last_error().decode().startswith(NEW[1] + ": null argument")
    up, kn = C.c_double(-1.0), C.c_double(-1.0)
    assert lib.bnmtf_fold_in_times(C.byref(up), C.byref(kn)) == 0 and up.value >= 0.0 and kn.value >= 0.0


# ---------------------------------------------------------------- the kernel and the host code
def test_the_new_kernel_compiles_for_gfx950_within_the_stated_budget():
    """kernel_foldin.hip, the budget of DESIGN.md section 2.10: two instantiations of one kernel (draw, mode), no spills, no scratch.
    Each holds per wave x, lambda and a as floats (3 x 256 x 4 bytes) and the three statistics as doubles (3 x 256 x 8 bytes) in LDS
    and nothing else -- 4 waves x 9 216 = 36 864 bytes, four blocks per CU --, within 128 VGPRs: four waves per SIMD."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_foldin.hip"), "-o", os.devnull]
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
    assert len(found) == 2 and all(re.search(r"\d+foldin_kernelILi[01]E", n) for n in found), sorted(found)
    for kernel, r in found.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (kernel, r)
        assert r["LDS Size [bytes/block]"] <= 4 * (3 * 256 * 4 + 3 * 256 * 8), (kernel, r)
    src = open(os.path.join(CSRC, "kernel_foldin.hip")).read()
    assert "atomic" not in src and "mfma" not in src.lower()


def test_the_entry_point_runs_clean_under_the_address_sanitizer():
    """tests/sanitize/driver_foldin.cpp: a stand-alone program (its own main, the HIP stub as it is) compiled with
    -fsanitize=address,undefined by `make asan_foldin` and started as an ordinary child process: both forms, ids null and given,
    samples null and given, a call that fails midway, every refusal."""
    exe = os.path.join(CSRC, "build", "san", "driver_foldin_asan")
    r = subprocess.run(["make", "-C", CSRC, "asan_foldin"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "sanitize driver foldin: ok" in out and ", 0 live stub allocations" in out
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]


# ---------------------------------------------------------------- the restatements the GPU tests rely on
def test_the_cases_cover_every_launch_shape():
    a = cases.case("a")
    assert (a.m, a.W, a.n) == (1200, 3, 11) and a.counts == (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1100) and a.n % 4 == 3
    assert (a.M.sum(axis=1) == np.array(a.counts)).all() and (a.R >= 0).all() and (a.lam == 1).all()
    assert [cases.case(n).W for n, *_ in cases.SHAPES[1:]] == [1, 4, 5, 32, 64, 65, 255, 256]
    for name, m, W, counts in cases.SHAPES[1:]:
        c = cases.case(name)
        assert c.m == 83 and c.n == 9 and c.counts[:6] == (1, 7, 63, 64, 65, 83) and (c.M.sum(axis=1) == np.array(counts)).all()
    rows, cols, _ = a.new.row_major()
    assert not (np.diff(a.new.rows.astype(np.int64) * a.m + a.new.cols) > 0).all()           # (given in a shuffled order)
    assert rows.tobytes() == a.sorted.rows.tobytes() and cols.tobytes() == a.sorted.cols.tobytes()
    assert np.linalg.matrix_rank(cases.case("b32").other[:, :8] @ np.ones((8, 8))) <= 8


@pytest.mark.parametrize("name", [s[0] for s in cases.SHAPES])
def test_the_inputs_meet_the_ambiguity_cap_on_the_fp32_restatement(name):
    """what GPU tests 2 and 3 rely on: on the restatement's chain every draw is explained and at most AMBIGUITY_CAP of them have
    more than one admissible candidate"""
    c = cases.case(name)
    chain = cases.fp32_chain(c, 3, 'draw')
    e = cases.explain(c, chain)
    print("%s: draws %d unexplained %d ambiguous %d" % (name, e.draws, e.unexplained, e.ambiguous))
    assert e.draws == 3 * c.n * c.W and e.unexplained == 0
    assert e.ambiguous <= _draw_cases.AMBIGUITY_CAP * e.draws
    other = cases.fp32_chain(c, 3, 'draw', seed=cases.SEED + 1)
    assert (other != chain).any()


@pytest.mark.parametrize("name", [s[0] for s in cases.SHAPES])
def test_the_restated_mode_chain_agrees_with_the_fp64_one(name):
    """the bound of GPU test 1 on the restatement: every value within dmu of max(0, mu) conditioned on the chain's own states"""
    c = cases.case(name)
    chain = cases.fp32_chain(c, 3, 'mode')
    prev = c.x0
    worst = 0.0
    for t in range(3):
        mu, tp, dmu = cases.conditionals(c, prev, chain[t])
        assert (tp > 0).all()
        worst = max(worst, float((np.abs(chain[t] - np.maximum(0.0, mu)) / dmu).max()))
        prev = chain[t]
    print("%s: largest |x - max(0, mu)| / dmu = %.3f" % (name, worst))
    assert worst <= 1.0
    if c.W == 1:                                        # (one column: the conditional does not depend on the state, so the fp64 chain is max(0, mu))
        mu, tp, dmu = cases.conditionals(c, c.x0, chain[0])
        assert (np.abs(cases.fp64_mode_chain(c, 3) - np.maximum(0.0, mu)) <= 1e-12 * (1 + np.abs(mu))).all()
