"""Host side of bnmtf_vb_observed: what the class refuses -- before any device call --, that
bnmtf_vb_optimised keeps refusing layout=, the five entry points in the header, the exports map and the binding, the claims of
tests/_obs_trivb_cases.py, and the resources of the new kernels.  No GPU needed."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, _observed, batch, bnmtf_vb_observed, bnmtf_vb_optimised

import _obs_trivb_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRI = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5
NEW = ("bnmtf_otvb_set_state", "bnmtf_otvb_get_state", "bnmtf_otvb_update", "bnmtf_otvb_exp_square_diff", "bnmtf_otvb_run")


def _model(K=2, L=3, **kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    return bnmtf_vb_observed(R, M, K, L, PRI, verbose=False, **kw)


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def test_the_class_is_a_bnmtf_vb_optimised_with_its_signature_and_api():
    assert issubclass(bnmtf_vb_observed, bnmtf_vb_optimised) and bnmtf_amd.bnmtf_vb_observed is bnmtf_vb_observed
    assert "bnmtf_vb_observed" in bnmtf_amd.__all__
    assert str(inspect.signature(bnmtf_vb_observed.__init__)) == str(inspect.signature(bnmtf_vb_optimised.__init__))
    assert bnmtf_vb_observed.run is bnmtf_vb_optimised.run and bnmtf_vb_observed.elbo is bnmtf_vb_optimised.elbo
    for name in ("initialise", "train", "update_F", "update_S", "update_G", "update_exp_F", "update_exp_S", "update_exp_G", "update_tau",
                 "update_exp_tau", "predict", "quality", "log_likelihood", "_draw_orders"):
        assert getattr(bnmtf_vb_observed, name) is getattr(bnmtf_vb_optimised, name), name
    m = _model()
    assert m._layout == 'observed' and m._blocks is None and m.is_small() is False
    tot, row, col = m.omega_counts()
    assert tot == I * J and list(row) == [J] * I and list(col) == [I] * J


def test_bnmtf_vb_optimised_keeps_refusing_layout():
    R = np.ones((I, J)); M = np.ones((I, J))
    assert "layout" not in inspect.signature(bnmtf_vb_optimised.__init__).parameters
    with pytest.raises(TypeError):
        bnmtf_vb_optimised(R, M, 2, 3, PRI, verbose=False, layout='observed')
    assert getattr(bnmtf_vb_optimised(R, M, 2, 3, PRI, verbose=False), "_layout", "dense") == 'dense'


def test_ranks_above_32_are_refused_and_32_is_taken(no_device):
    R = np.ones((40, 41)); M = np.ones((40, 41))
    for K, L, name in ((33, 4, "K = 33"), (4, 33, "L = 33"), (64, 64, "K = 64"), (0, 3, "K = 0")):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            bnmtf_vb_observed(R, M, K, L, PRI, verbose=False)
        assert name in str(e.value) and "K, L <= 32" in str(e.value) and "layout='observed'" in str(e.value) and "bnmtf_vb_observed" in str(e.value)
    assert bnmtf_vb_observed(R, M, 32, 32, PRI, verbose=False)._layout == 'observed'
    assert _observed.MAX_RANK_TRI == 32


def test_a_sharded_model_is_refused_at_construction(no_device):
    R = np.ones((I, J)); M = np.ones((I, J))
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_vb_observed(R, M, 2, 3, PRI, verbose=False, rank=0, world=2, comm_id=bytes(128))
    assert "layout='observed'" in str(e.value) and "world = 1" in str(e.value)


def test_the_reference_assertions_come_first(no_device):
    with pytest.raises(AssertionError) as e:
        bnmtf_vb_observed(np.ones((2, 3)), np.ones((3, 2)), 2, 2, PRI, verbose=False)
    assert str(e.value) == "Input matrix R is not of the same size as the indicator matrix M: (2, 3) and (3, 2) respectively."
    M = np.ones((3, 3)); M[1] = 0
    with pytest.raises(AssertionError) as e:
        bnmtf_vb_observed(np.ones((3, 3)), M, 2, 2, PRI, verbose=False)
    assert str(e.value) == "Fully unobserved row in R, row 1."


def test_M_test_is_refused_before_any_device_call(no_device):
    m = _model()
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        m.run(2, M_test=Mt)
    assert "M_test" in str(e.value) and "layout='observed'" in str(e.value)
    assert not hasattr(m, "all_performances_test")


def test_the_dense_layouts_switches_and_sums_are_refused(no_device):
    m = _model()
    for call, name in ((lambda: m.masked_sums(0), "masked_sums"), (lambda: m.column_maxima(0), "column_maxima"),
                       (lambda: m.set_sweep_path(False), "set_sweep_path"), (lambda: m.set_small_path(False), "set_small_path"),
                       (lambda: m.set_profiling(True), "set_profiling")):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            call()
        assert name in str(e.value) and "layout='observed'" in str(e.value)
    assert m.is_small() is False


def test_run_many_and_the_pools_refuse_the_model(no_device):
    m = _model()
    d = bnmtf_vb_optimised(m.R, m.M, 2, 3, PRI, verbose=False)
    assert batch.takes(m)                                  # (it reaches the layout's refusal, not the TypeError of a foreign run())
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([d, m], 3)
    assert "layout='observed'" in str(e.value) and "model 1" in str(e.value)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([m], 3, orders=[TC.orders(2, 3, 3, False)])
    assert "layout='observed'" in str(e.value) and "model 0" in str(e.value)


def test_run_draws_the_parents_shuffles(monkeypatch):
    """run() consumes random.shuffle exactly as bnmtf_vb_optimised.run: the same orders reach the device call, once per call."""
    import random
    seen = {}
    for cls in (bnmtf_vb_observed, bnmtf_vb_optimised):
        R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
        m = cls(R, M, 2, 3, PRI, verbose=False)
        monkeypatch.setattr(m, "_push", lambda: None)
        monkeypatch.setattr(m, "_run_device", lambda it, orders, *rest, _c=cls: seen.setdefault(_c, []).append(orders.copy()))
        monkeypatch.setattr(m, "_run_finish", lambda *a: None)
        random.seed(11)
        m.run(4)
        seen[cls].append(random.random())
    a, b = seen[bnmtf_vb_observed], seen[bnmtf_vb_optimised]
    assert len(a) == 2 and a[0].shape == (4, 2 * 3 + 2 + 3) and a[0].dtype == np.int32
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_header_exports_map_and_binding_list_the_same_five_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmt?f_otvb_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(NEW)
    assert {n for n in _lib.EXPORTS if "_otvb_" in n} == set(NEW)
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    emap = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    for n in NEW:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    # every one is a function-try-block ending in the guard
    src = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "api_obs_trivb.inc")).read()
    for n in NEW:
        assert re.search(r"^int %s\([^{]*?\) try \{" % n, src, flags=re.M | re.S), n
    assert src.count("} BNMTF_ABI_GUARD") == len(NEW)
    # a null handle is an error code, not a crash
    assert lib.bnmtf_otvb_set_state(None, *([None] * 12), 1.0) == -1
    assert lib.bnmtf_otvb_get_state(None, *([None] * 12)) == -1
    assert lib.bnmtf_otvb_update(None, 0, 0, 0, 0) == -1
    assert lib.bnmtf_otvb_exp_square_diff(None, None) == -1
    assert lib.bnmtf_otvb_run(None, 1, None, None, None, None, None) == -1
    assert b"bnmtf_otri_create" in lib.bnmtf_last_error()


def test_the_cases_cover_the_edges_they_claim():
    have = {name: TC.edges_of(name) for name in TC.CASES}
    for edge, name in TC.EDGES.items():
        assert edge in have[name], (edge, name, sorted(have[name]))
    for name in TC.CASES:
        M, K, L = TC.CASES[name]()
        assert M.shape[0] <= 520 and M.shape[1] <= 520 and M.size <= 520 * 130 and 1 <= K <= 32 and 1 <= L <= 32
        assert (M.sum(axis=0) > 0).all() and (M.sum(axis=1) > 0).all(), name
        assert TC.long_units_of(name) == TC.LONG_UNITS.get(name, "0/0"), name
    for n in TC.UNIT_COUNTS:
        assert "row of %d" % n in have["rows"] and "column of %d" % n in have["cols"]
    # both register-form edges (64, 128, 256, 512 entries and one beyond) and the long form, in each direction
    for cap in (64, 256, 512):
        assert {"row of %d" % cap, "row of %d" % (cap + 1)} <= have["rows"] and {"column of %d" % cap, "column of %d" % (cap + 1)} <= have["cols"]
    assert {K * L for _, K, L in (TC.CASES[n]() for n in TC.CASES)} >= {63, 64, 65, 128, 130, 1024}
    o = TC.orders(3, 2, 4, True)
    assert o.shape == (4, 11) and all(sorted(r[:6]) == list(range(6)) and sorted(r[6:9]) == [0, 1, 2] and sorted(r[9:]) == [0, 1] for r in o)
    assert not np.array_equal(o[0], TC.orders(3, 2, 4, False)[0])
    assert TC.oracle_orders(TC.orders(3, 2, 1, False)[0], 3, 2) == ([(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], [0, 1, 2], [0, 1])


def _resources(source):
    csrc = os.path.join(ROOT, "bnmtf_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, source), "-o", os.devnull]
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
    return found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("source,kernels", [
    ("kernel_obs_vb.hip", ("obs_trivb_sweep_kernel",)),
    ("kernel_obs_tri.hip", ("obs_tri_gram_kernel",)),          # (untouched: the variational form is a sibling in the new unit)
    ("kernel_obs_trivb.hip", ("obs_tri_gram_vb_kernel", "obs_trivb_eff_kernel", "obs_mv_kernel", "obs_trivb_finish_kernel", "obs_trivb_esd_kernel", "obs_fold_kernel")),          # (obs_fold_kernel<1>: obs_common.h's fold, instantiated here)
])
def test_the_new_kernels_compile_for_gfx950_without_spills_or_scratch(source, kernels):
    found = _resources(source)
    for kernel in kernels:
        hits = [r for n, r in found.items() if kernel in n]
        assert len(hits) == 1, (kernel, sorted(found))
        r = hits[0]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
    if source == "kernel_obs_vb.hip":
        # the covariance form shares the two-factor sweep's LDS and stays in its register class: four waves per SIMD
        r = [r for n, r in found.items() if "obs_trivb_sweep_kernel" in n][0]
        two = [r for n, r in found.items() if "obs_vb_sweep_kernel" in n][0]
        assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4 and r["LDS Size [bytes/block]"] == two["LDS Size [bytes/block]"], (r, two)
    if source == "kernel_obs_tri.hip":
        assert not [n for n in found if "_vb_" in n]
    if source == "kernel_obs_trivb.hip":
        assert [r for n, r in found.items() if "obs_tri_gram_vb_kernel" in n][0]["LDS Size [bytes/block]"] == 0
