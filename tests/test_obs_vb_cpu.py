"""Host side of bnmf_vb_observed: the class's signature and place beside bnmf_vb_optimised, what it
refuses -- before any device call --, and the five bnmf_vbo_* entry points in the header, the exports map and the binding.
No GPU needed."""
import fnmatch
import inspect
import os
import re

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, batch, bnmf_vb_observed, bnmf_vb_optimised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
I, J = 6, 5
NEW = ("bnmf_vbo_set_state", "bnmf_vbo_get_state", "bnmf_vbo_run", "bnmf_vbo_update", "bnmf_vbo_exp_square_diff")


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the refusals below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the refusal" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def _model(K=2, **kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    m = bnmf_vb_observed(R, M, K, PRI, verbose=False, **kw)
    for n in ("muU", "tauU", "expU", "varU"):
        setattr(m, n, np.ones((I, K)))
    for n in ("muV", "tauV", "expV", "varV"):
        setattr(m, n, np.ones((J, K)))
    m.exptau = 1.0
    return m


def test_the_signature_is_the_dense_classs_and_256_columns_run_on_one_handle(no_device):
    assert issubclass(bnmf_vb_observed, bnmf_vb_optimised) and bnmtf_amd.bnmf_vb_observed is bnmf_vb_observed and "bnmf_vb_observed" in bnmtf_amd.__all__
    want = inspect.signature(bnmf_vb_optimised.__init__)
    got = inspect.signature(bnmf_vb_observed.__init__)
    assert [(p.name, p.kind, p.default) for p in got.parameters.values()] == [(p.name, p.kind, p.default) for p in want.parameters.values()]
    assert "layout" not in got.parameters
    R = np.ones((300, 290)); M = np.ones((300, 290))
    m = bnmf_vb_observed(R, M, 256, PRI, verbose=False)
    assert m._layout == 'observed' and m._blocks is None and m._seed == 0
    assert bnmf_vb_observed(R, M, 1, PRI, verbose=False)._blocks is None and bnmf_vb_observed(R, M, 65, PRI, verbose=False)._blocks is None
    assert bnmf_vb_optimised(R, M, 256, PRI, verbose=False)._blocks is not None
    assert type(m).run is bnmf_vb_optimised.run            # (the parent's run(): what the batched entry points recognise a model by)


def test_the_parents_checks_keep_their_texts(no_device):
    with pytest.raises(AssertionError) as e:
        bnmf_vb_observed(np.ones(3), np.ones(3), 2, PRI, verbose=False)
    assert str(e.value) == "Input matrix R is not a two-dimensional array, but instead 1-dimensional."
    with pytest.raises(AssertionError) as e:
        bnmf_vb_observed(np.ones((3, 2)), np.ones((2, 3)), 2, PRI, verbose=False)
    assert str(e.value) == "Input matrix R is not of the same size as the indicator matrix M: (3, 2) and (2, 3) respectively."
    M = np.ones((3, 2)); M[1] = 0
    with pytest.raises(AssertionError) as e:
        bnmf_vb_observed(np.ones((3, 2)), M, 2, PRI, verbose=False)
    assert str(e.value) == "Fully unobserved row in R, row 1."
    with pytest.raises(AssertionError) as e:
        bnmf_vb_observed(np.ones((3, 2)), np.ones((3, 2)), 2, dict(PRI, lambdaU=np.ones((2, 2))), verbose=False)
    assert str(e.value) == "Prior matrix lambdaU has the wrong shape: (2, 2) instead of (3, 2)."
    with pytest.raises(AssertionError) as e:
        _model().initialise(init='bogus')
    assert str(e.value) == "Unrecognised init option for F,G: bogus."


def test_a_rank_above_256_and_a_sharded_model_are_refused_at_construction(no_device):
    R = np.ones((300, 290)); M = np.ones((300, 290))
    for K in (257, 0):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            bnmf_vb_observed(R, M, K, PRI, verbose=False)
        assert "K = %d" % K in str(e.value) and "K <= 256" in str(e.value) and "layout='observed'" in str(e.value) and "bnmf_vb_observed" in str(e.value)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmf_vb_observed(np.ones((I, J)), np.ones((I, J)), 2, PRI, verbose=False, rank=0, world=2, comm_id=bytes(128))
    assert "layout='observed'" in str(e.value) and "world = 1" in str(e.value)


def test_M_test_is_refused_before_any_device_call(no_device):
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    m = _model()
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        m.run(2, M_test=Mt)
    assert "M_test" in str(e.value) and "layout='observed'" in str(e.value) and "bnmf_vb_observed" in str(e.value)
    assert not hasattr(m, "all_performances_test")


def test_the_dense_layouts_hooks_and_switches_are_refused(no_device):
    m = _model()
    for call, name in ((lambda: m.masked_sums(0), "masked_sums"), (lambda: m.column_maxima(0), "column_maxima"), (lambda: m.set_sweep_path(False), "set_sweep_path"),
                       (lambda: m.set_small_path(False), "set_small_path"), (lambda: m.set_profiling(True), "set_profiling")):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            call()
        assert name in str(e.value) and "layout='observed'" in str(e.value)
    assert m.is_small() is False
    tot, row, col = m.omega_counts()
    assert tot == I * J and list(row) == [J] * I and list(col) == [I] * J


def test_run_many_refuses_the_model(no_device):
    m = _model()
    d = bnmf_vb_optimised(m.R, m.M, 2, PRI, verbose=False)
    assert batch.takes(m)                                  # (it reaches the layout's refusal, not the TypeError of a foreign run())
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([d, m], 3)
    assert "layout='observed'" in str(e.value) and "model 1" in str(e.value)


def test_header_exports_map_and_binding_list_the_same_five_names():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    declared = set(re.findall(r"^BNMTF_API\s+int\s+(bnmt?f_vbo_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(NEW)
    assert {n for n in _lib.EXPORTS if "_vbo_" in n} == set(NEW)
    assert not any("_obs_" in n for n in NEW)
    emap = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "exports.map")).read()
    globs = [g.strip() for g in re.search(r"global:([^}]*?)local:", emap, flags=re.S).group(1).replace("\n", " ").split(";") if g.strip()]
    for n in NEW:
        assert any(fnmatch.fnmatchcase(n, g) for g in globs), (n, globs)
    lib = bnmtf_amd.lib()
    for n in NEW:
        assert hasattr(lib, n), "libbnmtf_hip.so does not export %s" % n
    assert len(_lib.EXPORTS) == len(re.findall(r"^BNMTF_API\s", hdr, flags=re.M))
    # a null handle is an error code, not a crash (function-try-block guard and the handle check)
    assert lib.bnmf_vbo_set_state(None, None, None, None, None, None, None, None, None, 1.0) == -1
    assert lib.bnmf_vbo_get_state(None, None, None, None, None, None, None, None, None) == -1
    assert lib.bnmf_vbo_run(None, 1, None, None, None, None) == -1
    assert lib.bnmf_vbo_update(None, 0, 0, 0) == -1
    assert lib.bnmf_vbo_exp_square_diff(None, None) == -1
    assert b"bnmtf_obs_create" in lib.bnmtf_last_error()


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_sweep_kernel_keeps_four_waves_per_simd_without_spills():
    """obs_vb_sweep_kernel runs four waves per SIMD, i.e. in 128 VGPRs, with the register form up to 8 slots per lane (DESIGN.md
    section 2.7: 126 measured; with the fp64 erfc inlined into every form it took 135 and spilled scalars)."""
    import subprocess
    csrc = os.path.join(ROOT, "bnmtf_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "kernel_obs_vb.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in (out.stdout + out.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    hits = [r for n, r in found.items() if "obs_vb_sweep_kernel" in n]
    assert len(hits) == 1, sorted(found)
    r = hits[0]
    assert r["VGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
