"""Many variational tri-factorisations in one device call (csrc/api_many.inc, bnmtf_amd.run_many with bnmtf_vb_optimised) --
what needs no GPU: run_many takes the class's own run() and refuses a subclass that brings its own, the entry point is declared,
exported and bound, the list forms keep the single-model kernels' register budgets, and the empty calls return at once."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib
from bnmtf_amd.batch import takes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PRIORS = dict(alpha=1.0, beta=1.0, lambdaF=1.0, lambdaS=1.0, lambdaG=1.0)


def _model(cls=bnmtf_amd.bnmtf_vb_optimised, K=2, L=3):
    R = np.ones((6, 5)); M = np.ones((6, 5))
    return cls(R, M, K, L, PRIORS, verbose=False)


class OwnRun(bnmtf_amd.bnmtf_vb_optimised):
    def run(self, iterations, orders=None):      # (a subclass with a run() of its own: run_many cannot know what it does)
        return super().run(iterations, orders)


def test_run_many_takes_the_class_and_refuses_a_subclass_with_its_own_run():
    m = _model()
    assert takes(m)
    s = _model(OwnRun)
    assert not takes(s)
    with pytest.raises(TypeError, match="bnmtf_vb_optimised.run"):
        bnmtf_amd.run_many([m, s], 3)


def test_empty_calls_return_at_once():
    assert bnmtf_amd.run_many([], 4) == []
    ms = [_model(), _model(K=3, L=2)]
    assert bnmtf_amd.run_many(ms, 0) == [None, None]
    assert not hasattr(ms[0], "all_performances")       # (run(0) of the list changes nothing)
    with pytest.raises(ValueError, match="orders"):
        bnmtf_amd.run_many(ms, 2, orders=[None])


def test_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "bnmtf_hip.h")) as f:
        assert re.search(r"BNMTF_API int bnmtf_vb_run_many\(bnmtf_handle\* hs, int n_models, int n_iter, const int32_t\* const\* orders,"
                         r"\s+double\* exptau_out,\s+double\* perf_out, double\* elbo_terms_out, double\* times_out, int\* launch_info\);", f.read())
    assert "bnmtf_vb_run_many" in _lib.EXPORTS
    getattr(bnmtf_amd.lib(), "bnmtf_vb_run_many")
    nm = subprocess.run(["nm", "-D", "--defined-only", bnmtf_amd.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT bnmtf_vb_run_many$", nm.stdout, re.M)


def test_argument_checks_without_a_device_call():
    f = bnmtf_amd.lib().bnmtf_vb_run_many
    assert f(None, 0, 5, None, None, None, None, None, None) == 0
    assert f(None, -1, 5, None, None, None, None, None, None) != 0
    assert f(None, 2, 5, None, None, None, None, None, None) != 0


def _resources(tu):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, tu), "-o", os.devnull]
    return subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


# translation unit: the kernels written once as a struct K (csrc/many.h), by K's mangled name -- one_form<K> and list_form<K>
FORMS = {
    "kernel_trivb.hip": ["14SmallProductVbE", "12MaskedColsumE", "11SSysChainVbE", "18SSysChainVbBlockedE", "11SSysPermuteE", "8TriThirdE"],
    "kernel_ssys.hip": ["8SColGramILi1EE", "8SColGramILi0EE", "9GammaPackE", "12SSysGemmBf16E", "10SSysReduceE", "5SSysBE", "12SSysResidualE"],
    "kernel_bnmtf.hip": ["11SlabProductE"],
    "kernel_misc.hip": ["8VbFinishE"],
    "kernel_sweep_vb.hip": ["8VbPiecesE"],
    "kernel_np.hip": ["7NpSweepILi2ELi16EE", "7NpSweepILi4ELi8EE", "7NpSweepILi8ELi4EE", "7NpSweepILi16ELi1EE", "13NpStatsFinishE", "14NpSmallProductE",
                      "8NpBuildPE", "7NpSPassE"],
    # (in the file's unnamed namespace)
    "kernel_heldout.hip": ["12_GLOBAL__N_1%s" % k for k in ("7HeldoutILi32ELb1EE", "7HeldoutILi64ELb1EE", "7HeldoutILi32ELb0EE", "7HeldoutILi64ELb0EE",
                                                             "9HeldoutNpILb1EE", "9HeldoutNpILb0EE", "11HeldoutFoldE")],
}
# the pairs that are still written by hand: (single-model kernel, its list form)
# (the 8 + 2-wave shape: a model whose sweeps take the 16-wave one is not batched -- api_many.inc, trivb_batchable)
PAIRS = {"kernel_sweep_vb.hip": [("sweep_vb_kernelILi1ELi8ELi2ELi1EE", "sweep_vb_manyILi1ELi8ELi2ELi1EE")]}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_list_forms_keep_the_single_model_kernels_budgets():
    """Every list form runs its single-model kernel's body under the same launch bounds: no more VGPRs than a ceiling with room
    over the single-model kernel's, and no spills where it has none (read as tests/test_kernel_resources_cpu.py reads them).  The
    two forms of a struct K share the body, so they hold the same bytes of LDS, and neither has scratch."""
    procs = {tu: _resources(tu) for tu in FORMS}
    for tu, p in procs.items():
        out = p.communicate(timeout=900)[0]
        assert p.returncode == 0, out[-2000:]
        found, name = {}, None
        for line in out.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1); found[name] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                found[name][m.group(1)] = int(m.group(2))
        pairs = [("one_formINS_%s" % k, "list_formINS_%s" % k, True) for k in FORMS[tu]] + [(a, b, False) for a, b in PAIRS.get(tu, [])]
        for single, many, shared in pairs:
            hs = [n for n in found if single in n]
            hm = [n for n in found if many in n]
            assert len(hs) == 1 and len(hm) == 1, (tu, single, many, sorted(found))
            rs, rm = found[hs[0]], found[hm[0]]
            assert rm["VGPRs"] <= max(rs["VGPRs"] + 16, 32), (hm[0], rm, rs)
            assert rm["VGPRs Spill"] <= rs["VGPRs Spill"] + 8, (hm[0], rm, rs)
            if shared:
                assert rm["LDS Size [bytes/block]"] == rs["LDS Size [bytes/block]"], (hm[0], rm, rs)
                assert rm["ScratchSize [bytes/lane]"] == 0 and rs["ScratchSize [bytes/lane]"] == 0, (hm[0], rm, rs)
