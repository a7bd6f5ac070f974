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


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_list_forms_keep_the_single_model_kernels_budgets():
    """Every list form runs its single-model kernel's body under the same launch bounds: no more VGPRs than a ceiling with room
    over the single-model kernel's, and no spills where it has none (read as tests/test_kernel_resources_cpu.py reads them)."""
    pairs = {   # translation unit: [(single-model kernel, its list form)]
        "kernel_trivb.hip": [("small_product_vb_kernel", "small_product_vb_many"), ("masked_colsum_kernel", "masked_colsum_many"),
                             ("ssys_chain_vb_kernel", "ssys_chain_vb_many"), ("ssys_permute_kernel", "ssys_permute_many"),
                             ("ssys_chain_vb_blocked_kernel", "ssys_chain_vb_blocked_many"), ("tri_third_kernel", "tri_third_many")],
        "kernel_ssys.hip": [("scol_gram_kernelILi1ELi1EE", "scol_gram_manyILi1EE"), ("scol_gram_kernelILi0ELi1EE", "scol_gram_manyILi0EE"),
                            ("gamma_pack_kernel", "gamma_pack_many"), ("ssys_gemm_bf16_kernel", "ssys_gemm_bf16_many"),
                            ("ssys_reduce_kernel", "ssys_reduce_many"), ("ssys_b_kernel", "ssys_b_many"),
                            ("ssys_residual_kernel", "ssys_residual_many")],
        "kernel_bnmtf.hip": [("slab_product_kernel", "slab_product_many")],
        # (the 8 + 2-wave shape: a model whose sweeps take the 16-wave one is not batched -- api_many.inc, trivb_batchable)
        "kernel_sweep_vb.hip": [("sweep_vb_kernelILi1ELi8ELi2ELi1EE", "sweep_vb_manyILi1ELi8ELi2ELi1EE")],
    }
    procs = {tu: _resources(tu) for tu in pairs}
    for tu, p in procs.items():
        out = p.communicate(timeout=900)[0]
        assert p.returncode == 0, out[-2000:]
        found, name = {}, None
        for line in out.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1); found[name] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs Spill|VGPRs): (\d+)", line)
            if m and name:
                found[name][m.group(1)] = int(m.group(2))
        for single, many in pairs[tu]:
            hs = [n for n in found if single in n]
            hm = [n for n in found if many in n]
            assert len(hs) == 1 and len(hm) == 1, (tu, single, many, sorted(found))
            rs, rm = found[hs[0]], found[hm[0]]
            assert rm["VGPRs"] <= max(rs["VGPRs"] + 16, 32), (hm[0], rm, rs)
            assert rm["VGPRs Spill"] <= rs["VGPRs Spill"] + 8, (hm[0], rm, rs)
