"""Many non-probabilistic models in one device call (csrc/api_many.inc, bnmtf_amd.run_many with NMF / NMTF, the drivers'
batched=) -- what needs no GPU: the entry point is declared and exported, the list-form half sweeps keep the single-model
kernels' register budget, there is no CPU path, and the drivers plan the same folds batched or not."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib
from bnmtf_amd.cross_validation import MatrixCrossValidation, MatrixNestedCrossValidation, ParallelMatrixCrossValidation, ReplicaPool
from bnmtf_amd.cross_validation.matrix_cross_validation import fold_job, fold_jobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnmtf_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_entry_point_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "bnmtf_hip.h")) as f:
        assert re.search(r"BNMTF_API int bnmtf_np_run_many\(bnmtf_handle\* hs, int n_models, int n_iter, double\* perf_out, double\* idiv_out,"
                         r"\s+double\* times_out,\s+int\* launch_info\);", f.read())
    assert "bnmtf_np_run_many" in _lib.EXPORTS
    getattr(bnmtf_amd.lib(), "bnmtf_np_run_many")
    nm = subprocess.run(["nm", "-D", "--defined-only", bnmtf_amd.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT bnmtf_np_run_many$", nm.stdout, re.M)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_list_form_sweeps_keep_the_register_budget():
    """list_form<NpSweep<E, RB>> runs one_form<NpSweep<E, RB>>'s body (csrc/many.h) under the same __launch_bounds__(1024): at most 128 VGPRs, no spills
    (read as tests/test_kernel_resources_cpu.py reads the single-model instances)."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "kernel_np.hip"), "-o", os.devnull]
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in (out.stdout + out.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1); found[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|VGPRs): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    for sub in ("list_formINS_7NpSweepILi2ELi16EE", "list_formINS_7NpSweepILi4ELi8EE", "list_formINS_7NpSweepILi8ELi4EE", "list_formINS_7NpSweepILi16ELi1EE"):
        hits = [n for n in found if sub in n]
        assert len(hits) == 1, (sub, sorted(found))
        r = found[hits[0]]
        assert r["VGPRs"] <= 128 and r["VGPRs Spill"] == 0, (hits[0], r)
    # the list forms' names leave the single-model kernels' guard (one hit per substring) alone
    for sub in ("one_formINS_7NpSweepILi2ELi16EE", "one_formINS_7NpSweepILi4ELi8EE", "one_formINS_7NpSweepILi8ELi4EE", "one_formINS_7NpSweepILi16ELi1EE"):
        assert len([n for n in found if sub in n]) == 1, sub


def test_np_models_have_no_cpu_path_in_run_many():
    if bnmtf_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    rs = np.random.RandomState(0)
    R = rs.rand(12, 9) + 0.5; M = np.ones((12, 9))
    n = bnmtf_amd.NMF(R, M, 3, verbose=False); n.initialise("random")
    t = bnmtf_amd.NMTF(R, M, 2, 3, verbose=False); t.initialise("random", "random")
    assert bnmtf_amd.batch.takes(n) and bnmtf_amd.batch.takes(t)
    with pytest.raises(bnmtf_amd.BnmtfError):
        bnmtf_amd.run_many([n, t], 3)


def test_run_many_takes_np_models_once_initialised():
    R = np.ones((4, 3)); M = np.ones((4, 3))
    n = bnmtf_amd.NMF(R, M, 2, verbose=False)
    t = bnmtf_amd.NMTF(R, M, 2, 2, verbose=False)
    assert not bnmtf_amd.batch.takes(n) and not bnmtf_amd.batch.takes(t)
    with pytest.raises(TypeError, match="initialised"):
        bnmtf_amd.run_many([n], 2)
    n.initialise("ones"); t.initialise("ones", "ones")
    assert bnmtf_amd.batch.takes(n) and bnmtf_amd.batch.takes(t)


def test_run_many_refuses_a_subclass_with_its_own_run():
    class MyNMF(bnmtf_amd.NMF):
        def run(self, iterations):
            pass
    R = np.ones((4, 3)); M = np.ones((4, 3))
    m = MyNMF(R, M, 2, verbose=False)
    assert not bnmtf_amd.batch.takes(m)
    with pytest.raises(TypeError):
        bnmtf_amd.run_many([m], 2)


class Fake(object):
    """A model-free method: predict() reports the fold it was trained on and a draw from the global stream at train()."""
    def __init__(self, X, M, K):
        self.M, self.K = np.asarray(M), K

    def train(self, iterations):
        self.draw = np.random.rand()

    def predict(self, M_pred):
        return {"MSE": float(self.K + self.M.sum() * 1e-3 + self.draw), "n_test": float(np.asarray(M_pred).sum())}


def _data():
    rs = np.random.RandomState(1)
    X = rs.rand(14, 11) + 0.5
    M = (rs.rand(14, 11) < 0.9).astype(float)
    M[:, 0] = 1; M[0, :] = 1
    return X, M


@pytest.mark.parametrize("cls", [MatrixCrossValidation, ParallelMatrixCrossValidation])
def test_drivers_accept_batched_and_plan_the_same_folds(cls, tmp_path):
    X, M = _data()
    extra = {"P": 1} if cls is ParallelMatrixCrossValidation else {}
    plans, logs = [], []
    for batched in (False, True):
        random.seed(4); np.random.seed(4)
        cv = cls(Fake, X, M, 3, [{"K": 1}, {"K": 2}], {"iterations": 5}, str(tmp_path / ("cv%d.txt" % batched)), devices=[0],
                 batched=batched, **extra)
        assert cv.batched is batched
        plans.append([[(tr.copy(), te.copy()) for tr, te in s.folds] for s in cv._plan()])
        random.seed(4); np.random.seed(4)
        cv.run()
        cv.fout.close()
        logs.append(open(str(tmp_path / ("cv%d.txt" % batched))).read())
    for a, b in zip(*plans):
        assert len(a) == len(b) == 3
        for (tra, tea), (trb, teb) in zip(a, b):
            assert np.array_equal(tra, trb) and np.array_equal(tea, teb)
    assert logs[0] == logs[1] and "Tried parameters" in logs[0]


def test_nested_driver_accepts_batched(tmp_path):
    X, M = _data()
    logs = []
    for batched in (False, True):
        random.seed(5); np.random.seed(5)
        files = [str(tmp_path / ("in%d_%d.txt" % (batched, i))) for i in range(2)]
        n = MatrixNestedCrossValidation(Fake, X, M, 2, 1, [{"K": 1}, {"K": 2}], {"iterations": 5}, str(tmp_path / ("out%d.txt" % batched)),
                                        files, devices=[0], batched=batched)
        assert n.batched is batched
        n.run()
        logs.append([open(f).read() for f in files] + [open(str(tmp_path / ("out%d.txt" % batched))).read()])
    assert logs[0] == logs[1]


def test_fold_jobs_runs_other_methods_through_fold_job_in_job_order():
    X, M = _data()
    jobs = [dict(method=Fake, parameters={"K": k}, train=M, test=M, train_config={"iterations": 2}, seed=None if k < 3 else 11 * k)
            for k in (1, 2, 3, 4)]
    np.random.seed(9)
    one = [fold_job(j, {"X": X}) for j in jobs]
    np.random.seed(9)
    many = fold_jobs(jobs, {"X": X})
    assert one == many
    np.random.seed(9)
    with ReplicaPool(devices=[0], shared={"X": X}, batched=True) as pool:
        assert pool.map(fold_job, jobs) == one
