"""Many non-probabilistic models in one launch per launch site (csrc/api_many.inc; bnmtf_amd.run_many with nmf_np.NMF /
nmtf_np.NMTF, the cross-validation drivers' batched=).  The list-form kernels run the single-model kernels' bodies, so every model
must end with the BITS of its own run(): the factors, every iteration's metrics and the printed I-divergences.  No tolerances."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, BnmtfError, NMF, NMTF, bnmf_gibbs_optimised, bnmf_vb_optimised, run_many
from bnmtf_amd.synthetic import generate_bnmf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "np.npz"))
GDSC = np.load(os.path.join(HERE, "golden", "gdsc.npz"))


def problem(I, J, seed, frac=0.8):
    rs = np.random.RandomState(seed)
    R = rs.rand(I, J) * 4 + 0.5
    M = (rs.rand(I, J) < frac).astype(float)
    M[:, 0] = 1; M[0, :] = 1
    return R, M


# (I, J, K): GDSC's shape; a toy; row lengths for E = 4, 8 and 16 (the column sweeps of those take E = 2); a single row; K = 1 and 256
NMF_SPECS = [(622, 138, 10), (100, 80, 5), (30, 3000, 7), (20, 6000, 5), (40, 9000, 3), (1, 50, 2), (100, 80, 1), (64, 300, 256)]
# (I, J, K, L): S chains of 5, 101, 22 and 261 passes
NMTF_SPECS = [(622, 138, 2, 2), (100, 80, 10, 10), (300, 1200, 3, 7), (200, 150, 65, 4)]


def nmf_models(specs=NMF_SPECS, verbose=False):
    out = []
    for n, (I, J, K) in enumerate(specs):
        R, M = problem(I, J, seed=n, frac=1.0 if I == 1 else 0.8)
        np.random.seed(100 + n)
        m = NMF(R, M, K, verbose=verbose)
        m.initialise("exponential" if n % 2 else "random")
        out.append(m)
    return out


def nmtf_models(specs=NMTF_SPECS, verbose=False):
    out = []
    for n, (I, J, K, L) in enumerate(specs):
        R, M = problem(I, J, seed=20 + n)
        np.random.seed(200 + n)
        m = NMTF(R, M, K, L, verbose=verbose)
        m.initialise("random", "exponential" if n % 2 else "random")
        out.append(m)
    return out


def factors(m):
    return [m.F, m.S, m.G] if isinstance(m, NMTF) else [m.U, m.V]


def same(a, b):
    for x, y in zip(factors(a), factors(b)):
        np.testing.assert_array_equal(x, y)
    assert a.all_performances == b.all_performances
    assert len(a.all_times) == len(b.all_times)


def idiv_lines(text):
    return [l for l in text.splitlines() if l.startswith("Iteration ")]


def test_nmf_list_ends_with_the_bits_of_its_own_runs(capsys):
    alone, together = nmf_models(verbose=True), nmf_models(verbose=True)
    capsys.readouterr()
    for m in alone:
        m.run(20)
    out_alone = idiv_lines(capsys.readouterr().out)
    assert run_many(together, 20) == [None] * len(together)
    out_together = idiv_lines(capsys.readouterr().out)
    assert len(out_alone) == 20 * len(alone) and out_together == out_alone
    for a, b in zip(alone, together):
        same(a, b)
        assert b._many_info[0] == len(together)
    for a, b in zip(alone, together):                # a further run of each continues to the same bits
        a.run(5); b.run(5)
        same(a, b)
        assert a.compute_I_div() == b.compute_I_div()
    capsys.readouterr()
    for m in alone + together:
        m.close()


def test_nmtf_list_ends_with_the_bits_of_its_own_runs():
    alone, together = nmtf_models(), nmtf_models()
    for m in alone:
        m.run(6)
    run_many(together, 6)
    for a, b in zip(alone, together):
        same(a, b)
    shared, uploads, _ = together[0]._many_info
    assert shared == len(together)
    # argument lists go up with the first iteration only: the sites of the longest chain (2 + 262 + 6) and their splits
    assert 0 < uploads <= 2 * (2 + 262 + 6)
    for a in alone:
        a.run(3)
    run_many(together, 3)
    for a, b in zip(alone, together):
        same(a, b)
        assert a.predict(a.M) == b.predict(b.M)
    for m in alone + together:
        m.close()


def test_mixed_call_every_kind_gets_its_own_run():
    PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)

    def build():
        R, M, _, _ = generate_bnmf(100, 80, 6, 0.1, seed_data=1, seed_mask=2)
        np.random.seed(7)
        g = bnmf_gibbs_optimised(R, M, 6, PRI, seed=11, verbose=False)
        g.initialise("random")
        g.set_small_path("always")
        R2, M2, _, _ = generate_bnmf(300, 200, 8, 0.1, seed_data=3, seed_mask=4)
        np.random.seed(8)
        v = bnmf_vb_optimised(R2, M2, 8, PRI, verbose=False)
        v.initialise("random")
        return [g, v] + nmf_models(NMF_SPECS[:2]) + nmtf_models(NMTF_SPECS[:2])
    alone, together = build(), build()
    for m in alone:
        m.run(8)
    run_many(together, 8)
    g0, g1 = alone[0], together[0]
    assert np.array_equal(g0.all_U, g1.all_U) and np.array_equal(g0.all_tau, g1.all_tau) and np.array_equal(g0.U, g1.U)
    v0, v1 = alone[1], together[1]
    for name in ("muU", "tauU", "expU", "muV", "tauV", "expV"):
        np.testing.assert_array_equal(getattr(v0, name), getattr(v1, name))
    assert v0.all_performances == v1.all_performances and v0.all_exp_tau == v1.all_exp_tau
    for a, b in zip(alone[2:], together[2:]):
        same(a, b)
    assert together[2]._many_info[0] == 4


def test_two_calls_on_identical_lists_give_the_same_bits():
    outs = []
    for _ in range(2):
        ms = nmf_models(NMF_SPECS[:3]) + nmtf_models(NMTF_SPECS[:3])
        run_many(ms, 7)
        outs.append([(factors(m), m.all_performances) for m in ms])
        for m in ms:
            m.close()
    for (fa, pa), (fb, pb) in zip(*outs):
        for x, y in zip(fa, fb):
            np.testing.assert_array_equal(x, y)
        assert pa == pb


def test_refusals():
    ms = nmf_models(NMF_SPECS[:2])
    for m in ms:
        m._push()
    L = _lib.lib()
    with pytest.raises(BnmtfError, match="given twice"):
        run_many([ms[0], ms[0]], 2)
    hs = (C.c_void_p * 2)(ms[0]._handle().value, ms[0]._handle().value)
    with pytest.raises(BnmtfError, match="given twice"):
        _lib.check(L.bnmtf_np_run_many(hs, 2, 2, None, None, None, None))
    fresh = NMF(ms[1].R, ms[1].M, 3, verbose=False)               # a handle without state
    hs = (C.c_void_p * 2)(ms[0]._handle().value, fresh._handle().value)
    with pytest.raises(BnmtfError, match="before set_state"):
        _lib.check(L.bnmtf_np_run_many(hs, 2, 2, None, None, None, None))
    hs = (C.c_void_p * 2)(ms[0]._handle().value, None)
    with pytest.raises(BnmtfError, match="null handle"):
        _lib.check(L.bnmtf_np_run_many(hs, 2, 2, None, None, None, None))
    hs = (C.c_void_p * 2)(ms[0]._handle().value, ms[1]._handle().value)
    assert L.bnmtf_np_run_many(hs, 2, 0, None, None, None, None) == 0
    if bnmtf_amd.device_count() >= 2:                           # handles of two devices
        other = NMF(ms[1].R, ms[1].M, 3, device=1, verbose=False)
        other.initialise("random"); other._push()
        hs = (C.c_void_p * 2)(ms[0]._handle().value, other._handle().value)
        with pytest.raises(BnmtfError, match="share a device"):
            _lib.check(L.bnmtf_np_run_many(hs, 2, 2, None, None, None, None))
        other.close()
    fresh.close()
    for m in ms:
        m.close()


# ---------------------------------------------------------------- the cross-validation drivers
def _cv(method, X, M, search, config, path, stream_seed, **kw):
    from bnmtf_amd.cross_validation import MatrixCrossValidation
    random.seed(stream_seed); np.random.seed(stream_seed)
    cv = MatrixCrossValidation(method=method, X=X, M=M, K=5, parameter_search=search, train_config=config, file_performance=path, **kw)
    cv.run()
    cv.fout.close()
    return cv, open(path).read()


def test_nmf_fold_table_batched(tmp_path):
    runs = []
    for batched in (False, True):
        runs.append(_cv(NMF, GDSC["ex/X_min"], GDSC["ex/M"], [{"K": 2}, {"K": 4}], {"iterations": 50, "init_UV": "ones"},
                        str(tmp_path / ("cv%d.txt" % batched)), int(G["cv/seed"]), batched=batched))
    (a, log_a), (b, log_b) = runs
    for K in (2, 4):
        perf = b.all_performances[b.JSON({"K": K})]
        np.testing.assert_allclose(np.array([perf["MSE"], perf["R^2"], perf["Rp"]]), G["cv/K%d" % K], rtol=1e-4)
    assert a.all_performances == b.all_performances and log_a == log_b


def test_nmtf_grid_cross_validation_batched(tmp_path):
    X, M = problem(622, 138, seed=5, frac=0.8)
    search = [{"K": K, "L": L} for K in (2, 4) for L in (2, 5)]
    runs = [_cv(NMTF, X, M, search, {"iterations": 20, "init_S": "exponential", "init_FG": "kmeans"}, str(tmp_path / ("t%d.txt" % b)), 3,
                batched=b) for b in (False, True)]
    assert runs[0][0].all_performances == runs[1][0].all_performances and runs[0][1] == runs[1][1]


def test_nested_cross_validation_batched(tmp_path):
    from bnmtf_amd.cross_validation import MatrixNestedCrossValidation
    X, M = problem(120, 60, seed=6, frac=0.8)
    outs = []
    for b in (False, True):
        random.seed(2); np.random.seed(2)
        files = [str(tmp_path / ("n%d_%d.txt" % (b, i))) for i in range(3)]
        n = MatrixNestedCrossValidation(NMF, X, M, 3, 1, [{"K": 2}, {"K": 3}], {"iterations": 15, "init_UV": "random"},
                                        str(tmp_path / ("nout%d.txt" % b)), files, devices=[0], batched=b)
        n.run()
        outs.append((n.all_performances, [open(f).read() for f in files]))
    assert outs[0] == outs[1]


def test_two_slots_with_seeds_batched(tmp_path):
    X, M = problem(200, 90, seed=7, frac=0.8)
    runs = [_cv(NMF, X, M, [{"K": 2}, {"K": 5}], {"iterations": 15, "init_UV": "random"}, str(tmp_path / ("s%d.txt" % b)), 4,
                devices=[0, 0], seed=1234, batched=b) for b in (False, True)]
    assert runs[0][0].all_performances == runs[1][0].all_performances and runs[0][1] == runs[1][1]
