"""Many variational tri-factorisations in one launch per launch site (csrc/api_many.inc; bnmtf_amd.run_many with
bnmtf_vb_optimised models, a batched ReplicaPool): the list-form kernels run the single-model kernels' bodies, so every model must
end with the BITS of its own run() -- the twelve q arrays, exptau, the metrics and the ELBO terms of every iteration, elbo() -- and
Python's `random` (the update orders' shuffles) must end where the runs one after the other leave it.  No tolerances."""
import ctypes as C
import random

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, NMF, NMTF, bnmf_vb_optimised, bnmtf_vb_optimised, run_many
from bnmtf_amd.cross_validation.replicas import ReplicaPool, fit_model, fit_models
from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
PRI2 = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)


def _models(specs, init_FG="random"):
    """specs: (I, J, K, L, missing fraction, mask seed); the data of a shape is the same for every mask (the folds of one matrix)"""
    out = []
    for n, (I, J, K, L, frac, seed) in enumerate(specs):
        R, M, _, _, _ = generate_bnmtf(I, J, min(K, 8), min(L, 8), frac, seed_data=1, seed_mask=seed)
        np.random.seed(1000 + n); random.seed(2000 + n)
        b = bnmtf_vb_optimised(R, M, K, L, PRI, verbose=False)
        b.initialise("random", init_FG)
        out.append(b)
    return out


def _same(a, b):
    for n in bnmtf_vb_optimised._NAMES:
        np.testing.assert_array_equal(getattr(a, n), getattr(b, n), err_msg=n)
    assert a.all_exp_tau == b.all_exp_tau
    assert a.all_performances == b.all_performances
    np.testing.assert_array_equal(a.all_elbo_terms, b.all_elbo_terms)
    assert a.exptau == b.exptau and a.alpha_s == b.alpha_s and a.beta_s == b.beta_s
    assert a.elbo() == b.elbo()


def _alone_and_together(specs, iterations, init_FG="random"):
    alone = _models(specs, init_FG); together = _models(specs, init_FG)
    random.seed(42)
    for m in alone:
        m.run(iterations)
    after_alone = random.random()
    random.seed(42)
    assert run_many(together, iterations) == [None] * len(specs)
    assert random.random() == after_alone                  # the same shuffles, drawn in the same order
    for a, b in zip(alone, together):
        _same(a, b)
    return alone, together


GREEDY = [(5, 5), (5, 6), (6, 5), (6, 6), (7, 6), (6, 7), (7, 7), (8, 7), (7, 8), (8, 8), (9, 8), (8, 9), (9, 9), (10, 9), (9, 10), (10, 10)]


@pytest.mark.parametrize("specs, init_FG", [
    ([(622, 138, 8, 8, 0.19, s) for s in (2, 3, 4)], "kmeans"),                                  # the folds of one model: one launch per site
    ([(622, 138, K, L, 0.19, 5 + i) for i, (K, L) in enumerate(GREEDY)], "random"),              # a greedy walk's (K, L): K L below and above 64
    ([(300, 200, 4, 3, 0.1, 1), (210, 150, 6, 9, 0.3, 2), (128, 500, 12, 5, 0.5, 3), (1024, 512, 32, 32, 0.1, 4)], "random"),   # shapes; a 1 024-step blocked chain
], ids=["folds", "greedy", "shapes"])
def test_models_run_together_end_with_the_bits_of_their_own_runs(specs, init_FG):
    alone, together = _alone_and_together(specs, 10, init_FG)
    shared, uploads, _ = together[0]._many_info
    assert shared == len(specs)
    assert uploads <= 4 * 26 * len(specs), together[0]._many_info      # argument lists are uploaded when they change: not per iteration
    # a second call continues where the first stopped, as run(); run() does
    random.seed(7)
    for m in alone:
        m.run(5)
    random.seed(7)
    run_many(together, 5)
    for a, b in zip(alone, together):
        _same(a, b)


def test_argument_lists_are_not_uploaded_per_iteration():
    specs = [(622, 138, K, L, 0.19, 10 + i) for i, (K, L) in enumerate(GREEDY[:8])]
    short = _models(specs); run_many(short, 4)
    long = _models(specs); run_many(long, 40)
    assert long[0]._many_info[0] == len(specs)
    assert long[0]._many_info[1] == short[0]._many_info[1], (short[0]._many_info, long[0]._many_info)     # bounded by the sites, not the iterations


def test_run_and_run_many_alternate():
    specs = [(622, 138, 6, 7, 0.19, s) for s in (2, 3)] + [(622, 138, 9, 9, 0.19, 4)]
    alone = _models(specs); mixed = _models(specs)
    random.seed(3)
    for m in alone:
        m.run(4)
    for m in alone:
        m.run(3)
    for m in alone:
        m.run(4)
    random.seed(3)
    run_many(mixed, 4)
    for m in mixed:
        m.run(3)
    run_many(mixed, 4)
    for a, b in zip(alone, mixed):
        _same(a, b)


def test_mixed_call_with_the_other_kinds():
    tri_specs = [(622, 138, 5, 6, 0.19, 2), (622, 138, 9, 8, 0.19, 3)]
    def build():
        tri = _models(tri_specs)
        R, M, _, _ = generate_bnmf(300, 120, 6, 0.2, seed_data=3, seed_mask=4)
        np.random.seed(5)
        vb = [bnmf_vb_optimised(R, M, K, PRI2, verbose=False) for K in (6, 9)]
        for m in vb:
            m.initialise("random")
        np.random.seed(6)
        nmf = NMF(R, M, 5, verbose=False); nmf.initialise("random")
        nmtf = NMTF(R, M, 3, 4, verbose=False); nmtf.initialise("random", "random")
        return [tri[0], vb[0], nmf, tri[1], nmtf, vb[1]]
    alone = build(); together = build()
    random.seed(11)
    for m in alone:
        m.run(6)
    random.seed(11)
    run_many(together, 6)
    for a, b in zip(alone, together):
        if isinstance(a, bnmtf_vb_optimised):
            _same(a, b)
        else:
            for f in ("U", "V", "F", "S", "G", "expU", "expV", "varU", "varV"):
                if hasattr(a, f):
                    np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
            assert a.all_performances == b.all_performances
    assert together[0]._many_info[0] == 2


def test_models_that_cannot_share_launches_run_one_by_one_in_the_same_call():
    specs = [(622, 138, 6, 6, 0.19, s) for s in (2, 3, 4)]
    alone = _models(specs); together = _models(specs)
    _lib.check(_lib.lib().bnmtf_set_profiling(together[1]._handle(), 1))     # per-kernel timers: this one stays out of the batch
    random.seed(1)
    for m in alone:
        m.run(5)
    random.seed(1)
    run_many(together, 5)
    for a, b in zip(alone, together):
        _same(a, b)
    assert together[0]._many_info[0] == 2
    one = _models(specs[:1])                       # a single batchable model: its own run
    random.seed(1)
    run_many(one, 5)
    _same(alone[0], one[0])
    assert one[0]._many_info[0] == 0


def test_c_entry_point_argument_checks():
    ms = _models([(100, 80, 4, 5, 0.1, 1), (100, 80, 4, 5, 0.1, 2)])
    L = _lib.lib()                          # (include/bnmtf_hip.h: BNMTF_OK 0, BNMTF_EINVAL -1, BNMTF_ESTATE -5)
    for m in ms:
        m._push()
    o = [m._draw_orders(3) for m in ms]
    ords = (C.c_void_p * 2)(*[x.ctypes.data for x in o])
    hs = (C.c_void_p * 2)(ms[0]._handle().value, ms[0]._handle().value)
    assert L.bnmtf_vb_run_many(hs, 2, 3, ords, None, None, None, None, None) == -1          # the same model twice
    hs = (C.c_void_p * 2)(ms[0]._handle().value, None)
    assert L.bnmtf_vb_run_many(hs, 2, 3, ords, None, None, None, None, None) == -1          # a null handle
    hs = (C.c_void_p * 2)(ms[0]._handle().value, ms[1]._handle().value)
    assert L.bnmtf_vb_run_many(hs, 2, 0, ords, None, None, None, None, None) == 0
    assert L.bnmtf_vb_run_many(hs, 2, -1, ords, None, None, None, None, None) == -1
    assert L.bnmtf_vb_run_many(hs, 2, 3, None, None, None, None, None, None) == -1          # no orders
    fresh = bnmtf_vb_optimised(ms[0].R, ms[0].M, 4, 5, PRI, verbose=False)
    hs = (C.c_void_p * 2)(ms[0]._handle().value, fresh._handle().value)
    assert L.bnmtf_vb_run_many(hs, 2, 3, ords, None, None, None, None, None) == -5          # no state set


def _jobs(R, M, n, iterations):
    rs = np.random.RandomState(0)
    jobs = []
    for i in range(n):
        held = (rs.rand(*M.shape) < 0.1) * M
        K, L = [(4, 4), (5, 6), (9, 8), (6, 5), (8, 9)][i % 5]
        jobs.append(dict(classifier=bnmtf_vb_optimised, args=(K, L, PRI), init={"init_S": "random", "init_FG": "kmeans"}, iterations=iterations,
                         burn_in=None, thinning=None, minimum_TN=None, M=M - held, test=held, metrics=["loglikelihood", "AIC", "MSE"], seed=10 + i))
    return jobs


def test_fit_models_gives_what_fit_model_gives():
    R, M, _, _, _ = generate_bnmtf(622, 138, 6, 6, 0.19, seed_data=3, seed_mask=4)
    jobs = _jobs(R, M, 5, 25)
    shared = {"R": np.asarray(R, dtype=float)}
    one_by_one = [fit_model(j, shared) for j in jobs]
    batch = fit_models(jobs, shared)
    for a, b in zip(one_by_one, batch):       # (the same fitted bits; the metric passes sum with fp64 atomics: equal to rounding)
        for m in a["quality"]:
            assert abs(a["quality"][m] - b["quality"][m]) <= 1e-10 * abs(a["quality"][m]), (m, a, b)
        for m in a["performance"]:
            assert abs(a["performance"][m] - b["performance"][m]) <= 1e-10 * abs(a["performance"][m]), (m, a, b)


def test_greedy_search_batched_chooses_what_unbatched_chooses(tmp_path):
    from bnmtf_amd.cross_validation.greedy_search_cross_validation import GreedySearchCrossValidation
    R, M, _, _, _ = generate_bnmtf(622, 138, 6, 6, 0.19, seed_data=1, seed_mask=2)
    out = []
    for batched in (False, True):
        random.seed(0); np.random.seed(0)
        pool = ReplicaPool(devices=[0], shared={"R": R}, batched=batched)
        cv = GreedySearchCrossValidation(classifier=bnmtf_vb_optimised, R=R, M=M, values_K=[5, 6, 7], values_L=[5, 6, 7], folds=3, priors=PRI,
                                         init_S="random", init_FG="kmeans", iterations=30, restarts=1, quality_metric="AIC",
                                         file_performance=str(tmp_path / ("perf%d.txt" % batched)), pool=pool, seed=7)
        cv.run()
        pool.close()
        out.append(cv)
    assert out[0].performances == out[1].performances
    assert out[0].average_performance == out[1].average_performance
    logs = [open(str(tmp_path / ("perf%d.txt" % batched))).read() for batched in (False, True)]
    assert logs[0] == logs[1]                  # (every fold's chosen K, L and its performances, line by line)
