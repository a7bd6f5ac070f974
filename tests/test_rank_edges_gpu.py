"""Ranks 65-256 at the edges of their column blocks (bnmtf_amd/_blocked.py; csrc: bnmf_set_column_block, bnmf_set_residual_data,
bnmf_half_sweep, bnmtf_metric_sums_wide, the S blocks of TriBlocks) against the fp64 oracle, and wide models in the batch entry
points (bnmtf_amd.run_many, ReplicaPool(batched=True)) against their own run().

The edges: K = 64 (the last single-handle rank), 65 (a last block of one column at col0 = 64), 128 (two full blocks), 129 (a third
block of one column) and 256 (four blocks: the residual operand of a block is built from the three others, csrc kMaxOtherBlocks).
The bounds are those of tests/test_wide_rank_gpu.py and tests/test_wide_tri_gpu.py."""
import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import BnmtfError, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, nmf_icm, nmtf_icm
from bnmtf_amd._blocked import block_ranges
from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf
from oracle import bnmtf_oracle as O

pytestmark = pytest.mark.gpu


def _bnmf_problem(I, J, K, seed, scale=0.3):
    """Seeded R, M (every row and column observed) and an initial U, V of rank K."""
    rs = np.random.RandomState(seed)
    R = rs.exponential(1.0, (I, 10)) @ rs.exponential(1.0, (J, 10)).T + rs.randn(I, J)
    M = (rs.uniform(size=(I, J)) >= 0.15).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return R, M, rs.exponential(scale, (I, K)), rs.exponential(scale, (J, K))


def _tri_problem(I, J, K, L, seed):
    rs = np.random.RandomState(seed)
    R = rs.exponential(1.0, (I, 5)) @ rs.exponential(1.0, (5, 4)) @ rs.exponential(1.0, (J, 4)).T + rs.normal(0, 1, (I, J))
    M = (rs.rand(I, J) >= 0.15).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1.0; M[rs.randint(0, I, J), np.arange(J)] = 1.0
    return R, M, rs.exponential(0.4, (I, K)), rs.exponential(0.4, (K, L)), rs.exponential(0.4, (J, L))


def _draws_agree(dev, ora, ranges, axis, rel):
    """First-sweep draws: at least 98 % of the elements of every block within `rel` of the oracle's (the rest: decisions on a
    rounding boundary, and what follows from them later in the sweep)."""
    d = np.abs(dev - ora) / (1e-3 + np.abs(ora))
    for (c0, c1) in ranges:
        blk = d[:, c0:c1] if axis == 1 else d[c0:c1, :]
        assert np.mean(blk < rel) > 0.98, ((c0, c1), np.mean(blk < rel))


BNMF_EDGES = [(140, 110, 64), (150, 100, 65), (130, 120, 128), (160, 95, 129), (120, 130, 256)]


@pytest.mark.parametrize("I,J,K", BNMF_EDGES, ids=["k64", "k65", "k128", "k129", "k256"])
def test_gibbs_at_the_block_edges_follows_the_oracle(I, J, K):
    """Mode updates over four iterations, the first draw sweep block by block, and the conditional-parameter hooks on both sides of
    every cut (ColumnBlocks.cond: k -> its block and its offset in the block)."""
    R, M, U0, V0 = _bnmf_problem(I, J, K, seed=K)
    pri = dict(alpha=1., beta=1., lambdaU=0.5, lambdaV=0.5)
    assert (bnmf_gibbs_optimised(R, M, K, pri, verbose=False)._blocks is None) == (K <= 64)
    # mode updates (deterministic)
    b = bnmf_gibbs_optimised(R, M, K, pri, verbose=False, seed=21)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(4, update="mode")
    o = O.BNMFGibbsOracle(R, M, K, pri, seed=21)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(4, draw=False)
    sU = max(1.0, np.abs(o.all_U[0]).max()); sV = max(1.0, np.abs(o.all_V[0]).max())
    assert np.abs(b.all_U[0] - o.all_U[0]).max() < 5e-4 * sU and np.abs(b.all_V[0] - o.all_V[0]).max() < 5e-4 * sV
    np.testing.assert_allclose(b.all_performances["MSE"], o.all_performances["MSE"], rtol=5e-4)
    np.testing.assert_allclose(b.all_tau, o.all_tau, rtol=5e-4)
    b.close()
    # the first draw sweep: the Philox column word of a block's column is its wide index, so every block draws the oracle's values
    b = bnmf_gibbs_optimised(R, M, K, pri, verbose=False, seed=21)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(2)
    o = O.BNMFGibbsOracle(R, M, K, pri, seed=21)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(1)
    for dev, ora in ((b.all_U[0], o.all_U[0]), (b.all_V[0], o.all_V[0])):
        _draws_agree(dev, ora, block_ranges(K), 1, 1e-3)
    assert abs(b.all_tau[0] / o.all_tau[0] - 1) < 1e-3
    assert abs(b.all_performances["MSE"][0] / o.all_performances["MSE"][0] - 1) < 1e-3
    b.close()
    # conditional parameters of a column on either side of a cut
    b = bnmf_gibbs_optimised(R, M, K, pri, verbose=False, seed=21)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    o = O.BNMFGibbsOracle(R, M, K, pri)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    for k in sorted({0, 63, 64, K - 1} & set(range(K))):
        tU, tV = o.tauU(k), o.tauV(k)
        np.testing.assert_allclose(b.tauU(k), tU, rtol=2e-6)
        np.testing.assert_allclose(b.tauV(k), tV, rtol=2e-6)
        # mu: absolute, in units of the cancelling terms of the numerator (fp32 contractions), as in test_wide_rank_gpu.py
        mU, mV = o.muU(tU, k), o.muV(tV, k)
        assert np.abs(b.muU(tU, k) - mU).max() < 1e-4 * (np.abs(mU).max() + 1.0), k
        assert np.abs(b.muV(tV, k) - mV).max() < 1e-4 * (np.abs(mV).max() + 1.0), k
    b.close()


@pytest.mark.parametrize("I,J,K", [(150, 100, 65), (120, 130, 256)], ids=["k65", "k256"])
def test_icm_at_the_block_edges_follows_the_oracle(I, J, K):
    """nmf_icm (_run_blocked with the ICM rule and the minimum_TN clamp) over three iterations."""
    R, M, U0, V0 = _bnmf_problem(I, J, K, seed=100 + K)
    pri = dict(alpha=1., beta=1., lambdaU=0.5, lambdaV=0.5)
    b = nmf_icm(R, M, K, pri, verbose=False)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(3, minimum_TN=0.01)
    o = O.NMFICMOracle(R, M, K, pri)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.3
    o.run(3, minimum_TN=0.01)
    np.testing.assert_allclose(b.all_tau, o.all_tau, rtol=1e-3)
    np.testing.assert_allclose(b.all_performances["MSE"], o.all_performances["MSE"], rtol=1e-3)
    assert np.abs(b.U - o.U).max() < 5e-3 * np.abs(o.U).max() and np.abs(b.V - o.V).max() < 5e-3 * np.abs(o.V).max()
    assert (b.U >= 0.01 - 1e-7).all() and (b.V >= 0.01 - 1e-7).all()
    b.close()


@pytest.mark.parametrize("I,J,K", [(150, 100, 65), (160, 95, 129), (120, 130, 256)], ids=["k65", "k129", "k256"])
def test_vb_at_the_block_edges_follows_the_oracle(I, J, K):
    """bnmf_vb_optimised from init='exp' (deterministic) over four iterations; the bounds of
    test_wide_rank_gpu.py::test_vb_trajectory_at_k70_matches_the_reference."""
    R, M, _, _ = _bnmf_problem(I, J, K, seed=200 + K)
    pri = dict(alpha=1., beta=1., lambdaU=1.0, lambdaV=1.0)
    b = bnmf_vb_optimised(R, M, K, pri, verbose=False)
    b.initialise("exp")
    o = O.BNMFVBOracle(R, M, K, pri)
    o.initialise("exp")
    assert abs(b.exptau / o.exptau - 1) < 1e-6
    b.run(4); o.run(4)
    np.testing.assert_allclose(b.all_performances["MSE"], o.all_performances["MSE"], rtol=1e-3)
    np.testing.assert_allclose(b.all_exp_tau, o.all_exp_tau, rtol=1e-3)
    np.testing.assert_allclose(b.all_elbo[1:], o.all_elbo[1:], rtol=1e-3)
    for name in ("expU", "varU", "expV"):
        ref = getattr(o, name)
        assert np.abs(getattr(b, name) - ref).max() < 3e-3 * max(1e-3, np.abs(ref).max()), name
    b.close()


TRI_EDGES = [(46, 41, 65, 3), (42, 48, 3, 65), (44, 40, 65, 65), (40, 45, 256, 4)]


@pytest.mark.parametrize("I,J,K,L", TRI_EDGES, ids=["k65l3", "k3l65", "k65l65", "k256l4"])
def test_tri_gibbs_at_the_block_edges_follows_the_oracle(I, J, K, L):
    """bnmtf_gibbs_optimised: mode updates over three iterations and the first draw sweep per block of F, of G and of S; the
    bounds of test_wide_tri_gpu.py."""
    R, M, F0, S0, G0 = _tri_problem(I, J, K, L, seed=K + 7 * L)
    pri = dict(alpha=1.0, beta=1.0, lambdaF=0.5, lambdaS=0.5, lambdaG=0.5)
    b = bnmtf_gibbs_optimised(R, M, K, L, pri, verbose=False, seed=31)
    b.F, b.S, b.G, b.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    b.run(3, update="mode")
    o = O.BNMTFGibbsOracle(R, M, K, L, pri, seed=31)
    o.F, o.S, o.G, o.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    o.run(3, draw=False)
    np.testing.assert_allclose(b.all_performances["MSE"], o.all_performances["MSE"], rtol=2e-3)
    np.testing.assert_allclose(b.all_tau, o.all_tau, rtol=5e-4)
    for name in ("all_F", "all_S", "all_G"):
        dev, ora = getattr(b, name)[0], getattr(o, name)[0]
        assert np.abs(dev - ora).max() < 2e-3 * np.abs(ora).max(), name
    b.close()
    b = bnmtf_gibbs_optimised(R, M, K, L, pri, verbose=False, seed=31)
    b.F, b.S, b.G, b.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    b.run(2)
    o = O.BNMTFGibbsOracle(R, M, K, L, pri, seed=31)
    o.F, o.S, o.G, o.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    o.run(1)
    kr, lr = block_ranges(K), block_ranges(L)
    _draws_agree(b.all_F[0], o.all_F[0], kr, 1, 2e-3)
    _draws_agree(b.all_G[0], o.all_G[0], lr, 1, 2e-3)
    for (k0, k1) in kr:
        _draws_agree(b.all_S[0][k0:k1], o.all_S[0][k0:k1], lr, 1, 2e-3)
    assert abs(b.all_tau[0] / o.all_tau[0] - 1) < 2e-3
    b.close()


def test_tri_icm_at_k65_l65_follows_the_oracle():
    I, J, K, L = 44, 40, 65, 65
    R, M, F0, S0, G0 = _tri_problem(I, J, K, L, seed=3)
    pri = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
    m = nmtf_icm(R, M, K, L, pri, verbose=False)
    m.F, m.S, m.G, m.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    m.run(3, minimum_TN=0.01)
    o = O.NMTFICMOracle(R, M, K, L, pri)
    o.F, o.S, o.G, o.tau = F0.copy(), S0.copy(), G0.copy(), 0.9
    o.run(3, minimum_TN=0.01)
    np.testing.assert_allclose(m.all_tau, o.all_tau, rtol=2e-3)
    np.testing.assert_allclose(m.all_performances["MSE"], o.all_performances["MSE"], rtol=2e-3)
    for got, ref in ((m.F, o.F), (m.S, o.S), (m.G, o.G)):
        assert np.abs(got - ref).max() < 2e-2 * np.abs(ref).max()
    m.close()


def test_rank_257_is_refused_by_every_class_that_takes_256():
    R, M, _, _ = _bnmf_problem(30, 20, 1, seed=0)
    two = dict(alpha=1., beta=1., lambdaU=1.0, lambdaV=1.0)
    tri = dict(alpha=1., beta=1., lambdaF=1.0, lambdaS=1.0, lambdaG=1.0)
    for cls in (bnmf_gibbs_optimised, nmf_icm, bnmf_vb_optimised):
        cls(R, M, 256, two, verbose=False).close()
        with pytest.raises(BnmtfError, match="K = 257 is outside what this build runs"):
            cls(R, M, 257, two, verbose=False)
    for cls in (bnmtf_gibbs_optimised, nmtf_icm):
        cls(R, M, 256, 256, tri, verbose=False).close()
        with pytest.raises(BnmtfError, match="K = 257 is outside what this build runs"):
            cls(R, M, 257, 4, tri, verbose=False)
        with pytest.raises(BnmtfError, match="L = 257 is outside what this build runs"):
            cls(R, M, 4, 257, tri, verbose=False)


# -- batched runs of wide models -------------------------------------------------------------------------------------------------
PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
TRI_PRI = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)


def _bnmf_models(specs):
    ms = []
    for (I, J, K, seed) in specs:
        R, M, _, _ = generate_bnmf(I, J, min(K, 10), 0.1, seed_data=seed, seed_mask=seed + 50)
        np.random.seed(seed)
        m = bnmf_gibbs_optimised(R, M, K, PRI, seed=seed, verbose=False)
        m.initialise("random")
        if K <= 64:
            m.set_small_path("always")
        ms.append(m)
    return ms


def test_run_many_runs_wide_bnmf_models_as_their_own_runs():
    """Two models of the one-launch path next to K = 70 and K = 130 (two and three column blocks): run_many used to hand the first
    block's handle to the batched launch, which ran that block alone and installed its [I][64] state as U, V."""
    specs = [(60, 50, 4, 1), (70, 40, 5, 2), (90, 80, 70, 3), (100, 90, 130, 4)]
    solo = _bnmf_models(specs); batch = _bnmf_models(specs)
    assert [m._blocks is None for m in batch] == [True, True, False, False]
    for m in solo:
        m.run(5)
    assert len(bnmtf_amd.run_many(batch, 5)) == len(batch)
    for a, b in zip(solo, batch):
        assert np.array_equal(a.all_U, b.all_U) and np.array_equal(a.all_V, b.all_V) and np.array_equal(a.all_tau, b.all_tau)
        assert a.all_performances == b.all_performances
        assert np.array_equal(a.U, b.U) and np.array_equal(a.V, b.V) and a.tau == b.tau
    # a second call continues the chains, with the posterior means kept beside the run
    for m in solo:
        m.run(6, store_samples=False, expectation=(2, 2))
    bnmtf_amd.run_many(batch, 6, store_samples=False, expectation=(2, 2))
    for a, b in zip(solo, batch):
        assert np.array_equal(a.U, b.U) and np.array_equal(a.V, b.V) and a.tau == b.tau and np.array_equal(a.all_tau, b.all_tau)
        for x, y in zip(a.approx_expectation(2, 2), b.approx_expectation(2, 2)):
            assert np.array_equal(x, y)
    for m in solo + batch:
        m.close()


def test_run_many_runs_wide_tri_models_as_their_own_runs():
    """A small tri-factorisation next to K = 70, L = 5: run_many used to hand the first F block's handle (a BNMF model) to
    bnmtf_gibbs_run_many, which refused it (BNMTF_ESTATE)."""
    specs = [(40, 35, 3, 4, 1), (60, 50, 70, 5, 2)]

    def build():
        ms = []
        for (I, J, K, L, seed) in specs:
            R, M, _, _, _ = generate_bnmtf(I, J, min(K, 6), min(L, 6), 0.1, seed_data=seed, seed_mask=seed + 50)
            np.random.seed(seed)
            m = bnmtf_gibbs_optimised(R, M, K, L, TRI_PRI, seed=seed, verbose=False)
            m.initialise("random", "random")
            if m._blocks is None:
                m.set_small_path("always")
            ms.append(m)
        return ms
    solo = build(); batch = build()
    assert [m._blocks is None for m in batch] == [True, False]
    for m in solo:
        m.run(4)
    assert len(bnmtf_amd.run_many(batch, 4)) == len(batch)
    for a, b in zip(solo, batch):
        assert np.array_equal(a.all_F, b.all_F) and np.array_equal(a.all_S, b.all_S) and np.array_equal(a.all_G, b.all_G)
        assert np.array_equal(a.all_tau, b.all_tau) and a.all_performances == b.all_performances
        assert np.array_equal(a.F, b.F) and np.array_equal(a.S, b.S) and np.array_equal(a.G, b.G) and a.tau == b.tau
    for m in solo:
        m.run(4, store_samples=False, expectation=(1, 2))
    bnmtf_amd.run_many(batch, 4, store_samples=False, expectation=(1, 2))
    for a, b in zip(solo, batch):
        assert np.array_equal(a.F, b.F) and np.array_equal(a.S, b.S) and np.array_equal(a.G, b.G) and a.tau == b.tau
        for x, y in zip(a.approx_expectation(1, 2), b.approx_expectation(1, 2)):
            assert np.array_equal(x, y)
    for m in solo + batch:
        m.close()


def test_run_many_runs_a_wide_vb_model_as_its_own_run():
    def build():
        ms = []
        for n, (I, J, K) in enumerate([(90, 80, 70), (80, 60, 8)]):
            R, M, _, _ = generate_bnmf(I, J, min(K, 10), 0.1, seed_data=1, seed_mask=n + 2)
            np.random.seed(1000 + n)
            m = bnmf_vb_optimised(R, M, K, PRI, verbose=False)
            m.initialise("random")
            ms.append(m)
        return ms
    solo = build(); batch = build()
    for m in solo:
        m.run(6)
    assert bnmtf_amd.run_many(batch, 6) == [None, None]
    for a, b in zip(solo, batch):
        for n in ("muU", "tauU", "expU", "varU", "muV", "tauV", "expV", "varV"):
            np.testing.assert_array_equal(getattr(a, n), getattr(b, n), err_msg=n)
        assert a.all_exp_tau == b.all_exp_tau and a.all_performances == b.all_performances and a.all_elbo == b.all_elbo
        assert a.exptau == b.exptau
    for m in solo + batch:
        m.close()


def test_batched_replica_pool_with_wide_ranks_gives_the_sequential_results():
    """A model search whose value list reaches past 64: ReplicaPool(batched=True) fits the jobs through run_many."""
    from bnmtf_amd.cross_validation.replicas import ReplicaPool, fit_model
    R, M, _, _ = generate_bnmf(80, 70, 4, 0.2, seed_data=1, seed_mask=2)
    rs = np.random.RandomState(3)
    test = ((rs.rand(80, 70) < 0.5) & (M == 0)).astype(float)
    jobs = [dict(classifier=bnmf_gibbs_optimised, args=(K, PRI), init={"init": "random"}, iterations=12, burn_in=4, thinning=2, minimum_TN=None,
                 M=M, test=test, metrics=["loglikelihood", "AIC", "MSE"], seed=100 + K) for K in (3, 65, 70)]
    seq = ReplicaPool(devices=[0], shared={"R": R}).map(fit_model, jobs)
    bat = ReplicaPool(devices=[0], shared={"R": R}, batched=True).map(fit_model, jobs)
    for a, b in zip(seq, bat):
        for k in a["quality"]:
            assert a["quality"][k] == pytest.approx(b["quality"][k], rel=1e-12)
        for k in a["performance"]:
            assert a["performance"][k] == pytest.approx(b["performance"][k], rel=1e-12)


def _expectation_then_none(m):
    """run with the posterior means kept, run again without, ask for the means: (first means, what the last call gives)."""
    m.run(8, store_samples=False, expectation=(2, 2))
    first = m.approx_expectation(2, 2)
    m.run(8, store_samples=False)
    try:
        with np.errstate(all="ignore"):
            return first, m.approx_expectation(2, 2)
    except Exception as e:
        return first, e


def test_a_run_without_expectation_leaves_no_stale_means():
    R, M, _, _ = generate_bnmf(90, 80, 6, 0.1, seed_data=5, seed_mask=6)
    np.random.seed(2)
    narrow = bnmf_gibbs_optimised(R, M, 6, PRI, seed=3, verbose=False); narrow.initialise("random")
    np.random.seed(2)
    wide = bnmf_gibbs_optimised(R, M, 70, PRI, seed=3, verbose=False); wide.initialise("random")
    _, n_after = _expectation_then_none(narrow)
    w_first, w_after = _expectation_then_none(wide)
    if isinstance(n_after, Exception):
        assert type(w_after) is type(n_after), w_after
    else:
        assert not isinstance(w_after, Exception), w_after
        assert not np.array_equal(w_after[0], w_first[0])
    # a blocked run that keeps the means gives those of its samples (the existing contract)
    np.random.seed(2)
    kept = bnmf_gibbs_optimised(R, M, 70, PRI, seed=3, verbose=False); kept.initialise("random")
    kept.run(8)
    eU, eV, et = kept.approx_expectation(2, 2)
    np.testing.assert_allclose(w_first[0], eU, rtol=1e-5, atol=1e-6); np.testing.assert_allclose(w_first[1], eV, rtol=1e-5, atol=1e-6)
    assert abs(w_first[2] / et - 1) < 1e-9
    for m in (narrow, wide, kept):
        m.close()
