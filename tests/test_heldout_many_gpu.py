"""run_many(..., M_tests=): held-out curves for models fitted together.  In the lock-step families (bnmf_vb_optimised,
bnmtf_vb_optimised, NMF with NMTF) the list forms of the held-out kernels join the shared launches and run the single-model
kernels' bodies, so a model's all_performances_test must be the BITS of its own run(M_test=), its trajectory untouched, and its
argument lists the same from the first iteration on.  A Gibbs model with a mask is run by its own run(M_test=) (the one-launch
kernel has no per-iteration hook), its neighbours stay batched.  No tolerances."""

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import NMF, NMTF, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_optimised, run_many
from bnmtf_amd.synthetic import generate_bnmf, generate_bnmtf

pytestmark = pytest.mark.gpu

PRI2 = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
VB_NAMES = ("muU", "tauU", "expU", "varU", "muV", "tauV", "expV", "varV")


def _mask(M, seed, frac=0.6):
    """A held-out mask inside the complement of M, topped up from M where that is too small (seed stated by the caller)."""
    rs = np.random.RandomState(seed)
    Mt = ((rs.rand(*M.shape) < frac) & (M == 0)).astype(float)
    if Mt.sum() < 20:
        Mt = (rs.rand(*M.shape) < 0.3).astype(float)
    return Mt


# the three lock-step families: models of different shapes and ranks, (constructor, names of the state, orders or None)
def _vb_models():
    out = []
    for n, (I, J, K, frac, seed) in enumerate([(300, 200, 8, 0.1, 1), (210, 150, 12, 0.3, 2), (300, 200, 40, 0.1, 3), (64, 500, 5, 0.5, 4)]):
        R, M, _, _ = generate_bnmf(I, J, min(K, 10), frac, seed_data=1, seed_mask=seed)
        np.random.seed(1000 + n)
        b = bnmf_vb_optimised(R, M, K, PRI2, verbose=False); b.initialise("random")
        out.append(b)
    return out


def _trivb_models():
    out = []
    for n, (I, J, K, L, frac, seed) in enumerate([(300, 200, 4, 3, 0.1, 1), (210, 150, 6, 9, 0.3, 2), (128, 500, 12, 5, 0.5, 3)]):
        R, M, _, _, _ = generate_bnmtf(I, J, min(K, 8), min(L, 8), frac, seed_data=1, seed_mask=seed)
        np.random.seed(1000 + n)
        b = bnmtf_vb_optimised(R, M, K, L, PRI3, verbose=False); b.initialise("random", "random")
        out.append(b)
    return out


def _np_models():
    out = []
    for n, spec in enumerate([(90, 70, 5), (60, 130, 70, 3), (130, 64, 33), (65, 50, 4, 66)]):        # NMF and NMTF mixed, ranks above 64 too
        I, J = spec[:2]
        rs = np.random.RandomState(50 + n)
        R = rs.exponential(1.0, (I, 4)) @ rs.exponential(1.0, (J, 4)).T * (1.0 + 0.1 * rs.rand(I, J)) + 0.01
        M = (rs.rand(I, J) >= 0.2).astype(float)
        M[rs.randint(I, size=J), np.arange(J)] = 1; M[np.arange(I), rs.randint(J, size=I)] = 1
        np.random.seed(1000 + n)
        if len(spec) == 4:
            b = NMTF(R, M, spec[2], spec[3], verbose=False); b.initialise("random", "random")
        else:
            b = NMF(R, M, spec[2], verbose=False); b.initialise("random")
        out.append(b)
    return out


def _orders(ms, n_iter):
    rs = np.random.RandomState(12)
    return [np.array([np.concatenate([rs.permutation(b.K * b.L), rs.permutation(b.K), rs.permutation(b.L)]) for _ in range(n_iter)], dtype=np.int32)
            for b in ms]


def _state(b):
    if isinstance(b, bnmf_vb_optimised):
        names = VB_NAMES + ("all_exp_tau", "all_elbo_terms")
    elif isinstance(b, bnmtf_vb_optimised):
        names = tuple(bnmtf_vb_optimised._NAMES) + ("all_exp_tau", "all_elbo_terms")
    elif isinstance(b, NMTF):
        names = ("F", "S", "G")
    else:
        names = ("U", "V")
    return {n: np.array(getattr(b, n)) for n in names}


def _same(a, b):
    sa, sb = _state(a), _state(b)
    for n in sa:
        np.testing.assert_array_equal(sa[n], sb[n], err_msg=n)
    assert a.all_performances == b.all_performances


FAMILIES = {"bnmf_vb": (_vb_models, False), "bnmtf_vb": (_trivb_models, True), "np": (_np_models, False)}


# ---- 5: every model with a mask ends with the curve and the bits of its own run(M_test=)

@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_models_run_together_have_the_curves_of_their_own_runs(family):
    build, takes_orders = FAMILIES[family]
    n_iter = 5
    alone, together = build(), build()
    assert len(together) >= 3
    masks = [_mask(b.M, 30 + i) for i, b in enumerate(together)]
    masks[1] = None                                     # one model without a mask, between two that have one
    orders = _orders(alone, n_iter) if takes_orders else None
    for i, b in enumerate(alone):
        if takes_orders:
            b.run(n_iter, orders=orders[i], M_test=masks[i])
        else:
            b.run(n_iter, M_test=masks[i])
    assert run_many(together, n_iter, orders=orders, M_tests=masks) == [None] * len(together)
    for i, (a, b) in enumerate(zip(alone, together)):
        _same(a, b)
        assert b._many_info[0] == len(together), b._many_info         # they really shared launches
        if masks[i] is None:
            assert not hasattr(b, "all_performances_test") and not hasattr(a, "all_performances_test")
        else:
            assert a.all_performances_test == b.all_performances_test, i
            assert len(b.all_performances_test['MSE']) == n_iter and np.isfinite(b.all_performances_test['MSE']).all()
            assert len(set(b.all_performances_test['MSE'])) == n_iter     # (a curve that moves)
    # a second call with the masks moved on: the model that had none gets one, its neighbour loses its own
    masks2 = [None, _mask(together[1].M, 77)] + masks[2:]
    for i, b in enumerate(alone):
        if takes_orders:
            b.run(n_iter, orders=orders[i], M_test=masks2[i])
        else:
            b.run(n_iter, M_test=masks2[i])
    run_many(together, n_iter, orders=orders, M_tests=masks2)
    for i, (a, b) in enumerate(zip(alone, together)):
        _same(a, b)
        assert hasattr(a, "all_performances_test") == hasattr(b, "all_performances_test") == (masks2[i] is not None)
        if masks2[i] is not None:
            assert a.all_performances_test == b.all_performances_test, i


# ---- 6: the argument lists do not change per iteration

@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_argument_lists_with_masks_are_not_uploaded_per_iteration(family):
    build, takes_orders = FAMILIES[family]
    info = []
    for n_iter in (3, 9):
        ms = build()
        masks = [_mask(b.M, 30 + i) for i, b in enumerate(ms)]
        masks[1] = None
        run_many(ms, n_iter, orders=_orders(ms, n_iter) if takes_orders else None, M_tests=masks)
        info.append(ms[0]._many_info)
    assert info[0][0] == info[1][0] == len(ms)
    assert info[0][1] == info[1][1] and info[0][1] > 0, info


# ---- 7: Gibbs models: a mask takes the model out of the one-launch batch, and only that model

def _gibbs_models(tri):
    out = []
    for n, (I, J, K, L) in enumerate([(60, 50, 3, 2), (70, 40, 4, 3), (50, 60, 5, 2)]):
        if tri:
            R, M, _, _, _ = generate_bnmtf(I, J, K, L, 0.2, seed_data=1, seed_mask=n)
            np.random.seed(500 + n)
            b = bnmtf_gibbs_optimised(R, M, K, L, PRI3, verbose=False, seed=40 + n); b.initialise("random", "random")
        else:
            R, M, _, _ = generate_bnmf(I, J, K, 0.2, seed_data=1, seed_mask=n)
            np.random.seed(500 + n)
            b = bnmf_gibbs_optimised(R, M, K, PRI2, verbose=False, seed=40 + n); b.initialise("random")
        out.append(b)
    return out


@pytest.mark.parametrize("tri", [False, True], ids=["bnmf", "bnmtf"])
def test_gibbs_models_with_a_mask_run_on_their_own(tri):
    names = ("all_F", "all_S", "all_G", "all_tau") if tri else ("all_U", "all_V", "all_tau")
    own, plain, mixed = _gibbs_models(tri), _gibbs_models(tri), _gibbs_models(tri)
    Mt = _mask(mixed[1].M, 9)
    own[1].run(6, 'draw', True, None, M_test=Mt)        # the model with the mask: its own run(M_test=)
    run_many(plain, 6)                                  # its neighbours: run_many without M_tests
    run_many(mixed, 6, M_tests=[None, Mt, None])
    for n in names:
        np.testing.assert_array_equal(getattr(mixed[1], n), getattr(own[1], n), err_msg=n)
        for i in (0, 2):
            np.testing.assert_array_equal(getattr(mixed[i], n), getattr(plain[i], n), err_msg=n)
    assert mixed[1].all_performances_test == own[1].all_performances_test
    assert mixed[1].all_performances == own[1].all_performances
    for i in (0, 2):
        assert not hasattr(mixed[i], "all_performances_test") and mixed[i].all_performances == plain[i].all_performances
    # the mask stays on the handle: without M_tests the model is refused; with an entry of None the mask goes
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        run_many(mixed, 2)
    assert "held-out mask" in str(e.value)
    run_many(mixed, 2, M_tests=[None, None, None])
    assert not hasattr(mixed[1], "all_performances_test") and "heldout=" not in mixed[1].describe()


# ---- 8: validation comes before any model's state changes

def test_bad_masks_are_refused_before_anything_runs():
    ms = _vb_models()[:2]
    R, M, _, _ = generate_bnmf(120, 80, 5, 0.2, seed_data=1, seed_mask=1)
    np.random.seed(3)
    wide = bnmf_vb_optimised(R, M, 70, PRI2, verbose=False); wide.initialise("random")        # in column blocks
    before = ms[0].expU.copy()
    good = [_mask(b.M, 5) for b in ms]
    with pytest.raises(ValueError):
        run_many(ms, 3, M_tests=good[:1])
    with pytest.raises(AssertionError):
        run_many(ms, 3, M_tests=[good[0], np.ones((3, 3))])
    with pytest.raises(AssertionError):
        run_many(ms, 3, M_tests=[good[0], np.zeros(ms[1].R.shape)])
    with pytest.raises(bnmtf_amd.BnmtfError):
        run_many(ms + [wide], 3, M_tests=good + [np.ones(R.shape)])
    np.testing.assert_array_equal(ms[0].expU, before)
    assert not hasattr(ms[0], "all_performances_test") and not hasattr(ms[0], "_many_info")
    # without a mask the wide model is still taken, by its own run()
    run_many(ms + [wide], 2, M_tests=good + [None])
    assert hasattr(ms[0], "all_performances_test") and not hasattr(wide, "all_performances_test")
