"""run(..., M_test=): the held-out sums of every iteration, computed on the device by csrc/kernel_heldout.hip, against NumPy fp64
on the model's own samples (Gibbs), against predict() of a run cut short (ICM, VB), at the launch shapes where the kernel can go
wrong, and that nothing else changes when it is used -- or not used.

Tolerance.  Device and NumPy both sum fp64 products of the same fp32 values (the factors as sampled, R as the device holds it:
fp32) and differ in summation order only: at most K (+ L) terms per prediction and a few thousand entries per sum, i.e. below
1e-12 relative for sums whose terms do not cancel.  RTOL = 1e-9 leaves three decades."""
import ctypes as C

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (_lib, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_optimised, nmf_icm,
                       nmtf_icm)
from bnmtf_amd._base import metrics_from_sums

pytestmark = pytest.mark.gpu

RTOL = 1e-9
# (rates of 1: initial factors on the scale of the data's.  From Exp(10) factors the first mode / ICM sweep sets every entry to
# zero and stays there -- predictions of 0, no Rp, and sums that compare equal whatever the kernel does)
PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)
METRICS = ('MSE', 'R^2', 'Rp')


def _data(I, J, K, L=0, frac_missing=0.2, seed=3):
    rs = np.random.RandomState(seed)
    if L:
        R = rs.exponential(1.0, (I, K)) @ rs.exponential(1.0, (K, L)) @ rs.exponential(1.0, (J, L)).T
    else:
        R = rs.exponential(1.0, (I, K)) @ rs.exponential(1.0, (J, K)).T
    R = R + 0.3 * rs.randn(I, J)
    M = (rs.rand(I, J) >= frac_missing).astype(float)
    M[rs.randint(I, size=J), np.arange(J)] = 1; M[np.arange(I), rs.randint(J, size=I)] = 1      # no empty row / column
    return R, M


def _test_mask(M, frac, seed):
    """A held-out mask inside the complement of M where that has entries, topped up from M otherwise (seed stated by the caller)."""
    rs = np.random.RandomState(seed)
    Mt = ((rs.rand(*M.shape) < frac) & (M == 0)).astype(float)
    if Mt.sum() < 20:
        Mt = (rs.rand(*M.shape) < frac).astype(float)
    return Mt


def _numpy_sums(R, Mt, A, B, S=None):
    """The six sums in fp64 from fp32 factors and the fp32 R the device holds."""
    i, j = np.nonzero(np.asarray(Mt))
    r = np.asarray(R, dtype=np.float32)[i, j].astype(np.float64)
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    if S is not None:
        A = A @ np.asarray(S, dtype=np.float64)
    p = np.einsum('ek,ek->e', A[i], B[j])
    return np.array([float(len(r)), r.sum(), (r * r).sum(), p.sum(), (p * p).sum(), (r * p).sum()])


def _device_sums(model, n_iter):
    """bnmtf_get_heldout through ctypes: [n_iter][6]."""
    out = np.zeros((n_iter, 6))
    _lib.check(_lib.lib().bnmtf_get_heldout(model._handle(), C.c_int(n_iter), out.ctypes.data_as(C.c_void_p)))
    return out


def _check_against_samples(model, R, Mt, n_iter, tri):
    dev = _device_sums(model, n_iter)
    for t in range(n_iter):
        if tri:
            ref = _numpy_sums(R, Mt, model.all_F[t], model.all_G[t], model.all_S[t])
        else:
            ref = _numpy_sums(R, Mt, model.all_U[t], model.all_V[t])
        np.testing.assert_allclose(dev[t], ref, rtol=RTOL, atol=0, err_msg="iteration %d" % t)
        assert ref[3] > 0 and ref[4] > 0, "the predictions are all zero: nothing is compared"
        if ref[0] > 2:
            want = metrics_from_sums(ref)
            for m in METRICS:
                np.testing.assert_allclose(model.all_performances_test[m][t], want[m], rtol=RTOL, err_msg="%s, iteration %d" % (m, t))
    return dev


def _gibbs(R, M, K, L=0, seed=11, cls=None):
    np.random.seed(seed)
    if L:
        b = (cls or bnmtf_gibbs_optimised)(R, M, K, L, PRI3, verbose=False, seed=seed)
        b.initialise('random', 'random')
    else:
        b = (cls or bnmf_gibbs_optimised)(R, M, K, PRI2, verbose=False, seed=seed)
        b.initialise('random')
    return b


# ---- 1: the entry point of the feature

def test_run_with_M_test_returns_one_entry_per_iteration_and_metric():
    R, M = _data(120, 90, 4)
    Mt = _test_mask(M, 0.5, seed=1)
    b = _gibbs(R, M, 4)
    b.run(5, M_test=Mt)
    assert sorted(b.all_performances_test) == sorted(METRICS)
    for m in METRICS:
        assert len(b.all_performances_test[m]) == 5 and np.isfinite(b.all_performances_test[m]).all()
    assert "heldout=%d" % int(Mt.sum()) in b.describe()


# ---- 2: against the model's own samples (Gibbs, draw and mode)

@pytest.mark.parametrize("update", ["draw", "mode"])
@pytest.mark.parametrize("tri", [False, True], ids=["bnmf", "bnmtf"])
def test_every_iteration_matches_numpy_on_the_stored_samples(update, tri):
    I, J, K, L = 150, 110, 6, (4 if tri else 0)
    R, M = _data(I, J, K, L)
    Mt = _test_mask(M, 0.6, seed=2)                     # mask seed 2
    b = _gibbs(R, M, K, L)
    b.run(6, update=update, store_samples=True, M_test=Mt)
    _check_against_samples(b, R, Mt, 6, tri)
    # and asking for more iterations than the last run call recorded is a state error
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        _device_sums(b, 7)
    assert "error -5" in str(e.value)


# ---- 3: ICM and VB keep no trajectory: a run cut short + predict()

def _fresh(kind, R, M, K, L):
    np.random.seed(4)
    if kind == "nmf_icm":
        m = nmf_icm(R, M, K, PRI2, verbose=False); m.initialise('random')
    elif kind == "nmtf_icm":
        m = nmtf_icm(R, M, K, L, PRI3, verbose=False); m.initialise('random', 'random')
    elif kind == "bnmf_vb":
        m = bnmf_vb_optimised(R, M, K, PRI2, verbose=False); m.initialise('random')
    else:
        m = bnmtf_vb_optimised(R, M, K, L, PRI3, verbose=False); m.initialise('random', 'random')
    if hasattr(m, "set_small_path"):
        m.set_small_path(False)           # (the model with a mask runs the multi-launch path: the same fp32 summation order for both)
    return m


@pytest.mark.parametrize("kind", ["nmf_icm", "nmtf_icm", "bnmf_vb", "bnmtf_vb"])
def test_entry_t_equals_predict_after_a_run_of_t_iterations(kind):
    tri = kind in ("nmtf_icm", "bnmtf_vb")
    I, J, K, L = 140, 100, 5, (3 if tri else 0)
    R, M = _data(I, J, K, L, seed=6)
    Mt = _test_mask(M, 0.7, seed=8)                     # mask seed 8: ~2 000 entries of a rank-5 product plus noise, far from constant
    n = 4
    if kind == "bnmtf_vb":
        rs = np.random.RandomState(12)
        orders = np.array([np.concatenate([rs.permutation(K * L), rs.permutation(K), rs.permutation(L)]) for _ in range(n)], dtype=np.int32)
    a = _fresh(kind, R, M, K, L)
    if kind == "bnmtf_vb":
        a.run(n, orders=orders, M_test=Mt)
    else:
        a.run(n, M_test=Mt)
    assert len(a.all_performances_test['MSE']) == n
    for t in (1, 2, n):
        b = _fresh(kind, R, M, K, L)
        if kind == "bnmtf_vb":
            b.run(t, orders=orders[:t])
        else:
            b.run(t)
        assert not hasattr(b, "all_performances_test")
        want = b.predict(Mt)
        print(kind, t, {m: (a.all_performances_test[m][t - 1], want[m]) for m in METRICS})
        for m in METRICS:
            assert np.isfinite(want[m]) and np.isfinite(a.all_performances_test[m][t - 1]), (m, t)
            np.testing.assert_allclose(a.all_performances_test[m][t - 1], want[m], rtol=RTOL, err_msg="%s after %d iterations" % (m, t))
    assert len(set(a.all_performances_test['MSE'])) == n          # (a trajectory that moves: the entries are not one value n times)


# ---- 4: launch shapes.  The kernel's chunks: a wave step takes 64 / (KP / 4) entries of a row (8 for ranks up to 32, 4 above), a
# wave owns a row, a block four rows; there is no grid stride (one wave per row of R).

def _shape_masks(I, J, M, eps):
    rs = np.random.RandomState(21)                      # mask seed 21
    masks = {}
    one = np.zeros((I, J)); one[I - 1, J - 1] = 1
    masks["one entry"] = one
    row = np.zeros((I, J)); row[I // 2, :] = 1
    masks["one full row"] = row
    masks["full"] = np.ones((I, J))
    masks["overlapping the training mask"] = np.maximum((rs.rand(I, J) < 0.5) * M, one)
    if I >= 8:
        gaps = (rs.rand(I, J) < 0.4).astype(float)
        gaps[2, 0] = 1
        gaps[0, :] = 0; gaps[1, :] = 0; gaps[I // 2, :] = 0; gaps[I - 1, :] = 0
        masks["empty rows at the start, in the middle, at the end"] = gaps
    # entry counts around the wave step and its multiples, one count per row (rows beyond the list stay empty)
    counts = [c for c in (eps - 1, eps, eps + 1, 2 * eps - 1, 2 * eps, 2 * eps + 1, 63, 64, 65, J - 1, J) if 1 <= c <= J]
    per_row = np.zeros((I, J))
    for i, c in enumerate(counts[:I]):
        per_row[i, rs.permutation(J)[:c]] = 1
    masks["row counts around the wave step"] = per_row
    # rows in use: one below, at and one above a block's four rows and the next block's
    for rows in (3, 4, 5, 7, 8, 9):
        if rows <= I:
            blk = np.zeros((I, J)); blk[:rows, :] = (rs.rand(rows, J) < 0.5); blk[0, 0] = 1
            masks["%d rows in use" % rows] = blk
    return masks


SHAPES2 = [(1, 130, 1), (130, 1, 31), (63, 64, 32), (64, 65, 33), (65, 63, 64), (130, 130, 64), (64, 130, 31), (65, 1, 33)]
SHAPES3 = [(1, 65, 1, 31), (63, 130, 31, 32), (64, 1, 32, 33), (65, 64, 33, 64), (130, 63, 64, 1), (130, 65, 32, 31), (64, 64, 1, 64)]


@pytest.mark.parametrize("shape", SHAPES2 + SHAPES3, ids=lambda s: "x".join(str(v) for v in s))
def test_launch_shapes_match_numpy(shape):
    tri = len(shape) == 4
    I, J, K = shape[:3]; L = shape[3] if tri else 0
    R, M = _data(I, J, min(K, 4), min(L, 4) if tri else 0, frac_missing=0.2 if min(I, J) > 1 else 0.0, seed=I + J)
    b = _gibbs(R, M, K, L, seed=17)
    eps = 8 if (L if tri else K) <= 32 else 4
    for name, Mt in _shape_masks(I, J, M, eps).items():
        b.run(1, store_samples=True, M_test=Mt)
        assert "heldout=%d" % int(Mt.sum()) in b.describe(), name
        dev = _device_sums(b, 1)
        ref = _numpy_sums(R, Mt, b.all_F[0], b.all_G[0], b.all_S[0]) if tri else _numpy_sums(R, Mt, b.all_U[0], b.all_V[0])
        np.testing.assert_allclose(dev[0], ref, rtol=RTOL, atol=0, err_msg="%s: %s" % (shape, name))
        assert ref[3] > 0 and ref[4] > 0, (shape, name)


# ---- 5: no effect when unused, none on the chain when used

def _assert_same_run(a, b, names):
    for n in names:
        assert np.array_equal(np.asarray(getattr(a, n)), np.asarray(getattr(b, n))), n
    for m in METRICS:
        assert a.all_performances[m] == b.all_performances[m], m


def test_gibbs_chain_is_bit_identical_with_and_without_a_mask():
    R, M = _data(200, 170, 7, seed=9)
    Mt = _test_mask(M, 0.5, seed=5)
    runs = []
    for use in (False, True, True):
        b = _gibbs(R, M, 7, seed=23)
        b.set_small_path(False)
        b.run(5, M_test=Mt if use else None)
        runs.append(b)
    plain, held, held2 = runs
    assert not hasattr(plain, "all_performances_test")
    _assert_same_run(plain, held, ("all_U", "all_V", "all_tau"))
    assert held.all_performances_test == held2.all_performances_test            # two runs with the mask: the same bits
    # then again without: no attribute, and the chain goes on as that of a model that never had a mask
    held.run(4)
    plain.run(4)
    assert not hasattr(held, "all_performances_test") and "heldout=" not in held.describe()
    _assert_same_run(plain, held, ("all_U", "all_V", "all_tau"))
    with pytest.raises(bnmtf_amd.BnmtfError):                                   # (no mask on the handle: no record)
        _device_sums(held, 1)


def test_bnmtf_vb_trajectory_is_bit_identical_with_and_without_a_mask():
    I, J, K, L = 120, 90, 4, 3
    R, M = _data(I, J, K, L, seed=10)
    Mt = _test_mask(M, 0.5, seed=6)
    rs = np.random.RandomState(3)
    orders = np.array([np.concatenate([rs.permutation(K * L), rs.permutation(K), rs.permutation(L)]) for _ in range(4)], dtype=np.int32)
    runs = []
    for use in (False, True, True):
        np.random.seed(1)
        b = bnmtf_vb_optimised(R, M, K, L, PRI3, verbose=False); b.initialise('random', 'random')
        b.run(4, orders=orders, M_test=Mt if use else None)
        runs.append(b)
    plain, held, held2 = runs
    assert not hasattr(plain, "all_performances_test")
    _assert_same_run(plain, held, ("all_exp_tau", "expF", "expS", "expG", "all_elbo_terms"))
    assert held.all_performances_test == held2.all_performances_test


def test_run_many_refuses_a_model_that_still_has_a_mask():
    R, M = _data(60, 50, 3, seed=2)
    Mt = _test_mask(M, 0.5, seed=7)
    b = _gibbs(R, M, 3)
    b.run(2, M_test=Mt)
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        bnmtf_amd.run_many([b], 2)
    assert "held-out mask" in str(e.value)
    b.run(2)                                            # a run without M_test takes it off the handle
    bnmtf_amd.run_many([b], 2)
    assert not hasattr(b, "all_performances_test")


# ---- 6: a model of the one-launch kind

@pytest.mark.parametrize("tri", [False, True], ids=["bnmf", "bnmtf"])
def test_small_model_with_a_mask_runs_the_multi_launch_path(golden, tri):
    t = golden("toy_data.npz").case("bnmtf" if tri else "bnmf")
    R, M = t["R"], t["M"]                               # 100 x 80
    assert R.shape == (100, 80)
    Mt = _test_mask(M, 0.8, seed=13)
    b = _gibbs(R, M, 10 if not tri else 5, 5 if tri else 0, seed=31)
    assert b.is_small()
    b.run(5, store_samples=True, M_test=Mt)
    d = b.describe()
    assert not b.is_small() and "run_path=multi-launch" in d and "std_built=1" in d and "heldout=%d" % int(Mt.sum()) in d
    _check_against_samples(b, R, Mt, 5, tri)
    b.run(2)                                            # the mask gone, it is a one-launch model again
    assert b.is_small() and "heldout=" not in b.describe()
