"""NMF.run(..., M_test=) and NMTF.run(..., M_test=): the held-out sums of every iteration of the non-probabilistic models, computed
on the device from their column-major fp32 factors (csrc/kernel_heldout.hip: heldout_np_kernel), against NumPy fp64 on the factors
pulled from the model, at the launch shapes where the kernel can go wrong, and that nothing else changes when it is used -- or
not used.

Yardstick.  NumPy in fp64 on the factors pulled from the model (the device's fp32 values, exactly representable) and the
fp32-rounded R; never predict(), whose P goes through the fp32 pass of bnmtf_np_metrics.  Device and NumPy sum fp64 products of
the same fp32 values and differ in summation order only: RTOL = 1e-9, atol 0, as tests/test_heldout_gpu.py has for the same
quantity.  Every comparison also asserts sum P > 0 and sum P^2 > 0.

Data.  R is a product of Exp(1) factors of rank min(K, 4) (times a factor in [1, 1.1], plus 0.01: strictly positive, what the
I-divergence's updates need), the initial factors are rand(): with the reference's update rules in NumPy alone, every model of
SHAPES2 / SHAPES3 below has finite, strictly positive predictions on all of R after one iteration (checked on the host before the
seeds were fixed; the multiplicative updates keep positive factors positive)."""
import ctypes as C

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import NMF, NMTF, _lib
from bnmtf_amd._base import metrics_from_sums

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRICS = ('MSE', 'R^2', 'Rp')


def np_data(I, J, K, L=0, frac_missing=0.2, seed=3):
    rs = np.random.RandomState(seed)
    k, l = min(K, 4), min(L, 4)
    if L:
        R = rs.exponential(1.0, (I, k)) @ rs.exponential(1.0, (k, l)) @ rs.exponential(1.0, (J, l)).T
    else:
        R = rs.exponential(1.0, (I, k)) @ rs.exponential(1.0, (J, k)).T
    R = R * (1.0 + 0.1 * rs.rand(I, J)) + 0.01
    M = (rs.rand(I, J) >= frac_missing).astype(float)
    M[rs.randint(I, size=J), np.arange(J)] = 1; M[np.arange(I), rs.randint(J, size=I)] = 1      # no empty row / column
    return R, M


def shape_data(shape):
    """The data of a launch-shape case (a matrix with a single row or column is fully observed)."""
    I, J, K = shape[:3]; L = shape[3] if len(shape) == 4 else 0
    return np_data(I, J, K, L, frac_missing=0.2 if min(I, J) > 1 else 0.0, seed=I + J)


def initial_factors(shape, seed=17):
    """rand() factors in the order NMF.initialise('random') / NMTF.initialise('random', 'random') draw them."""
    I, J, K = shape[:3]
    rs = np.random.RandomState(seed)
    if len(shape) == 4:
        L = shape[3]
        S = rs.rand(K, L); F = rs.rand(I, K); G = rs.rand(J, L)
        return F, S, G
    U = rs.rand(I, K); V = rs.rand(J, K)
    return U, V


def _model(R, M, K, L=0, seed=17):
    np.random.seed(seed)
    if L:
        m = NMTF(R, M, K, L, verbose=False); m.initialise('random', 'random')
    else:
        m = NMF(R, M, K, verbose=False); m.initialise('random')
    return m


def _test_mask(M, frac, seed):
    """A held-out mask inside the complement of M (seed stated by the caller)."""
    rs = np.random.RandomState(seed)
    Mt = ((rs.rand(*M.shape) < frac) & (M == 0)).astype(float)
    assert Mt.sum() >= 20
    return Mt


def _numpy_sums(R, Mt, m):
    """The six sums in fp64 from the model's factors (fp32 values) and the fp32 R the device holds."""
    i, j = np.nonzero(np.asarray(Mt))
    r = np.asarray(R, dtype=np.float32)[i, j].astype(np.float64)
    if hasattr(m, "L"):
        A = np.asarray(m.F, dtype=np.float64) @ np.asarray(m.S, dtype=np.float64); B = np.asarray(m.G, dtype=np.float64)
    else:
        A = np.asarray(m.U, dtype=np.float64); B = np.asarray(m.V, dtype=np.float64)
    for f in _factors(m):
        assert np.array_equal(getattr(m, f), np.asarray(getattr(m, f), dtype=np.float32)), f      # (the device's fp32 values)
    p = np.einsum('ek,ek->e', A[i], B[j])
    return np.array([float(len(r)), r.sum(), (r * r).sum(), p.sum(), (p * p).sum(), (r * p).sum()])


def _device_sums(model, n_iter):
    """bnmtf_get_heldout through ctypes: [n_iter][6]."""
    out = np.zeros((n_iter, 6))
    _lib.check(_lib.lib().bnmtf_get_heldout(model._handle(), C.c_int(n_iter), out.ctypes.data_as(C.c_void_p)))
    return out


def _factors(m):
    return ("F", "S", "G") if hasattr(m, "L") else ("U", "V")


# ---- 1: the entry point of the feature

@pytest.mark.parametrize("tri", [False, True], ids=["nmf", "nmtf"])
def test_run_with_M_test_returns_one_entry_per_iteration_and_metric(tri):
    R, M = np_data(120, 90, 4, 3 if tri else 0)
    Mt = _test_mask(M, 0.5, seed=1)
    m = _model(R, M, 4, 3 if tri else 0)
    m.run(3, M_test=Mt)
    assert sorted(m.all_performances_test) == sorted(METRICS)
    for name in METRICS:
        assert len(m.all_performances_test[name]) == 3 and np.isfinite(m.all_performances_test[name]).all()
    assert len(m.all_performances['MSE']) == 3


# ---- 2: entry t - 1 is the state a run of t iterations ends with

@pytest.mark.parametrize("tri", [False, True], ids=["nmf", "nmtf"])
def test_entry_t_equals_numpy_on_the_factors_after_t_iterations(tri):
    I, J, K, L = 140, 100, 5, (3 if tri else 0)
    R, M = np_data(I, J, K, L, seed=6)
    Mt = _test_mask(M, 0.7, seed=8)                     # mask seed 8
    n = 4
    a = _model(R, M, K, L)
    a.run(n, M_test=Mt)
    dev = _device_sums(a, n)
    for t in range(1, n + 1):
        b = _model(R, M, K, L)
        b.run(t)
        assert not hasattr(b, "all_performances_test")
        ref = _numpy_sums(R, Mt, b)
        print("tri" if tri else "bi", t, dev[t - 1], ref)
        assert ref[3] > 0 and ref[4] > 0, "the predictions are all zero: nothing is compared"
        np.testing.assert_allclose(dev[t - 1], ref, rtol=RTOL, atol=0, err_msg="iteration %d" % t)
        got = metrics_from_sums(dev[t - 1]); want = metrics_from_sums(ref)
        for name in METRICS:
            assert a.all_performances_test[name][t - 1] == got[name], (name, t)            # finished from the record, with metrics_from_sums
            np.testing.assert_allclose(a.all_performances_test[name][t - 1], want[name], rtol=RTOL, err_msg="%s after %d iterations" % (name, t))
    for f in _factors(a):                               # (and the run with the mask ended where the run of n iterations without it did)
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert len(set(a.all_performances_test['MSE'])) == n          # (a trajectory that moves)
    with pytest.raises(bnmtf_amd.BnmtfError):           # more iterations than the last run call recorded
        _device_sums(a, n + 1)


# ---- 3: launch shapes.  A wave owns a row and takes 64 of its entries per step (a lane per entry), a block four rows; no grid
# stride.  The factor row is staged over the lanes in strides of 64 columns (ranks 1, 63, 64, 65, 128, 129, 256); NMTF forms it
# with K multiply-adds per column.

def shape_masks(I, J, M):
    rs = np.random.RandomState(21)                      # mask seed 21
    masks = {}
    one = np.zeros((I, J)); one[I - 1, J - 1] = 1
    masks["one entry"] = one
    masks["full"] = np.ones((I, J))
    masks["overlapping the training mask"] = np.maximum((rs.rand(I, J) < 0.5) * M, one)
    if I >= 8:
        gaps = (rs.rand(I, J) < 0.4).astype(float)
        gaps[2, 0] = 1
        gaps[0, :] = 0; gaps[1, :] = 0; gaps[I // 2, :] = 0; gaps[I - 1, :] = 0
        masks["empty rows at the start, in the middle, at the end"] = gaps
    # entry counts around the wave step and its multiples, one count per row (rows beyond the list stay empty)
    counts = [c for c in (1, 63, 64, 65, 127, 128, 129, J - 1, J) if 1 <= c <= J]
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


SHAPES2 = [(1, 130, 1), (130, 1, 63), (63, 64, 64), (64, 65, 65), (65, 129, 256), (130, 130, 128)]
SHAPES3 = [(1, 65, 1, 63), (63, 130, 64, 65), (64, 1, 65, 1), (65, 64, 256, 64), (130, 63, 2, 256), (64, 129, 129, 129)]


@pytest.mark.parametrize("shape", SHAPES2 + SHAPES3, ids=lambda s: "x".join(str(v) for v in s))
def test_launch_shapes_match_numpy(shape):
    tri = len(shape) == 4
    I, J, K = shape[:3]; L = shape[3] if tri else 0
    R, M = shape_data(shape)
    m = _model(R, M, K, L, seed=17)
    for f, x in zip(_factors(m), initial_factors(shape, 17)):
        assert np.array_equal(getattr(m, f), x), f          # (the factors whose first iteration was checked on the host)
    for name, Mt in shape_masks(I, J, M).items():
        m.run(1, M_test=Mt)
        dev = _device_sums(m, 1)
        ref = _numpy_sums(R, Mt, m)
        assert dev[0][0] == Mt.sum(), name
        assert ref[3] > 0 and ref[4] > 0 and np.isfinite(ref).all(), (shape, name)
        np.testing.assert_allclose(dev[0], ref, rtol=RTOL, atol=0, err_msg="%s: %s" % (shape, name))


# ---- 4: no effect when unused, none on the trajectory when used

@pytest.mark.parametrize("tri", [False, True], ids=["nmf", "nmtf"])
def test_trajectory_is_bit_identical_with_and_without_a_mask(tri):
    K, L = 7, (5 if tri else 0)
    R, M = np_data(200, 170, K, L, seed=9)
    Mt = _test_mask(M, 0.5, seed=5)
    runs, idivs = [], []
    for use in (False, True, True):
        m = _model(R, M, K, L, seed=23)
        fn = _lib.lib().bnmtf_np_run if tri else _lib.lib().bnmf_np_run
        idivs.append(m._run_device(fn, 5, Mt if use else None))         # (run()'s body: it returns the I-divergences run() prints)
        runs.append(m)
    plain, held, held2 = runs
    assert not hasattr(plain, "all_performances_test")
    for f in _factors(plain):
        assert np.array_equal(getattr(plain, f), getattr(held, f)), f
    assert plain.all_performances == held.all_performances
    assert np.array_equal(idivs[0], idivs[1]) and np.isfinite(idivs[0]).all()
    assert held.all_performances_test == held2.all_performances_test            # two runs with the mask: the same bits
    assert np.array_equal(_device_sums(held, 5), _device_sums(held2, 5))
    # then again without: no attribute, no record, and the trajectory goes on as that of a model that never had a mask
    held.run(4); plain.run(4)
    assert not hasattr(held, "all_performances_test")
    for f in _factors(plain):
        assert np.array_equal(getattr(plain, f), getattr(held, f)), f
    assert plain.all_performances == held.all_performances
    with pytest.raises(bnmtf_amd.BnmtfError):                                   # (no mask on the handle: no record)
        _device_sums(held, 1)


def test_the_mask_is_validated_before_any_device_call():
    R, M = np_data(40, 30, 3)
    m = _model(R, M, 3)
    U0 = m.U.copy()
    with pytest.raises(AssertionError):
        m.run(2, M_test=np.ones((30, 40)))
    with pytest.raises(AssertionError):
        m.run(2, M_test=np.zeros((40, 30)))
    with pytest.raises(AssertionError):
        m.run(2, M_test=np.full((40, 30), 0.5))
    assert np.array_equal(m.U, U0) and m._h is None     # (no handle was created: nothing reached the device)
