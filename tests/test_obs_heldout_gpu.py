"""run(..., M_test=Entries) on the observed-entry layout: the held-out sums of every iteration, computed on
the device by csrc/kernel_obs_heldout.hip from the handle's own fp32 factors, against NumPy fp64 on the model's samples (Gibbs) or
its pulled factors (ICM, VB), at every launch shape of the kernel, twice for equal bits, and that nothing else moves when a list
is set -- or not set.

Tolerance: RTOL = 1e-9, the project's own for fp64 device sums (tests/test_heldout_gpu.py): device and NumPy both sum fp64 products
of the same fp32 values and differ in summation order only; the data and the factors are non-negative, so nothing cancels inside
a dot product or a sum.

The kernel's constants: W = 64 entries of a row per wave step (a lane each), B = 4 rows per block; the fold takes 256 blocks per
trip."""
import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import Entries, bnmf_gibbs_optimised, bnmf_vb_observed, nmf_icm
from bnmtf_amd._base import metrics_from_sums

pytestmark = pytest.mark.gpu

RTOL = 1e-9
W, B = 64, 4
PRI = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)      # (rates of 1: factors on the data's scale, tests/test_heldout_gpu.py)
METRICS = ('MSE', 'R^2', 'Rp')


def _data(I, J, K, seed=3, share=0.3):
    """Non-negative R of rank min(K, 8) and a training mask without an empty row or column."""
    rs = np.random.RandomState(seed)
    k = min(K, 8)
    R = rs.exponential(1.0, (I, k)) @ rs.exponential(1.0, (J, k)).T
    M = (rs.rand(I, J) < share).astype(float)
    M[np.arange(I), np.arange(I) % J] = 1; M[np.arange(J) % I, np.arange(J)] = 1
    return R, M


def _held(R, M, counts, seed=9):
    """A held-out list built by hand: row i gets counts[i] entries (its first columns from a seeded permutation), then the entry
    (I - 1, J - 1) and ten training entries of other rows than those and EMPTY, none twice; in a seeded shuffled order."""
    I, J = R.shape
    rs = np.random.RandomState(seed)
    at = set()
    for i, c in counts.items():
        at.update((i, int(j)) for j in rs.permutation(J)[:c])
    at.add((I - 1, J - 1))
    ti, tj = np.nonzero(M)
    for q in rs.choice(np.flatnonzero(~np.isin(ti, list(counts) + [EMPTY])), 10, replace=False):
        at.add((int(ti[q]), int(tj[q])))
    at = sorted(at)
    order = rs.permutation(len(at))
    rows = np.array([at[q][0] for q in order]); cols = np.array([at[q][1] for q in order])
    return Entries((I, J), rows, cols, R[rows, cols])


def _numpy_sums(E, A, Bf):
    """The six sums in fp64 from fp32 factors and the fp32 values the device is handed."""
    r = E.values32().astype(np.float64)
    p = np.einsum('ek,ek->e', np.asarray(A, dtype=np.float64)[E.rows], np.asarray(Bf, dtype=np.float64)[E.cols])
    return np.array([float(len(r)), r.sum(), (r * r).sum(), p.sum(), (p * p).sum(), (r * p).sum()])


def _gibbs(R, M, K, n, E=None, seed=123):
    np.random.seed(5)
    m = bnmf_gibbs_optimised(R, M, K, PRI, seed=seed, verbose=False, layout='observed')
    m.initialise('random')
    m.run(n, M_test=E)
    return m


def _check_gibbs(m, E, n):
    sums = m._heldout_sums(n)
    assert (sums[:, 0] == len(E)).all()
    for t in range(n):
        ref = _numpy_sums(E, m.all_U[t], m.all_V[t])
        print("iteration %d: largest relative difference %.3g" % (t, np.max(np.abs(sums[t] - ref) / np.abs(ref))))
        np.testing.assert_allclose(sums[t], ref, rtol=RTOL, atol=0, err_msg="iteration %d" % t)
        assert ref[3] > 0 and ref[4] > 0, "the predictions are all zero: nothing is compared"
        want = metrics_from_sums(sums[t])
        for name in METRICS:
            assert m.all_performances_test[name][t] == want[name] or (np.isnan(want[name]) and np.isnan(m.all_performances_test[name][t]))
    assert all(len(m.all_performances_test[name]) == n for name in METRICS)
    return sums


# ---------------------------------------------------------------- every launch shape
# rows without an entry, with 1, W - 1, W, W + 1 entries; I = 97 leaves the last block of B rows partial
EMPTY = 1
COUNTS_97 = {0: 1, 2: W - 1, 3: W, 4: W + 1, 50: 7, 95: 3}
SHAPES = [(97, 83, K, COUNTS_97) for K in (1, 5, 32, 64, 65, 256)]
SHAPES.append((9, 200, 5, {0: 2 * W + 1, 3: 200, 5: 1}))             # the lane loop's third trip
SHAPES.append((1100, 7, 3, {i: 1 + i % 7 for i in range(0, 1100, 3)}))   # 275 blocks: the fold's strided loop


@pytest.mark.parametrize("I, J, K, counts", SHAPES, ids=["%dx%d-k%d" % s[:3] for s in SHAPES])
def test_gibbs_sums_match_numpy_at_every_launch_shape_and_twice_give_the_same_bits(I, J, K, counts):
    R, M = _data(I, J, K)
    E = _held(R, M, counts)
    per_row = E.counts()[1]
    assert per_row[EMPTY] == 0 and all(per_row[i] == c for i, c in counts.items()) and (I - 1, J - 1) in set(zip(E.rows.tolist(), E.cols.tolist()))
    assert M[E.rows, E.cols].sum() >= 10                   # (overlaps the training entries)
    n = 3
    a = _gibbs(R, M, K, n, E)
    sums = _check_gibbs(a, E, n)
    b = _gibbs(R, M, K, n, E)
    assert b._heldout_sums(n).tobytes() == sums.tobytes()
    a.close(); b.close()


# ---------------------------------------------------------------- ICM and VB: no per-iteration state
def _icm(R, M, K):
    np.random.seed(5)
    m = nmf_icm(R, M, K, PRI, verbose=False, layout='observed')
    m.initialise('random')
    return m, ("U", "V")


def _vb(R, M, K):
    np.random.seed(5)
    m = bnmf_vb_observed(R, M, K, PRI, verbose=False)
    m.initialise('random')
    return m, ("expU", "expV")


@pytest.mark.parametrize("make", [_icm, _vb], ids=["icm", "vb"])
def test_icm_and_vb_records_match_numpy_one_iteration_per_call_and_equal_the_single_runs(make):
    R, M = _data(97, 83, 5)
    E = _held(R, M, COUNTS_97)
    n = 4
    m, names = make(R, M, 5)
    recs, curve = [], {name: [] for name in METRICS}
    for t in range(n):
        m.run(1, M_test=E)
        s = m._heldout_sums(1)[0]
        ref = _numpy_sums(E, getattr(m, names[0]), getattr(m, names[1]))
        np.testing.assert_allclose(s, ref, rtol=RTOL, atol=0, err_msg="iteration %d" % t)
        assert s[0] == len(E) and ref[3] > 0
        recs.append(s)
        for name in METRICS:
            curve[name].append(m.all_performances_test[name][0])
    one, _ = make(R, M, 5)
    one.run(n, M_test=E)
    assert one._heldout_sums(n).tobytes() == np.array(recs).tobytes()           # run(a); run(b) is run(a + b) on this layout
    assert all(np.array_equal(one.all_performances_test[name], curve[name]) for name in METRICS)
    # the curve's last element is predict(E) on the final state (fp64 copies of the same fp32 factors)
    got = one.predict(E)
    for name in METRICS:
        np.testing.assert_allclose(one.all_performances_test[name][-1], got[name], rtol=RTOL)
    m.close(); one.close()


# ---------------------------------------------------------------- nothing else moves
def test_a_run_with_a_list_is_the_run_without_it_and_the_attribute_goes_with_the_list():
    R, M = _data(97, 83, 5)
    E = _held(R, M, COUNTS_97)
    n = 4
    a, b = _gibbs(R, M, 5, n, E), _gibbs(R, M, 5, n)
    assert hasattr(a, "all_performances_test") and not hasattr(b, "all_performances_test")
    for name in ("all_U", "all_V", "U", "V", "all_tau"):
        assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), name
    assert a.tau == b.tau and all(np.array_equal(a.all_performances[k], b.all_performances[k]) for k in METRICS)
    # the last element of the curve is predict(E) of the last sample
    got = a.predict(E, n - 1, 1)
    for name in METRICS:
        np.testing.assert_allclose(a.all_performances_test[name][-1], got[name], rtol=RTOL)
    # a list in another order: the same bits
    order = np.random.RandomState(2).permutation(len(E))[::-1]
    c = _gibbs(R, M, 5, n, Entries(E.shape, E.rows[order], E.cols[order], E.values[order]))
    assert c._heldout_sums(n).tobytes() == a._heldout_sums(n).tobytes()
    # replacing the list between calls gives the new list's curve
    E2 = _held(R, M, {7: 5, 8: W + 3}, seed=4)
    a.run(2, M_test=E2)
    sums = _check_gibbs(a, E2, 2)
    assert len(a.all_performances_test['MSE']) == 2 and sums[0, 0] == len(E2) != len(E)
    # a call without M_test: the attribute is gone and the handle holds no list
    a.run(2)
    assert not hasattr(a, "all_performances_test")
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        a._heldout_sums(1)
    assert "no held-out mask set" in str(e.value)
    for m in (a, b, c):
        m.close()
