"""Pins of the exact K-means cases (tests/_kmeans_cases.py), no GPU: the cases are exact, each named situation really occurs
in its case, the models of the two launches equal the reference, and each single fault in them changes a checked output.
The GPU side is test_kmeans_kernels_gpu.py."""
import numpy as np
import pytest

from _kmeans_cases import (ASSIGN_FAULTS, CASES, INF, LANES, PASS, SHAPES, SUMS_FAULTS, assign_model, assign_reference, by_name,
                           distances, sums_model, sums_reference)

IDS = [c.id for c in CASES]


def _one(name):
    (c,) = by_name(name)
    return c


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_exact(case):
    """integers in range, 0/1 masks; num, overlap and the totals are integers far below 2^53 in any order, so mse is one
    correctly rounded division of two exact doubles and cnt / tot are exact"""
    for X in (case.X, case.X_after()):
        assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 6
    assert np.array_equal(case.C, np.round(case.C))
    assert set(np.unique(case.M)) <= {0, 1} and set(np.unique(case.Mc)) <= {0, 1}
    assert case.M.sum(axis=1).min() > 0                     # (what KMeans accepts: no fully unobserved point)
    num, ov = distances(case.X_after(), case.M, case.C, case.Mc)
    assert num.max() < 2 ** 53 and ov.max() <= case.d
    assert case.n * 6 < 2 ** 53
    for a in case.sums:
        assert a.min() >= 0 and a.max() < case.K and a.shape == (case.n,)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_models_of_the_launches_equal_the_reference(case):
    X = case.X_after()
    a, dist = assign_model(X, case.M, case.C, case.Mc)
    ra, rdist = assign_reference(X, case.M, case.C, case.Mc)
    assert np.array_equal(a, ra) and np.array_equal(dist, rdist)
    for s in case.sums:
        cnt, tot = sums_model(X, case.M, s, case.K)
        rcnt, rtot = sums_reference(X, case.M, s, case.K)
        assert np.array_equal(cnt, rcnt) and np.array_equal(tot, rtot)
    for p, (c, dv) in case.expect.items():
        assert ra[p] == c and (dv is None or rdist[p] == dv), (p, ra[p], rdist[p])


def test_the_shapes_reach_every_edge():
    assert {s[0] for s in SHAPES} == {1, 3, 4, 5, 255, 256, 257}
    assert {s[1] for s in SHAPES} == {1, 63, 64, 65, 128, 129}
    assert {s[2] for s in SHAPES} == {1, 2, 39, 40, 41, 80, 81}
    assert [(c.n, c.d, c.K) for c in by_name("shape")] == SHAPES
    assert max(c.n * c.d for c in CASES) == 257 * 129
    names = {c.name for c in CASES}
    assert names == {"shape", "tie2", "tie3", "tie_after_undefined", "no_overlap", "single_overlap", "zero_mask_centroid",
                     "sums_one_cluster", "sums_straddle_passes", "sums_unobserved_coordinate", "sums_twice", "set_row"}


@pytest.mark.parametrize("ties", (2, 3))
def test_the_tie_is_exact_and_nearest(ties):
    c = _one("tie%d" % ties)
    num, ov = distances(c.X, c.M, c.C, c.Mc)
    mse = num / ov
    for t in range(1, ties):
        assert np.array_equal(num[:, t], num[:, 0]) and np.array_equal(ov[:, t], ov[:, 0])
    assert (mse[:, :ties].max(axis=1) < mse[:, ties:].min(axis=1)).all()
    assert (assign_reference(c.X, c.M, c.C, c.Mc)[0] == 0).all()


def test_the_tie_behind_an_undefined_first_centroid():
    c = _one("tie_after_undefined")
    num, ov = distances(c.X, c.M, c.C, c.Mc)
    assert (ov[:, 0] == 0).all() and c.Mc[0].any()
    assert np.array_equal(num[:, 1], num[:, 2]) and np.array_equal(ov[:, 1], ov[:, 2]) and (ov[:, 1] > 0).all()
    assert (num[:, 1] * ov[:, 3] < num[:, 3] * ov[:, 1]).all()            # strictly nearer than centroid 3
    assert (assign_reference(c.X, c.M, c.C, c.Mc)[0] == 1).all()


def test_the_point_without_overlap():
    c = _one("no_overlap")
    num, ov = distances(c.X, c.M, c.C, c.Mc)
    assert (ov[2] == 0).all() and c.M[2].sum() == 2 and c.M[2, 64]
    assert (ov[[0, 1, 3, 4, 5]].max(axis=1) > 0).all()
    a, dist = assign_reference(c.X, c.M, c.C, c.Mc)
    assert a[2] == c.K - 1 and dist[2] == INF and np.isfinite(np.delete(dist, 2)).all()


def test_the_single_overlaps_sit_on_the_stride_edges():
    c = _one("single_overlap")
    assert c.d - 1 == 99 and c.d % LANES != 0
    for p, j in enumerate((99, 64, 63)):
        assert np.flatnonzero(c.M[p]).tolist() == [j]
        _, ov = distances(c.X, c.M, c.C, c.Mc)
        assert (ov[p] == 1).all()
        assert len(set(c.C[:, j])) == c.K
    a, dist = assign_reference(c.X, c.M, c.C, c.Mc)
    assert a[:3].tolist() == [3, 2, 4] and dist[:3].tolist() == [0.0, 0.0, 0.0]


def test_the_centroid_that_knows_no_coordinate():
    c = _one("zero_mask_centroid")
    assert not c.Mc[2].any() and np.array_equal(c.C[2], c.X[0])
    a, _ = assign_reference(c.X, c.M, c.C, c.Mc)
    assert (a != 2).all()
    seen = c.Mc.copy(); seen[2] = 1
    assert assign_reference(c.X, c.M, c.C, seen)[0][0] == 2              # (with a mask it would take point 0)


def test_the_sums_situations():
    c = _one("sums_one_cluster")
    assert (c.sums[0] == 1).all()
    cnt, tot = sums_reference(c.X, c.M, c.sums[0], c.K)
    assert not cnt[[0, 2]].any() and not tot[[0, 2]].any() and np.array_equal(cnt[1], c.M.sum(axis=0))

    c = _one("sums_straddle_passes")
    assert set(c.sums[0]) == {PASS - 1, PASS, 2 * PASS - 1, 2 * PASS} and c.K == 2 * PASS + 1
    cnt, _ = sums_reference(c.X, c.M, c.sums[0], c.K)
    assert np.flatnonzero(cnt.sum(axis=1)).tolist() == [39, 40, 79, 80]   # 38, 41, 78 and the rest empty

    c = _one("sums_unobserved_coordinate")
    cnt, tot = sums_reference(c.X, c.M, c.sums[0], c.K)
    for j in (64, 69):
        assert cnt[0, j] == 0 and tot[0, j] == 0 and cnt[1, j] == 4
    assert cnt[0].max() > 0

    c = _one("sums_twice")
    first, second = (sums_reference(c.X, c.M, a, c.K) for a in c.sums)
    assert (first[0].sum(axis=1) > 0).all() and c.K > PASS
    assert np.flatnonzero(second[0].sum(axis=1)).tolist() == [0, 41]
    assert not np.array_equal(first[0][[0, 41]], second[0][[0, 41]])


def test_set_row_moves_the_last_point():
    c = _one("set_row")
    before, _ = assign_reference(c.X, c.M, c.C, c.Mc)
    after, dist = assign_reference(c.X_after(), c.M, c.C, c.Mc)
    assert before[c.n - 1] == 0 and after[c.n - 1] == 2 and dist[c.n - 1] == 0.0
    assert np.array_equal(c.X_after()[:-1], c.X[:-1]) and not np.array_equal(c.X_after()[-1], c.X[-1])
    s = c.sums[0]
    assert not np.array_equal(sums_reference(c.X, c.M, s, c.K)[1], sums_reference(c.X_after(), c.M, s, c.K)[1])


def _assign_differs(c, fault):
    X = c.X_after()
    a, dist = assign_model(X, c.M, c.C, c.Mc, fault)
    ra, rdist = assign_reference(X, c.M, c.C, c.Mc)
    return not (np.array_equal(a, ra) and np.array_equal(dist, rdist))


def _sums_differ(c, fault):
    X = c.X_after()
    return any(not all(np.array_equal(g, w) for g, w in zip(sums_model(X, c.M, s, c.K, fault), sums_reference(X, c.M, s, c.K))) for s in c.sums)


@pytest.mark.parametrize("fault", ASSIGN_FAULTS + SUMS_FAULTS)
def test_a_single_fault_changes_a_checked_output(fault):
    differs = _assign_differs if fault in ASSIGN_FAULTS else _sums_differ
    seen = [c.id for c in CASES if differs(c, fault)]
    print("%s: seen by %s" % (fault, seen))
    assert seen, fault
    # and by the case that is there for it
    want = {"lanes_stop_at_full_strides": "single_overlap", "le_compare": "tie2", "undefined_first_keeps": "no_overlap",
            "tail_points_skipped": "shape", "pass_writes_at_c": "sums_straddle_passes", "fourth_group_dropped": "sums_one_cluster"}[fault]
    assert any(differs(c, fault) for c in by_name(want))
