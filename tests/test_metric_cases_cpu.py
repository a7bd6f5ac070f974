"""Pins of the exact metric-sum cases (tests/_metric_cases.py), no GPU: every case is exact in fp64 in any summation order,
every family has a sum no fp32 accumulator holds, a NumPy model of metric_kernel's tiling equals the reference and each single
fault in it moves a checked sum of some case, and the shapes reach every launch edge.  The GPU side is
test_metric_sums_gpu.py."""
import numpy as np
import pytest

from _metric_cases import (CASES, FAMILIES, FAULTS, FOLD, TILE, TWO24, TWO53, as_doubles, by_family, kernel_model, model_outputs,
                           problem, real_case, reference, tiles)

IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_exact_in_any_order(case):
    """(a) the sum of the |terms| of each of the seven sums, and every single contraction, stays below 2^53; the inputs are
    integers in their ranges, R exact in fp32, the VB second moment exact in the fp32 the device forms it in"""
    p = problem(case)
    assert np.array_equal(p.R, np.round(p.R)) and np.abs(p.R).max() <= 8 and p.R.dtype == np.float32
    hi = 5 if case.family == "vb" else 7
    for X in (p.A, p.B):
        assert np.array_equal(X, np.round(X)) and X.min() >= 0 and X.max() <= hi
    if p.S is not None:
        assert np.array_equal(p.S, np.round(p.S)) and p.S.min() >= 0 and p.S.max() <= 3
    if case.family == "vb":
        # S2 = var + exp * exp in fp32 (vb_upload_dir); fused or not, it is the integer var + exp^2, far below 2^24
        for e, v, s2 in ((p.A, p.varA, p.second_moments()[0]), (p.B, p.varB, p.second_moments()[1])):
            assert v.min() >= 0 and v.max() <= 3 and np.array_equal(v, np.round(v))
            assert np.array_equal(s2, v + e * e) and s2.max() < TWO24
            assert np.array_equal((e * e).astype(np.float32), e * e)
    assert p.M.sum(axis=0).min() > 0 and p.M.sum(axis=1).min() > 0           # (what the model classes accept)
    for name in case.masks:
        mags = reference(p, name, magnitudes=True)
        assert max(mags) < TWO53, (name, mags)
        as_doubles(reference(p, name))                                       # every checked value is a double


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_has_a_sum_beyond_fp32(family):
    """(b) at least one checked sum above 2^24: an fp32 accumulator anywhere fails the comparison"""
    top = max(max(abs(v) for v in reference(problem(c), name)) for c in by_family(*FAMILIES[family]) for name in c.masks)
    assert top > TWO24, top


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_of_the_tiling_equals_the_reference(case):
    """(c), first half: the model without a fault is the reference -- on every mask"""
    p = problem(case)
    for name in case.masks:
        assert model_outputs(p, name) == reference(p, name), name


def test_stride_64_on_both_sides_is_no_fault():
    """a chunk is at most 64 columns wide, so index r * 64 + k never reaches row r + 1: a tile stride of 64 used by the load
    AND the product changes no value (65 is there for the LDS banks).  The fault that aliases rows is the two disagreeing."""
    for c in by_family("plain", "wide", "vb")[::4]:
        p = problem(c)
        assert model_outputs(p, "train", "stride64_both") == reference(p, "train")


def _sees(fault):
    """cases (and masks) on which the fault changes a checked sum; smallest shapes first, the first find is enough"""
    for c in sorted(CASES, key=lambda c: c.I * c.J * c.width):
        if fault == "fold_stops_at_256" and tiles(c.I, c.J) <= FOLD:
            continue
        if fault == "second_moment_ignores_mask" and c.family != "vb":
            continue
        p = problem(c)
        for name in c.masks:
            if model_outputs(p, name, fault) != reference(p, name):
                return c.id, name
    return None


@pytest.mark.parametrize("fault", FAULTS)
def test_a_single_fault_moves_a_checked_sum(fault):
    """(c), second half"""
    seen = _sees(fault)
    assert seen is not None, fault
    print("%s: seen by %s on mask %s" % ((fault,) + seen))


def test_the_fold_faults_are_seen_at_every_tile_count_above_256():
    for c in CASES:
        if tiles(c.I, c.J) > FOLD:
            p = problem(c)
            assert model_outputs(p, "corner", "fold_stops_at_256") != reference(p, "corner"), c.id


def test_the_shapes_reach_every_edge():
    """(d)"""
    met = by_family("plain", "wide", "tri", "state", "state_tri")
    assert {256, 272, 257} <= {tiles(c.I, c.J) for c in met}
    sizes = {1, 31, 32, 33, 63, 64, 65, 130}
    assert sizes <= {c.I for c in met} and sizes <= {c.J for c in met}
    assert {c.I % TILE for c in met} >= {0, 1, 2, 31} and {c.J % TILE for c in met} >= {0, 1, 2, 31}
    assert {c.K for c in by_family("plain")} == {1, 31, 63, 64}
    wide = {c.K for c in by_family("wide")}
    assert wide == {65, 127, 128, 129, 256} and {w % 64 for w in wide} == {0, 1, 63}
    assert {w % 64 for w in {c.K for c in by_family("plain")}} == {0, 1, 31, 63}
    assert {(c.K, c.L) for c in by_family("tri")} == {(1, 64), (64, 1), (33, 31)}
    vb = by_family("vb")
    assert {c.K for c in vb} == {1, 33, 63, 64} and {c.I for c in vb} == {33, 65} == {c.J for c in vb}
    assert {c.family for c in CASES} == {"plain", "wide", "tri", "state", "state_tri", "vb"}
    # a row group past the edge (I mod 32 <= 24) and one cut by it; every mask of the issue on every non-VB case
    assert any(0 < c.I % TILE <= 24 for c in met) and any(c.I % TILE > 24 for c in met)
    assert all(len(c.masks) == 8 for c in met)


def test_each_mask_is_what_its_name_says():
    for c in CASES[:11]:
        p, I, J = problem(c), c.I, c.J
        assert p.argument("train") is None and np.array_equal(p.mask("train"), p.M)
        assert p.mask("full").all() and not p.mask("empty").any()
        m = p.mask("corner"); assert m.sum() == 1 and m[I - 1, J - 1]
        m = p.mask("last_row"); assert m.sum() == J and m[I - 1].all()
        m = p.mask("last_col"); assert m.sum() == I and m[:, J - 1].all()
        m = p.mask("tile_out")
        zi, zj = np.nonzero(m == 0)
        assert len(zi) and zi.min() % TILE == 0 and zj.min() % TILE == 0 and zi.max() - zi.min() < TILE and zj.max() - zj.min() < TILE
        assert len(zi) == min(TILE, I - zi.min()) * min(TILE, J - zj.min())
        assert reference(p, "empty") == [0] * 6
        if I * J >= 64:
            assert 0.3 < p.mask("half").mean() < 0.7


def test_the_real_valued_case_leaves_room_for_its_bound():
    """the derived bound of the cancelling SSE is below 1e-3 of the reference SSE (so the test still resolves the SSE), and the
    data are what the issue asks for: about 1e4 entries, values near 100, residuals near 1e-2"""
    rc = real_case()
    print("N = %d, reference SSE = %.6e, bound = %.6e, bound / SSE = %.3e" % (rc.N, rc.sse, rc.bound, rc.bound / rc.sse))
    assert 8000 < rc.N < 12000 and 70 < rc.R.mean() < 130
    rms = (rc.sse / rc.N) ** 0.5
    assert 0.5e-2 < rms < 2e-2
    assert rc.bound < 1e-3 * rc.sse
    assert rc.R.dtype == np.float32 and not np.array_equal(rc.R, np.round(rc.R))
