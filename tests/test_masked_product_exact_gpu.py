"""The variational sweep's masked product (csrc/kernel_maskgemm.hip: integer accumulation on the int8 matrix cores, one fp32
combine per slab) held to its bits at every launch shape, and the column maxima that fix its fixed-point grid.

  * test_the_masked_product_returns_the_models_bits: per case of tests/_masked_product_cases.py (its docstring: the families, the
    masks, the model; test_masked_product_cases_cpu.py: what the cases cover and which defects they would see) the hook
    bnmf_vb_masked_sums for both directions and both value families against the expected fp32 bits -- family X: the exact fp64
    product itself, family G: the slab-aware NumPy model.  No tolerance, no element left out.  The restated launch geometry is
    compared with what the handle reports (describe(): rows[...], cols[...], masked_product[...]) first.
  * the posted maxima: on the on-chip path run() takes the column maxima of [S2 | E^2] from the relayout (post_kernel<true> ->
    mpart -> gram_reduce_kernel's maxima block -> PostArgs::umax), not from vb_colmax_kernel; the hook bnmf_vb_column_maxima
    reads both.  A maximum that is too large only coarsens the grid -- inside every tolerance of the trajectory tests.

The statement of the product's ACCURACY against fp64 stays where it was: test_bnmf_vb_gpu.py's bound-based test."""
import re

import numpy as np
import pytest

import _masked_product_cases as C
from bnmtf_amd import _lib, bnmf_vb_optimised

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)


def _reported(desc):
    """{direction: (n, n_pad, inner_pad, msplit, mipw)} of a handle's description"""
    out = {}
    mp = re.search(r"masked_product\[row_units=(\d+)/(\d+) col_units=(\d+)/(\d+)\]$", desc)
    assert mp, desc
    for d, (a, b) in zip(C.DIRS, ((1, 2), (3, 4))):
        m = re.search(r"%s\[n=(\d+) n_pad=(\d+) split=\d+ ipw=\d+ inner_pad=(\d+) " % d, desc)
        assert m, desc
        out[d] = tuple(int(t) for t in m.groups()) + (int(mp.group(a)), int(mp.group(b)))
    return out


def _model(case):
    rs = np.random.RandomState(case.seed + 1)
    M = C.mask(case)
    b = bnmf_vb_optimised(rs.rand(case.I, case.J), M, case.K, PRI, verbose=False)
    b.initialise('exp')
    return b, M


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_the_masked_product_returns_the_models_bits(case):
    b, M = _model(case)
    rep = _reported(b.describe())
    for d in C.DIRS:
        g = case.geometry(d)
        assert rep[d] == (case.shape(d)[0], g["n_pad"], g["inner_pad"], g["msplit"], g["mipw"]), (d, rep[d], g)
        assert (g["msplit"], g["mipw"] // 32) == case.expect[d]
    failures = []
    for fam in C.FAMILIES:
        mom = C.moments(case, fam)
        b.expU, b.varU, b.expV, b.varV = (a.copy() for a in mom)
        for which, d in enumerate(C.DIRS):
            want_a, want_v, g = C.expected(case, fam, d, M, mom)
            want = np.concatenate([want_a, want_v], axis=1)
            got64 = np.concatenate(b.masked_sums(which), axis=1)
            got = got64.astype(np.float32)
            assert np.array_equal(got.astype(np.float64), got64)                  # (the hook hands fp32 sums on as doubles)
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                failures.append(C.first_mismatch(case, fam, d, which, got, want, g))
            again = np.concatenate(b.masked_sums(which), axis=1)
            if not np.array_equal(again, got64):
                failures.append("%s family %s %s: a second call on the same handle returns other bits (%d elements)" % (
                    case.id, fam, d, int((again != got64).sum())))
    b.close()
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- the posted column maxima
# Row counts of a factor.  gram_reduce_kernel's maxima block walks the nblk = ceil(rows / 32) partials of post_kernel eight groups
# x eight in flight: nblk = 1, 8, 9, 63, 64, 65, 129 (and 128).  vb_colmax_kernel's trip is 256 blocks x nsub sub-rows x 4 rows in
# flight = 4096 rows at KP = 32, 2048 at KP = 64: rows at both edges of one and of two trips.
MAXIMA_SHAPES = [(4097, 17), (4096, 256), (4095, 257), (2049, 2016), (2048, 2047)]


def test_the_maxima_shapes_cover_the_strides():
    rows = sorted(r for s in MAXIMA_SHAPES for r in s)
    assert {-(-r // 32) for r in rows} >= {1, 8, 9, 63, 64, 65, 129}
    for trip in (2048, 4096):
        assert {trip - 1, trip, trip + 1} <= set(rows)


def _peak_rows(rows, count):
    """`count` rows for the columns' maxima: the first block, the last (partial) block, blocks 62-65, block edges, then rows spread
    over the factor -- all different while the factor has that many rows"""
    first = [0, rows - 1, 31, 32, (rows - 1) // 32 * 32] + [32 * blk + 5 + blk % 7 for blk in (62, 63, 64, 65, 7, 8, 127, 128)]
    out = []
    for r in first + [(k * 7919 + 11) % rows for k in range(4 * count)] + list(range(rows)):
        if 0 <= r < rows and r not in out:
            out.append(r)
        if len(out) == count:
            break
    while len(out) < count:                                                    # (fewer rows than columns: round again)
        out.append(out[len(out) % rows])
    return out


def _peaked_moments(rows, K, rs):
    """exp / var with the maximum of every S2 column and of every E^2 column in a row of its own"""
    ex = rs.uniform(0.1, 1.0, (rows, K)); var = rs.uniform(0.01, 1.0, (rows, K))
    peaks = _peak_rows(rows, 2 * K)
    for k in range(K):
        ex[peaks[2 * k + 1], k] = 3.0 + 0.01 * k; var[peaks[2 * k + 1], k] = 0.5        # E^2 ~ 9, S2 ~ 9.5
        var[peaks[2 * k], k] = 20.0 + k                                                # S2 > 20
    return ex.astype(np.float32).astype(np.float64), var.astype(np.float32).astype(np.float64), peaks


def _want_maxima(ex, var):
    K = ex.shape[1]
    x = C.operand(ex, var)
    return x.max(0).view(np.uint32).reshape(2, K), x.argmax(0).reshape(2, K)


@pytest.mark.parametrize("K", [7, 40], ids=["KP32", "KP64"])
@pytest.mark.parametrize("I,J", MAXIMA_SHAPES, ids=["%dx%d" % s for s in MAXIMA_SHAPES])
def test_the_relayout_posts_the_column_maxima(monkeypatch, I, J, K):
    monkeypatch.setenv("BNMTF_VB_PATH", "masked")                              # (read when the model is built: both directions post)
    rs = np.random.RandomState(I + 3 * K)
    M = (rs.rand(I, J) >= 0.3).astype(np.float64)
    M[0, :] = 1; M[:, 0] = 1
    b = bnmf_vb_optimised(rs.rand(I, J), M, K, PRI, verbose=False)
    b.initialise('exp')
    b.expU, b.varU, pU = _peaked_moments(I, K, rs)
    b.expV, b.varV, pV = _peaked_moments(J, K, rs)
    for which, (ex, var, peaks, rows) in enumerate([(b.expU, b.varU, pU, I), (b.expV, b.varV, pV, J)]):
        want, where = _want_maxima(ex, var)
        if rows >= 2 * K:
            assert len(set(where.ravel())) == 2 * K                            # a different row for every column's maximum
            blocks = set(where.ravel() // 32)
            assert {0, (rows - 1) // 32} <= blocks and {blk for blk in (62, 63, 64, 65) if 32 * blk + 12 < rows} <= blocks
        posted, own, flag = b.column_maxima(which)
        assert flag, "the relayout of factor %d did not post its maxima" % which
        for name, got in (("posted", posted), ("own", own)):
            bad = np.argwhere(got != want)
            assert len(bad) == 0, "factor %d (%d rows, nblk = %d), %s maxima: %d of %d differ; first: %s column %d, maximum in row %d (block %d): expected bits %08x, got %08x" % (
                which, rows, -(-rows // 32), name, len(bad), want.size, ("S2", "E^2")[bad[0][0]], bad[0][1], where[tuple(bad[0])], where[tuple(bad[0])] // 32,
                want[tuple(bad[0])], got[tuple(bad[0])])
        again = b.column_maxima(which)                                        # read-only: the same answer, the flag still up
        assert np.array_equal(again[0], posted) and np.array_equal(again[1], own) and again[2]
    b.close()


@pytest.mark.parametrize("K", [7, 40], ids=["KP32", "KP64"])
def test_a_half_sweep_posts_the_maxima_of_the_new_moments(monkeypatch, K):
    from bnmtf_amd.synthetic import generate_bnmf
    monkeypatch.setenv("BNMTF_VB_PATH", "masked")
    I, J = 300, 200
    R, M, _, _ = generate_bnmf(I, J, K, 0.3, seed_data=3, seed_mask=4)
    b = bnmf_vb_optimised(R, M, K, PRI, verbose=False)
    b.initialise('exp')
    for which in (0, 1):
        before, own0, flag = b.column_maxima(which)
        assert flag and np.array_equal(before, own0)
        _lib.check(_lib.lib().bnmf_vb_half_sweep(b._handle(), which))        # rewrites the factor and relays it out
        b._pull()
        posted, own, flag = b.column_maxima(which)
        assert flag and "vb_sweep=masked" in b.describe(), b.describe()
        assert np.array_equal(posted, own)                                    # both from the device's new S2 and exp
        ex, var = (b.expU, b.varU) if which == 0 else (b.expV, b.varV)
        want, _ = _want_maxima(ex, var)
        assert np.array_equal(posted[1], want[1])                             # E^2: the square of the new fp32 exp
        assert np.all(posted[1] != before[1]) and np.all(posted[0] != before[0])        # ... not the old moments'
        # S2 is formed on the device (var + exp^2 in fp32, its rounding the kernel's own): the host's restatement to a few ulp
        s2 = posted[0].view(np.float32).astype(np.float64); ref = want[0].view(np.float32).astype(np.float64)
        assert np.all(np.abs(s2 - ref) <= 4 * 2.0 ** -24 * ref)
    b.close()
