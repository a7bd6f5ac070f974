"""CPU model of the arithmetic in bnmtf_amd/csrc/kernel_maskgemm.hip (the variational sweep's chain-independent masked sums,
bnmf_vb_optimised.py:189-199): per-column fixed-point grid, balanced base-256 digits, integer accumulation, one rounding at the
end.  Checks the statements the kernel's header makes -- digit ranges (int8 operands), exact reconstruction, the accumulators'
range (int32), the error bound against the fp64 sum -- without a GPU; tests/test_bnmf_vb_gpu.py holds the device against the
same bound through bnmf_vb_masked_sums, and tests/test_masked_product_exact_gpu.py to the bits of the model (planes, masked_sums and
their slab-aware form: tests/_masked_product_cases.py)."""
import numpy as np

from _masked_product_cases import masked_sums, planes     # (the model, shared with the exact tests of the product: test_masked_product_*)


def test_digit_planes_are_int8_and_exact():
    rs = np.random.RandomState(0)
    x = (10.0 ** rs.uniform(-8, 3, (4096, 24))).astype(np.float32)
    x[::7, 3] = 0.0; x[:, 5] = 0.0                                                    # zeros and an all-zero column
    x[11, 7] = np.float32(2.0) ** 100; x[12, 8] = np.float32(2.0) ** -120             # a huge and a tiny column maximum
    e, d0, d1, d2, n = planes(x)
    assert d0.min() >= 0 and d0.max() <= 64 and d1.min() >= -128 and d1.max() <= 127 and d2.min() >= -128 and d2.max() <= 127
    assert np.array_equal(d0 * 65536 + d1 * 256 + d2, n) and n.min() >= 0 and n.max() <= 2 ** 22
    # the grid: 2^(e-1) <= max < 2^e for every non-zero column; an element is off by at most half a grid step
    mx = x.max(0).astype(np.float64)
    nz = mx > 0
    assert np.all(mx[nz] < np.ldexp(1.0, e[nz])) and np.all(mx[nz] >= np.ldexp(1.0, e[nz] - 1))
    err = np.abs(np.ldexp(n.astype(np.float64), (e - 22)[None, :]) - x.astype(np.float64))
    assert np.all(err <= np.ldexp(1.0, e - 23)[None, :] * (1 + 1e-12))


def test_masked_sums_model_against_fp64_and_accumulator_range():
    rs = np.random.RandomState(1)
    rows, units, cols = 8192, 96, 16
    x = (10.0 ** rs.uniform(-5, 1, (rows, cols))).astype(np.float32)
    miss = rs.rand(units, rows) < 0.1
    miss[0] = True                                                                     # a unit with every entry missing: the accumulators' worst case
    got, (D0, D1, D2) = masked_sums(miss, x)
    for D in (D0, D1, D2):
        assert np.abs(D).max() < 2 ** 31                                               # fits the int32 accumulator tiles (8192 x 128 at most)
        assert np.abs(D).max() < 2 ** 24                                               # ... and converts to fp32 exactly
    ref = miss.astype(np.float64) @ x.astype(np.float64)
    n_miss = miss.sum(1)[:, None]
    bound = n_miss * x.max(0).astype(np.float64)[None, :] * 2.0 ** -22 + 1.2e-7 * ref
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
    # the order of the additions does not matter (integers): any split of the inner range gives the same digits sums
    half = rows // 2
    e, d0, d1, d2, _ = planes(x)
    mi = miss.astype(np.int64)
    assert np.array_equal(mi[:, :half] @ d0[:half] + mi[:, half:] @ d0[half:], D0)
    # typical accuracy: ~sqrt(n) half-steps -- an order below the fp32 rounding of the sums the sweep forms beside it
    big = ref > 1e-2 * ref.max()
    assert (np.abs(got.astype(np.float64) - ref)[big] / ref[big]).max() < 3e-7
