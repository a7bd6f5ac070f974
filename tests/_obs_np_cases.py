"""The launch shapes of the non-probabilistic models on the observed-entry layout (csrc/kernel_obs_np.hip) that
tests/test_obs_np_gpu.py runs: positive data and starting points on the masks of _obs_cases.SHAPES -- units of 1, 2, 63 .. 65,
127 .. 129, 255 .. 257 and 511 .. 513 entries as rows and as columns, the full matrix and its long form, I and J at 1, 3, 4 and 5,
K in {1, 2, 31, 32, 33, 63, 64, 65, 130} -- and, beyond them, K = 256, a 1 029 x 7 mask and its transpose (more than 256 blocks in
the end-of-iteration fold and in the S pass) and NMTF's ranks on the row-count and column-count masks."""
import numpy as np

import _obs_cases as OC

# mask name -> () -> (M, K) for NMF
NMF_SHAPES = dict(OC.SHAPES)
NMF_SHAPES["K256"] = lambda: (OC._random_mask(40, 37, 0.5, 30 + 256), 256)
NMF_SHAPES["tall_1029x7"] = lambda: (OC._random_mask(1029, 7, 0.6, 77), 3)
NMF_SHAPES["wide_7x1029"] = lambda: (OC._random_mask(1029, 7, 0.6, 77).T.copy(), 3)

TRI_RANKS = ((1, 1), (3, 11), (7, 3), (33, 5), (5, 130))
# case name -> () -> (M, K, L) for NMTF
NMTF_SHAPES = {}
for _mask in ("row_counts", "col_counts"):
    for _K, _L in TRI_RANKS:
        NMTF_SHAPES["%s_K%d_L%d" % (_mask, _K, _L)] = (lambda m=_mask, k=_K, l=_L: (OC.SHAPES[m]()[0], k, l))
NMTF_SHAPES["tall_1029x7_K3_L2"] = lambda: (OC._random_mask(1029, 7, 0.6, 77), 3, 2)
NMTF_SHAPES["wide_7x1029_K2_L3"] = lambda: (OC._random_mask(1029, 7, 0.6, 77).T.copy(), 2, 3)
NMTF_SHAPES["full_matrix_long_K2_L3"] = lambda: (np.ones((3, 600)), 2, 3)


def nmf_problem(M, K, seed=5):
    """R = A B^T (0.8 + 0.4 rand) as _np_restatement.edge_problem makes it, and a starting point with every factor >= 0.1."""
    I, J = M.shape
    rs = np.random.RandomState(seed)
    R = rs.rand(I, K) @ rs.rand(J, K).T * (0.8 + 0.4 * rs.rand(I, J))
    return R, rs.rand(I, K) + 0.1, rs.rand(J, K) + 0.1


def nmtf_problem(M, K, L, seed=5):
    I, J = M.shape
    rs = np.random.RandomState(seed)
    R = rs.rand(I, K) @ rs.rand(K, L) @ rs.rand(J, L).T * (0.8 + 0.4 * rs.rand(I, J))
    return R, rs.rand(I, K) + 0.1, rs.rand(K, L) + 0.1, rs.rand(J, L) + 0.1


def nmf_model(R, M, K, U0, V0, **kw):
    from bnmtf_amd import NMF
    m = NMF(R, M, K, verbose=False, **kw)
    m.U, m.V = U0.copy(), V0.copy()
    return m


def nmtf_model(R, M, K, L, F0, S0, G0, **kw):
    from bnmtf_amd import NMTF
    m = NMTF(R, M, K, L, verbose=False, **kw)
    m.F, m.S, m.G = F0.copy(), S0.copy(), G0.copy()
    return m


# what the bit-for-bit child processes run (BNMTF_OBS_LONG=1 against the default): long units in the row sweep, in the column
# sweep with its end-of-iteration sums, and in NMTF's three steps
BITS_NMF = ("row_counts", "col_counts")
BITS_NMTF = ("row_counts_K3_L11",)


def bits_runs():
    """name -> arrays of two iterations of every bit-for-bit case (factors, performances, I-divergence per iteration)."""
    out = {}
    for name in BITS_NMF:
        M, K = NMF_SHAPES[name]()
        R, U0, V0 = nmf_problem(M, K)
        m = nmf_model(R, M, K, U0, V0, layout='observed')
        m.run(2)
        out[name + "_U"], out[name + "_V"] = m.U, m.V
        out[name + "_perf"] = np.array([m.all_performances[k] for k in ("MSE", "R^2", "Rp")])
        out[name + "_idiv"] = np.array([m.compute_I_div()])
        m.close()
    for name in BITS_NMTF:
        M, K, L = NMTF_SHAPES[name]()
        R, F0, S0, G0 = nmtf_problem(M, K, L)
        m = nmtf_model(R, M, K, L, F0, S0, G0, layout='observed')
        m.run(2)
        out[name + "_F"], out[name + "_S"], out[name + "_G"] = m.F, m.S, m.G
        out[name + "_perf"] = np.array([m.all_performances[k] for k in ("MSE", "R^2", "Rp")])
        out[name + "_idiv"] = np.array([m.compute_I_div()])
        m.close()
    return out
