"""The launch shapes of the observed-entry sweep kernel (csrc/kernel_obs.hip) that tests/test_obs_gpu.py runs, and the two
runs its child processes repeat: seeded masks, data and initial states.  The smallest shapes at which the kernel can go wrong:
units of 1 .. 129 entries, units at, one below and one above every register-slot instantiation's capacity and the long-form
threshold, I and J around the units per block, a full row and a full matrix, ranks around the 64-lane steps of the row staging."""
import numpy as np

from bnmtf_amd import bnmf_gibbs_optimised

PRI = dict(alpha=1., beta=1., lambdaU=0.5, lambdaV=0.5)
WAVES = 4                        # csrc/kernels.h kObsWaves: units per block
SLOT_CAPS = (64, 128, 256, 512)  # entries of the register form's instantiations (1, 2, 4, 8 slots per lane); 512 = the long form's threshold


def _problem(M, K, seed):
    """Seeded data and an initial state for the mask M (factors at least 0.1: every conditional's precision is well away from zero)."""
    I, J = M.shape
    rs = np.random.RandomState(seed)
    R = rs.exponential(1.0, (I, 4)) @ rs.exponential(1.0, (J, 4)).T + rs.randn(I, J)
    return R, rs.exponential(0.3, (I, K)) + 0.1, rs.exponential(0.3, (J, K)) + 0.1


def _counts_mask(counts, J, seed):
    """A mask whose row u has counts[u] entries at seeded columns; the rows behind them are full, so no column is empty."""
    rs = np.random.RandomState(seed)
    M = np.zeros((len(counts) + 2, J))
    for u, c in enumerate(counts):
        M[u, rs.choice(J, size=c, replace=False)] = 1
    M[len(counts):] = 1
    return M


def _random_mask(I, J, frac, seed):
    rs = np.random.RandomState(seed)
    M = (rs.rand(I, J) < frac).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return M


ROW_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129] + [c + d for c in SLOT_CAPS[2:] for d in (-1, 0, 1)]        # ... and 255 .. 257, 511 .. 513
SHAPES = {
    # rows of 1 .. 129 entries and at, one below, one above every register-slot capacity and the long-form threshold; two full rows
    "row_counts": lambda: (_counts_mask(ROW_COUNTS, 520, 1), 5),
    # the same units as columns
    "col_counts": lambda: (_counts_mask(ROW_COUNTS, 520, 2).T.copy(), 5),
    "full_matrix": lambda: (np.ones((9, 11)), 3),
    "full_matrix_long": lambda: (np.ones((3, 600)), 2),
}
for _n in (1, WAVES - 1, WAVES, WAVES + 1):
    SHAPES["I%d" % _n] = (lambda n=_n: (_random_mask(n, 7, 0.6, 10 + n), 3))
    SHAPES["J%d" % _n] = (lambda n=_n: (_random_mask(7, n, 0.6, 20 + n), 3))
for _k in (1, 2, 31, 32, 33, 63, 64, 65, 130):
    SHAPES["K%d" % _k] = (lambda k=_k: (_random_mask(40, 37, 0.5, 30 + k), k))


def _mode_iteration(M, K, seed=5, **kw):
    R, U0, V0 = _problem(M, K, seed)
    b = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, layout='observed', **kw)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(1, update='mode')
    out = (b.all_U[0].copy(), b.all_V[0].copy(), float(b.all_tau[0]), [b.all_performances[m][0] for m in ("MSE", "R^2", "Rp")], b.describe())
    b.close()
    return R, U0, V0, out


def _draw_iterations(M, K):
    R, U0, V0 = _problem(M, K, 5)
    b = bnmf_gibbs_optimised(R, M, K, PRI, verbose=False, layout='observed', seed=123)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.3
    b.run(3)
    out = (b.all_U.copy(), b.all_V.copy(), b.all_tau.copy(), np.array([b.all_performances[m] for m in ("MSE", "R^2", "Rp")]))
    b.close()
    return out
