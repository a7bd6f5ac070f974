"""Inputs and restatements for the tests of bnmtf_amd.fold_in (NumPy, no GPU).

case(...)          the inputs of one launch shape: a fixed factor, the new units' entries (given in a shuffled order), rates 1
conditionals(...)  fp64: (mu, tau_p, dmu) of every (unit, column), conditioned on a given state -- column k sees new[:, :k] and
                   prev[:, k:] -- with the bound dmu = 2e-5 scale / tau_p + 1e-6 and the absolute-value sum `scale` of
                   _draw_explainer._factor_pass (the bound test_bnmf_gibbs_gpu.py holds a half sweep's mu to)
fp64_mode_chain    the ICM chain in fp64
fp32_chain(...)    the device's chain restated in np.float32 in the manner of test_draw_explainer_cpu.fp32_device_run: numerator and
                   precision from the chain's own state in fp64, rounded to fp32 with fp32-sized noise (4e-6 of the cancelling
                   terms: a fifth of the bound), then device_rng.h's tn_params / tn_candidate / tn_guard operation by operation
"""
import numpy as np

from oracle import rng
from bnmtf_amd import Entries

f32 = np.float32
STREAM = 4                       # kStreamFoldIn
SEED = 20240611
TAU = 2.0
ELEM0 = 1000                     # the tests' ids are arange + ELEM0
C_MU = 2e-5

COUNTS_A = (1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1100)      # every slot class, both sides of the register / long boundary
COUNTS_B = (1, 7, 63, 64, 65, 83, 2, 40, 83)
RANKS_B = (1, 4, 5, 32, 64, 65, 255, 256)
SHAPES = [("a", 1200, 3, COUNTS_A)] + [("b%d" % W, 83, W, COUNTS_B) for W in RANKS_B]


class Case(object):
    """other [m][W] (fp32-representable), new: Entries (n, m) in a shuffled order, R, M: the same dense [n][m], lam [n][W], x0"""

    def __init__(self, m, W, counts, seed):
        rs = np.random.RandomState(seed)
        n, k = len(counts), min(W, 8)
        self.m, self.W, self.n, self.counts = m, W, n, tuple(counts)
        self.other = rs.exponential(1.0, (m, W)).astype(f32).astype(np.float64)
        truth = rs.exponential(1.0, (n, k))
        full = (truth @ self.other[:, :k].T).astype(f32).astype(np.float64)        # non-negative, of rank min(W, 8)
        self.M = np.zeros((n, m))
        for q, c in enumerate(counts):
            self.M[q, rs.choice(m, size=c, replace=False)] = 1.0
        self.R = full * self.M
        rows, cols = np.nonzero(self.M)
        self.sorted = Entries((n, m), rows, cols, self.R[rows, cols])
        order = rs.permutation(len(rows))
        self.new = Entries((n, m), rows[order], cols[order], self.R[rows, cols][order])
        self.lam = np.ones((n, W))
        self.x0 = 1.0 / self.lam
        self.ids = (np.arange(n) + ELEM0).astype(np.uint32)

    def unit(self, q):
        """unit q alone: (Entries (1, m), its id)"""
        cols = np.flatnonzero(self.M[q])
        return Entries((1, self.m), np.zeros(len(cols), dtype=np.int32), cols, self.R[q, cols]), self.ids[q:q + 1]


_CASES = {}


def case(name):
    if name not in _CASES:
        for seed, (nm, m, W, counts) in enumerate(SHAPES):
            if nm == name:
                _CASES[name] = Case(m, W, counts, 100 + seed)
    return _CASES[name]


def conditionals(c, prev, new, tau=TAU):
    """fp64 (mu, tau_p, dmu), each [n][W]: column k conditioned on new[:, :k] and prev[:, k:] (_factor_pass's formulas)"""
    X = np.array(prev, dtype=np.float64); new = np.asarray(new, dtype=np.float64)
    Y, M, R = c.other, c.M, c.R
    MR = M * np.abs(R)
    E = M * (R - X @ Y.T)
    mu, tp, dmu = np.zeros(X.shape), np.zeros(X.shape), np.zeros(X.shape)
    for k in range(c.W):
        y = Y[:, k]
        g = M @ (y * y)
        tp[:, k] = tau * g
        numer = -c.lam[:, k] + tau * (E @ y + X[:, k] * g)
        scale = tau * (MR @ np.abs(y) + np.abs(X) @ np.abs(Y.T @ y))
        with np.errstate(all="ignore"):
            mu[:, k] = numer / tp[:, k]
            dmu[:, k] = np.where(tp[:, k] > 0, C_MU * scale / tp[:, k], 0.0) + 1e-6
        E -= M * np.outer(new[:, k] - X[:, k], y)
        X[:, k] = new[:, k]
    return mu, tp, dmu


def fp64_mode_chain(c, T, tau=TAU, min_x=0.0):
    """the ICM chain in fp64: [T][n][W]"""
    X = c.x0.copy()
    out = []
    for _ in range(T):
        E = c.M * (c.R - X @ c.other.T)
        for k in range(c.W):
            y = c.other[:, k]
            g = c.M @ (y * y)
            mu = (-c.lam[:, k] + tau * (E @ y + X[:, k] * g)) / (tau * g)
            x = np.maximum(np.maximum(0.0, mu), min_x)
            E -= c.M * np.outer(x - X[:, k], y)
            X[:, k] = x
        out.append(X.copy())
    return np.array(out)


def tn_draw_f32(mu, tau_p, elem, col, it, seed):
    """device_rng.h's tn_params / tn_candidate / tn_guard in np.float32, the candidates in order: the first accepted one"""
    mu = np.asarray(mu, dtype=f32); tau_p = np.asarray(tau_p, dtype=f32)
    elem = np.asarray(elem)
    n = mu.size
    with np.errstate(all="ignore"):
        live = tau_p > 0
        rt = np.sqrt(np.where(live, tau_p, f32(1.0))).astype(f32)
        a = (-mu * rt).astype(f32)
        live &= np.isfinite(a)
        d = (f32(2.0) / (np.sqrt(a * a + f32(4.0)).astype(f32) + a)).astype(f32)
        lam = (a + d).astype(f32)
        tail = a >= f32(0.25)
    out = np.zeros(n, dtype=f32)
    todo = np.nonzero(live)[0]
    cand = 0
    while todo.size and cand < 4096:
        r0, r1, _, _ = rng.philox4x32_10(elem[todo], col, it, STREAM + 16 * cand, seed)
        u1 = rng.u23(r0).astype(f32); u2 = rng.u23(r1).astype(f32)
        with np.errstate(all="ignore"):
            nl = (-np.log(u1)).astype(f32)
            e = (nl / lam[todo]).astype(f32)
            t = (e - d[todo]).astype(f32)
            acc_t = u2 <= np.exp((f32(-0.5) * t * t).astype(f32)).astype(f32)
            x_t = (e / rt[todo]).astype(f32)
            z = (np.sqrt((f32(2.0) * nl).astype(f32)).astype(f32) * np.cos((f32(6.283185307179586) * u2).astype(f32)).astype(f32)).astype(f32)
            acc_n = z >= a[todo]
            x_n = (mu[todo] + (z / rt[todo]).astype(f32)).astype(f32)
        acc = np.where(tail[todo], acc_t, acc_n)
        x = np.where(tail[todo], x_t, x_n).astype(f32)
        x = np.where(np.isfinite(x) & (x >= 0), x, f32(0.0)).astype(f32)
        out[todo[acc]] = x[acc]
        todo = todo[~acc]
        cand += 1
    return out


def fp32_chain(c, T, update='draw', seed=SEED, ids=None, it0=0, tau=TAU, min_x=0.0, noise_seed=4):
    """The device's chain restated (see the module's text): fp32 [T][n][W]."""
    ids = c.ids if ids is None else ids
    nrs = np.random.RandomState(noise_seed)
    X = c.x0.astype(f32).astype(np.float64)
    Y, M, R = c.other, c.M, c.R
    MR = M * np.abs(R)
    out = []
    for t in range(T):
        E = M * (R - X @ Y.T)
        for k in range(c.W):
            y = Y[:, k]
            g = M @ (y * y)
            scale = tau * (MR @ np.abs(y) + np.abs(X) @ np.abs(Y.T @ y))
            numer = f32(-c.lam[:, k] + tau * (E @ y + X[:, k] * g) + 4e-6 * scale * nrs.uniform(-1, 1, c.n))
            tau_p = f32(tau * g * (1.0 + 2e-7 * nrs.uniform(-1, 1, c.n)))
            with np.errstate(all="ignore"):
                mu = (numer / tau_p).astype(f32)
            if update == 'draw':
                x = tn_draw_f32(mu, tau_p, ids, k, it0 + t, seed)
            else:
                x = np.maximum(np.where((tau_p > 0) & (mu > 0), mu, f32(0.0)), f32(min_x)).astype(f32)
            x = x.astype(np.float64)
            E -= M * np.outer(x - X[:, k], y)
            X[:, k] = x
        out.append(X.astype(f32))
    return np.array(out)


def explain(c, samples, x0=None, it0=0, seed=SEED, elem0=ELEM0, tau=TAU):
    """Every draw of the chain `samples` [T][n][W] explained by the oracle's candidate sequence, conditioned on the chain's own
    states: _draw_explainer._factor_pass with stream 4.  Returns the Explained."""
    import _draw_explainer as X
    out = X.Explained(seed)
    MR = c.M * np.abs(c.R)
    prev = np.array(c.x0.astype(f32) if x0 is None else x0, dtype=np.float64)
    for t in range(len(samples)):
        state = prev.copy()
        E = c.M * (c.R - state @ c.other.T)
        X._factor_pass(out, "X", state, c.other, E, c.M, MR, c.lam, tau, np.asarray(samples[t]), elem0, 0, it0 + t, STREAM, seed, C_MU)
        prev = np.array(samples[t], dtype=np.float64)
    return out
