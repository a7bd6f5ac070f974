"""The cases of tests/test_draws_explained_gpu.py: per kernel form the smallest shapes that reach its edges, with ragged masks
and STEERED prior rates (_draw_explainer.steer_lambda) so that the draws' standardised bounds a land where the sampler goes
wrong unnoticed: half of them in [0.10, 0.24] (acceptance ~ 0.42: walks far past a kernel's first candidate batch), the rest
on both sides of the regime switch and deep in either regime.  tests/test_draw_explainer_cpu.py checks without a GPU that the
oracle's own chain on these inputs meets every case's ambiguity cap and every form's coverage counts.

Everything the device is handed is fp32-representable (data, initial state, rates), so the fp64 conditionals the explainer
forms are those of the numbers the device holds."""
import functools

import numpy as np

from _draw_explainer import steer_lambda

ITERATIONS = 3
SEED = 20251

# first candidate batch of a form's sampler, read from the kernels: the chip kernels (sweep_chip.inc, kernel_sweep_unit.hip
# kUnitCands, kernel_sweep_turns.hip) test four table candidates per draw; kernel_small.hip's factor sweeps one (nc0); the generic
# sweep (kernel_sweep.hip) and the observed-entry kernel (kernel_obs.hip) a whole wave's 64; every S step four (stab / NH).
BATCH = {"small": 1, "unit": 4, "pairs": 4, "wide": 4, "twin": 4, "turns": 4, "blocks": 4, "generic": 64, "obs": 64, "obs_long": 64}
S_BATCH = 4


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _ragged_mask(rs, I, J, lo, hi):
    """row i misses a fraction between lo and hi of its entries (tests/test_wide_sweep_gpu.py)"""
    M = np.ones((I, J))
    for i in range(I):
        f = lo + (hi - lo) * rs.rand()
        M[i, rs.choice(J, int(f * J), replace=False)] = 0
    M[rs.randint(I, size=J), np.arange(J)] = 1
    return M


def _sparse_mask(rs, I, J, frac, long_row):
    M = (rs.rand(I, J) < frac).astype(float)
    if long_row:                                   # one unit above the long form's threshold of 512 entries
        M[0, :] = 0; M[0, rs.choice(J, long_row, replace=False)] = 1
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return M


def _tau0(prec_rows, x2_rows, prec_cols, x2_cols):
    """The noise level of a case's data: tau = 1 / sigma^2 at which a conditional's standard deviation 1 / sqrt(tau_p) is about
    the factors' own size in both directions (prec: tau_p / tau of the initial state, x2: the factor's size squared, _size2).  With less
    noise the steered first sweep -- most of its draws at a > 0, i.e. of size 1 / sqrt(tau_p) -- shrinks the factors, the next
    sweep's precisions shrink with them and every later draw sits deep in the tail regime; with this much, a = (lambda - tau
    numer) / sqrt(tau_p) of the later sweeps stays within a few units of its steered value, so both regimes and long candidate
    walks occur in every iteration."""
    return float(np.float32(1.0 / np.sqrt(prec_rows.mean() * x2_rows * prec_cols.mean() * x2_cols)))


LEVEL = 1.25         # the data's level over the initial product's: see bnmf_inputs
TN_MEAN = 0.81       # E[x sqrt(tau_p)] of a draw under the steering mixture of targets: sum over the mixture of pdf(a) / sf(a) - a


def _size2(X0):
    """the size 1 / tau_p is matched to: a steered draw's mean TN_MEAN / sqrt(tau_p) then equals the initial factor's mean, so the
    first sweep leaves the product's level where the data have it (a level shift is coherent with every later regressor)"""
    return (X0.mean() / TN_MEAN) ** 2


@functools.lru_cache(maxsize=None)
def bnmf_inputs(I, J, K, lo, hi, zero_col=-1, sparse=0.0, long_row=0):
    """(R, M, (U0, V0, tau0), (lambdaU, lambdaV)) of a two-factor case.  zero_col >= 0: that column of V0 is zero (tau_p = 0:
    the U draws of the column are the guarded 0).  sparse > 0: that share observed (the observed-entry layout's cases).  The data
    are the initial state's own product plus noise: the first sweep's residual has no part that is coherent with a regressor
    (which would push tau numer / sqrt(tau_p) -- and with it the reachable a -- to one side)."""
    rs = np.random.RandomState(1000 * I + 10 * J + K)
    M = _sparse_mask(rs, I, J, sparse, long_row) if sparse > 0 else _ragged_mask(rs, I, J, lo, hi)
    sc = np.sqrt(min(K, 8) / float(K))
    U0 = _f32(rs.exponential(sc, (I, K))); V0 = _f32(rs.exponential(sc, (J, K)))
    tau0 = _tau0(M @ V0 ** 2, _size2(U0), M.T @ U0 ** 2, _size2(V0))
    R = _f32(LEVEL * (U0 @ V0.T) + rs.randn(I, J) / np.sqrt(tau0))
    if zero_col >= 0:
        V0[:, zero_col] = 0.0
    init = (U0, V0, tau0)
    lamU, lamV = steer_lambda(R, M, init, SEED, rs)
    return R, M, init, (_f32(lamU), _f32(lamV))


@functools.lru_cache(maxsize=None)
def bnmtf_inputs(I, J, K, L):
    rs = np.random.RandomState(1000 * I + 10 * J + K + 7 * L)
    M = _ragged_mask(rs, I, J, 0.0, 0.4)
    sS = 1.0 / np.sqrt(K * L / 4.0)
    F0 = _f32(rs.exponential(1.0, (I, K))); S0 = _f32(rs.exponential(sS, (K, L))); G0 = _f32(rs.exponential(1.0, (J, L)))
    tau0 = _tau0(M @ ((S0 @ G0.T) ** 2).T, _size2(F0), M.T @ ((F0 @ S0) ** 2), _size2(G0))
    R = _f32(LEVEL * (F0 @ S0 @ G0.T) + rs.randn(I, J) / np.sqrt(tau0))
    init = (F0, S0, G0, tau0)
    lamF, lamS, lamG = steer_lambda(R, M, init, SEED, rs)
    return R, M, init, (_f32(lamF), _f32(lamS), _f32(lamG))


def _c(id, form, shape, env=None, path=None, experiment=False, **kw):
    return dict(id=id, form=form, shape=shape, env=env or {}, path=path, experiment=experiment, kw=kw)


# (I, J, K, lo, hi): ragged mask between lo and hi missing per row
BNMF_CASES = [
    _c("small-37x29k5", "small", (37, 29, 5, 0.0, 0.4), path="small"),
    _c("small-100x80k10", "small", (100, 80, 10, 0.0, 0.4), path="small", zero_col=3),
    _c("small-130x97k32", "small", (130, 97, 32, 0.0, 0.4), path="small"),
    _c("unit-192x130k12", "unit", (192, 130, 12, 0.0, 0.5), path="multi", zero_col=5),
    _c("unit-257x201k32", "unit", (257, 201, 32, 0.0, 0.5), path="multi"),
    _c("pairs-192x130k12", "pairs", (192, 130, 12, 0.0, 0.5), env={"BNMTF_UNIT": "0"}, path="multi", zero_col=5),
    _c("pairs-150x77k64", "pairs", (150, 77, 64, 0.0, 0.6), env={"BNMTF_UNIT": "0"}, path="multi"),
    _c("pairs-nw2-192x130k12", "pairs", (192, 130, 12, 0.0, 0.5), env={"BNMTF_UNIT": "0", "BNMTF_FAST_NW": "2"}, path="multi"),
    _c("pairs-nw4-192x130k12", "pairs", (192, 130, 12, 0.0, 0.5), env={"BNMTF_UNIT": "0", "BNMTF_FAST_NW": "4"}, path="multi"),
    _c("wide-ho1-513x389k32", "wide", (513, 389, 32, 0.05, 0.5), env={"BNMTF_WIDE": "1", "BNMTF_HANDOVER": "1"}, path="multi", zero_col=7),
    _c("wide-ho0-513x389k32", "wide", (513, 389, 32, 0.05, 0.5), env={"BNMTF_WIDE": "1", "BNMTF_HANDOVER": "0"}, path="multi"),
    _c("wide-ho1-640x800k64", "wide", (640, 800, 64, 0.0, 0.9), env={"BNMTF_WIDE": "1", "BNMTF_HANDOVER": "1"}, path="multi"),
    _c("wide-ho0-640x800k64", "wide", (640, 800, 64, 0.0, 0.9), env={"BNMTF_WIDE": "1", "BNMTF_HANDOVER": "0"}, path="multi"),
    _c("twin-513x389k32", "twin", (513, 389, 32, 0.05, 0.5), env={"BNMTF_WIDE": "1", "BNMTF_TWIN": "1"}, path="multi", experiment=True),
    _c("turns-513x389k32", "turns", (513, 389, 32, 0.05, 0.5), env={"BNMTF_WIDE": "1", "BNMTF_TURNS": "1"}, path="multi", experiment=True),
    _c("generic-130x97k7", "generic", (130, 97, 7, 0.0, 0.4), path="generic", zero_col=2),
    _c("generic-150x77k64", "generic", (150, 77, 64, 0.0, 0.6), path="generic"),
    _c("blocks-150x77k70", "blocks", (150, 77, 70, 0.0, 0.6), path="blocks", zero_col=66),
    _c("blocks-150x77k130", "blocks", (150, 77, 130, 0.0, 0.6), path="blocks"),
    _c("obs-300x260k9", "obs", (300, 260, 9, 0.0, 0.0), path="obs", sparse=0.1, zero_col=4),
    _c("obs-150x140k70", "obs", (150, 140, 70, 0.0, 0.0), path="obs", sparse=0.1),
    _c("obs-long-40x700k9", "obs_long", (40, 700, 9, 0.0, 0.0), path="obs", sparse=0.1, long_row=600, zero_col=4),
    _c("obs-forced-long-40x700k9", "obs_long", (40, 700, 9, 0.0, 0.0), env={"BNMTF_OBS_LONG": "1"}, path="obs", sparse=0.1, long_row=600),
]

# (I, J, K, L)
BNMTF_CASES = [
    _c("small-dense-60x40k6l10", "small_dense", (60, 40, 6, 10), path="small"),
    _c("small-dense-100x80k10l10", "small_dense", (100, 80, 10, 10), path="small"),
    _c("small-dense-80x60k9l10", "small_dense", (80, 60, 9, 10), path="small"),
    _c("small-other-60x40k12l7", "small_other", (60, 40, 12, 7), path="small"),
    _c("small-other-60x40k11l16", "small_other", (60, 40, 11, 16), path="small"),
    _c("ssys-130x97k10l10", "ssys", (130, 97, 10, 10), path="multi"),
    _c("ssys-130x97k32l17", "ssys", (130, 97, 32, 17), path="multi"),
    _c("rowwise-90x70k5l4", "rowwise", (90, 70, 5, 4), env={"BNMTF_SSYS": "0"}, path="multi"),
    _c("rowwise-90x70k20l16", "rowwise", (90, 70, 20, 16), env={"BNMTF_SSYS": "0"}, path="multi"),
    _c("wide-160x130k70l66", "wide_tri", (160, 130, 70, 66), path="blocks"),
]


def case_inputs(case):
    if len(case["shape"]) == 5:
        I, J, K, lo, hi = case["shape"]
        kw = case["kw"]
        return bnmf_inputs(I, J, K, lo, hi, kw.get("zero_col", -1), kw.get("sparse", 0.0), kw.get("long_row", 0))
    return bnmtf_inputs(*case["shape"])


def forms(cases):
    out = {}
    for c in cases:
        out.setdefault(c["form"], []).append(c)
    return out


AMBIGUITY_CAP = 0.01


def coverage_failures(form, batch, results, tri=False, blocks=None):
    """Assertion 4 of the issue for one kernel form, summed over its cases (results: the cases' Explained records), counted among
    the uniquely explained draws.  Returns the list of conditions that are not met (empty: covered).
      * >= 30 draws whose accepted candidate index is >= the form's first-batch size.  A first batch of 64 (the generic sweep,
        the observed-entry kernel) cannot be left by any input: the sampler's acceptance is at least 1 - Phi(0.25) = 0.40, so a
        draw goes past 64 candidates with probability 0.6^64 < 1e-14 -- for those forms the count is taken at index >= 4, which
        still walks the lanes of the batch, and "past the batch" is stated as unreachable rather than asserted.
      * >= 5 draws at index >= 8;  S steps: >= 10 draws at index >= 4 (S has at most K L draws per iteration).
      * both regimes hold >= 20 % of the draws each.
      * column blocks (blocks = [(c0, c1), ...] per result): every block contributes draws past its first batch."""
    fails = []
    fg = ("F", "G") if tri else None
    b = batch if batch < 64 else 4
    past_b = sum(r.past(b, fg) for r in results)
    past_8 = sum(r.past(8, fg) for r in results)
    if past_b < 30:
        fails.append("%s: %d draws at accepted index >= %d, want >= 30" % (form, past_b, b))
    if past_8 < 5:
        fails.append("%s: %d draws at accepted index >= 8, want >= 5" % (form, past_8))
    if tri:
        past_s = sum(r.past(S_BATCH, ("S",)) for r in results)
        if past_s < 10:
            fails.append("%s: %d S draws at accepted index >= %d, want >= 10" % (form, past_s, S_BATCH))
    n = [0.0, 0.0]
    tot = 0
    for r in results:
        u = int((r.unique() & (r["regime"] >= 0)).sum())
        sh = r.regime_shares()
        n[0] += sh[0] * u; n[1] += sh[1] * u; tot += u
    if min(n) < 0.2 * tot:
        fails.append("%s: regime shares %.3f / %.3f, want >= 0.2 each" % (form, n[0] / max(tot, 1), n[1] / max(tot, 1)))
    if blocks is not None:
        for r, ranges in zip(results, blocks):
            for (c0, c1) in ranges:
                if r.past(batch, None, (c0, c1)) == 0:
                    fails.append("%s: block (%d, %d) has no draw past its first batch" % (form, c0, c1))
    return fails


def oracle_bnmtf_chain(R, M, lams, init, seed, iterations):
    """oracle.BNMTFGibbsOracle's chain (same conditionals -- bnmtf_gibbs_optimised.py:195-211 --, same sampler and counter words)
    on the masked residual kept current by rank-one updates, as BNMFGibbsFairCPU does for the two-factor model: a K L = 4620
    S step costs O(I J) per entry instead of a full F S G^T product.  tests/test_draw_explainer_cpu.py holds it to the as-written
    oracle on a small case."""
    from oracle import rng
    lamF, lamS, lamG = lams
    F, S, G = (np.array(a, dtype=np.float64) for a in init[:3]); tau = float(init[3])
    I, J = R.shape; K, L = S.shape
    alpha_s = 1.0 + M.sum() / 2.0
    rows = np.arange(I); cols = np.arange(J)
    out = ([], [], [], [])
    for it in range(iterations):
        E = M * (R - F @ S @ G.T)
        for k in range(K):
            sg = S[k] @ G.T
            g = M @ (sg * sg)
            with np.errstate(all="ignore"):
                x = rng.tn_draw((-lamF[:, k] + tau * (E @ sg + F[:, k] * g)) / (tau * g), tau * g, rows, k, it, rng.STREAM_ROWS, seed)
            E -= M * np.outer(x - F[:, k], sg)
            F[:, k] = x
        for k in range(K):
            for l in range(L):
                mfg = M * np.outer(F[:, k], G[:, l])
                g = float((mfg * mfg).sum())           # (M is 0 / 1)
                tp = tau * g
                x = float(rng.tn_draw((-lamS[k, l] + tau * (float((E * mfg).sum()) + S[k, l] * g)) / tp if tp > 0 else 0.0, tp, 0, k * L + l, it, rng.STREAM_S, seed))
                E -= (x - S[k, l]) * mfg
                S[k, l] = x
        for l in range(L):
            fs = F @ S[:, l]
            g = (fs * fs) @ M
            with np.errstate(all="ignore"):
                x = rng.tn_draw((-lamG[:, l] + tau * (fs @ E + G[:, l] * g)) / (tau * g), tau * g, cols, l, it, rng.STREAM_COLS, seed)
            E -= M * np.outer(fs, x - G[:, l])
            G[:, l] = x
        tau = rng.gamma_draw(alpha_s, 1.0 + 0.5 * (E * E).sum(), it, seed)
        for o, v in zip(out, (F.copy(), S.copy(), G.copy(), tau)):
            o.append(v)
    return tuple(np.array(o) for o in out)
