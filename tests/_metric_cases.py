"""Cases of the exact tests of the fp64 metric sums (csrc/kernel_misc.hip: metric_kernel, metric_reduce_kernel) and a NumPy
model of the kernel's tiling.

The kernels stand behind bnmtf_metric_sums, bnmtf_metric_sums_wide, bnmtf_beta_s, bnmf_vb_exp_square_diff and
bnmf_vb_esd_terms: over a 0/1 mask they return n, sum R, sum R^2, sum P, sum P^2, sum R P (P = A B^T, or F S G^T) and, for the
variational model, sum_k [(varU + expU^2)(varV + expV^2) - expU^2 expV^2].  Launch: 32 x 32 tiles of R, a 32 x 8 block walking
four row groups, the contraction in chunks of 64 columns through LDS tiles of stride 65, the second-moment product on the same
tiles, then ONE block folding the tiles' partial sums 256 at a time.

Every case is on integers -- R in [-8, 8] (exact in the fp32 the handle stores), factors in [0, 7], S of a tri-factorisation
in [0, 3], VB moments exp in [0, 5] and var in [0, 3] -- so every product and every partial sum, in any order, is an integer
below 2^53 (test_metric_cases_cpu.py bounds them) and the only correct fp64 answer is the exact one.  The reference is integer
arithmetic entry by entry (reference()).

Seeds: R and the training mask of a shape come from RandomState(SEED + 1009 I + J); the factors of a case from
RandomState(SEED + 7919 index of the case); the 50 % mask of a case from RandomState(SEED + 104729 + index).
"""
import math

import numpy as np

SEED = 20261018
TWO24 = 2 ** 24
TWO53 = 2 ** 53
TILE, ROWGROUPS, CHUNK, STRIDE, FOLD = 32, 4, 64, 65, 256       # metric_kernel / metric_reduce_kernel

MASKS = ("train", "full", "empty", "corner", "last_row", "last_col", "tile_out", "half")


def tiles(I, J):
    return ((I + TILE - 1) // TILE) * ((J + TILE - 1) // TILE)


class Case:
    """family: plain (bnmtf_metric_sums on a handle of K = width), wide (bnmtf_metric_sums_wide), tri (a BNMTF handle, S
    given: K x L -> width L), state / state_tri (A = None: the factors the handle holds), vb (bnmf_vb_set_state, then
    bnmf_vb_exp_square_diff / bnmf_vb_esd_terms on the training mask)."""

    def __init__(self, family, I, J, K, L=0, train="seeded"):
        self.family, self.I, self.J, self.K, self.L, self.train = family, I, J, K, L, train
        self.index = None

    @property
    def width(self):
        return self.L if self.L else self.K

    @property
    def id(self):
        return "%s-%dx%d-%s%s" % (self.family, self.I, self.J, "%dx%d" % (self.K, self.L) if self.L else self.K,
                                 "" if self.train == "seeded" else "-" + self.train)

    @property
    def masks(self):
        return ("train",) if self.family == "vb" else MASKS


CASES = [
    # ---- plain: widths 1, 31, 63, 64 on handles of that K; I and J through 1, 31, 32, 33, 63, 64, 65, 130
    Case("plain", 1, 130, 31), Case("plain", 31, 33, 1), Case("plain", 32, 64, 64), Case("plain", 33, 31, 63),
    Case("plain", 63, 1, 64), Case("plain", 64, 65, 31), Case("plain", 65, 63, 1), Case("plain", 130, 32, 63),
    # the fold: 256 tiles (one `t += 256` round), 272 (two rounds), 257 (a one-tile tail)
    Case("plain", 512, 512, 1), Case("plain", 513, 512, 64), Case("plain", 3, 8200, 31),
    # ---- wide: 65, 127, 128, 129, 256 columns (two to four chunks, last chunk of 1, 63, 64 columns)
    Case("wide", 31, 33, 65), Case("wide", 33, 31, 127), Case("wide", 64, 65, 128), Case("wide", 65, 63, 129),
    Case("wide", 130, 32, 256), Case("wide", 1, 130, 129), Case("wide", 63, 1, 65), Case("wide", 32, 64, 127),
    Case("wide", 3, 8200, 65), Case("wide", 513, 512, 128),
    # ---- tri: (K, L) -> width L
    Case("tri", 33, 31, 1, 64), Case("tri", 64, 65, 64, 1), Case("tri", 65, 63, 33, 31), Case("tri", 130, 32, 33, 31),
    # ---- the state path (A = None); both shapes qualify for the one-launch kind of handle (K, L <= 32)
    Case("state", 65, 63, 7), Case("state_tri", 33, 31, 5, 6),
    # ---- VB: K in 1, 33, 63, 64; I and J at 33 and 65
    Case("vb", 33, 65, 1), Case("vb", 65, 33, 33), Case("vb", 33, 33, 63), Case("vb", 65, 65, 64), Case("vb", 65, 33, 64, train="full"),
]
for _n, _c in enumerate(CASES):
    _c.index = _n
FAMILIES = {"plain": ("plain", "state"), "wide": ("wide",), "tri": ("tri", "state_tri"), "vb": ("vb",)}


def by_family(*fams):
    return [c for c in CASES if c.family in fams]


# ------------------------------------------------------------------ data
_shape_cache = {}


def shape_data(I, J, train="seeded"):
    """R (fp32 integers in [-8, 8]) and the training mask (about 70 %, no empty row or column) of a shape"""
    key = (I, J, train)
    if key not in _shape_cache:
        rs = np.random.RandomState(SEED + 1009 * I + J)
        R = rs.randint(-8, 9, size=(I, J)).astype(np.float32)
        M = (rs.random_sample((I, J)) < 0.7).astype(np.uint8)
        if train == "full":
            M[:] = 1
        for i in np.flatnonzero(M.sum(axis=1) == 0):
            M[i, rs.randint(J)] = 1
        for j in np.flatnonzero(M.sum(axis=0) == 0):
            M[rs.randint(I), j] = 1
        R.setflags(write=False); M.setflags(write=False)
        _shape_cache[key] = (R, M)
    return _shape_cache[key]


class Problem:
    """R, M and the factors of one case: A [I][K], B [J][width] (S [K][L] for a tri-factorisation); vb: A, B are the
    expectations and varA, varB the variances."""

    def __init__(self, case):
        c = self.case = case
        self.R, self.M = shape_data(c.I, c.J, c.train)
        rs = np.random.RandomState(SEED + 7919 * c.index)
        hi = 6 if c.family == "vb" else 8
        self.A = rs.randint(0, hi, size=(c.I, c.K)).astype(np.float64)
        self.B = rs.randint(0, hi, size=(c.J, c.width)).astype(np.float64)
        self.S = rs.randint(0, 4, size=(c.K, c.L)).astype(np.float64) if c.L else None
        self.varA = rs.randint(0, 4, size=(c.I, c.K)).astype(np.float64) if c.family == "vb" else None
        self.varB = rs.randint(0, 4, size=(c.J, c.K)).astype(np.float64) if c.family == "vb" else None
        self._masks = {}

    def left(self):
        """the I x width left operand the kernel contracts with B (the host forms A S for a tri-factorisation)"""
        return self.A @ self.S if self.S is not None else self.A

    def second_moments(self):
        """(A2, B2) as the device holds them: S2 = var + exp * exp formed in fp32 (api_models.inc: vb_upload_dir), or None"""
        if self.varA is None:
            return None, None
        f = np.float32
        return ((self.varA.astype(f) + self.A.astype(f) * self.A.astype(f)).astype(np.float64),
                (self.varB.astype(f) + self.B.astype(f) * self.B.astype(f)).astype(np.float64))

    def mask(self, name):
        """the uint8 mask the sums run over (`train`: what Mp = None selects)"""
        if name not in self._masks:
            I, J = self.case.I, self.case.J
            Mp = np.zeros((I, J), np.uint8)
            if name == "train":
                Mp = self.M.copy()
            elif name == "full":
                Mp[:] = 1
            elif name == "corner":
                Mp[I - 1, J - 1] = 1
            elif name == "last_row":
                Mp[I - 1, :] = 1
            elif name == "last_col":
                Mp[:, J - 1] = 1
            elif name == "tile_out":                            # one whole 32 x 32 tile out, in the middle of the grid
                Mp[:] = 1
                ty, tx = ((I + TILE - 1) // TILE) // 2, ((J + TILE - 1) // TILE) // 2
                Mp[TILE * ty:TILE * (ty + 1), TILE * tx:TILE * (tx + 1)] = 0
            elif name == "half":
                Mp = (np.random.RandomState(SEED + 104729 + self.case.index).random_sample((I, J)) < 0.5).astype(np.uint8)
            elif name != "empty":
                raise ValueError(name)
            self._masks[name] = Mp
        return self._masks[name]

    def argument(self, name):
        """what the entry point is handed as M_pred"""
        return None if name == "train" else self.mask(name)


_problems = {}


def problem(case):
    if case.index not in _problems:
        _problems[case.index] = Problem(case)
    return _problems[case.index]


# ------------------------------------------------------------------ the reference: integers, entry by entry
def _ints(x):
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi, x)
    return xi


def product(p):
    """P = A B^T (or F S G^T) in int64"""
    A, B = _ints(p.A), _ints(p.B)
    return (A @ _ints(p.S) @ B.T) if p.S is not None else A @ B.T


def reference(p, name, magnitudes=False):
    """The six sums over the mask (Python ints), then -- vb -- sum (R - P)^2 and the second-moment sum.  magnitudes: the sums
    of the |terms| instead (what any partial sum in any order stays below), and the largest |term| of a single contraction."""
    m = p.mask(name) != 0
    r = _ints(p.R)[m]
    P = product(p)
    q = P[m]
    if magnitudes:
        r = np.abs(r)
    six = [int(m.sum()), int(r.sum()), int((r * r).sum()), int(q.sum()), int((q * q).sum()), int((r * q).sum())]
    if p.varA is None:
        return six + ([int(P.max(initial=0))] if magnitudes else [])
    A, B, vA, vB = _ints(p.A), _ints(p.B), _ints(p.varA), _ints(p.varB)
    S2 = (vA + A * A) @ (vB + B * B).T
    E2 = (A * A) @ (B * B).T
    if magnitudes:
        return six + [int(S2[m].sum()) + int(E2[m].sum()), int(max(P.max(initial=0), S2.max(initial=0)))]
    res = _ints(p.R) - P
    return six + [int((res * res)[m].sum()), int((S2 - E2)[m].sum())]


def as_doubles(v):
    out = np.array([float(x) for x in v])
    assert all(int(o) == x for o, x in zip(out, v))
    return out


# ------------------------------------------------------------------ a NumPy model of metric_kernel + metric_reduce_kernel
FAULTS = ("drop_last_rowgroup", "i_le", "j_le", "drop_partial_chunk", "stale_columns", "stride64_load", "fold_stops_at_256",
          "b_bound_swapped", "second_moment_ignores_mask")
# (not a fault: stride 64 on BOTH the load and the product.  A chunk has at most 64 columns, so no index r * 64 + k reaches the
#  next row: stride 65 spreads the LDS banks and changes no value.  `stride64_both` shows that; the fault that aliases rows is
#  the load and the product disagreeing, `stride64_load`.)


def kernel_model(p, name, fault=None):
    """The seven sums {n, sum R, sum R^2, sum P, sum P^2, sum R P, second-moment sum} as the launch forms them: tile by tile,
    row group by row group, chunk by chunk through flat LDS tiles, then the fold over the tiles -- with one line changed when
    `fault` names it.  Memory past the end of an array reads as ONE (only a faulty bound gets there)."""
    I, J = p.case.I, p.case.J
    A, B = _ints(p.left()), _ints(p.B)
    A2, B2 = p.second_moments()
    K = A.shape[1]
    Rf = np.concatenate([_ints(p.R).ravel(), np.ones(J + 1, np.int64)])
    Mf = np.concatenate([p.mask(name).ravel().astype(np.int64), np.ones(J + 1, np.int64)])
    pad = lambda X: np.vstack([_ints(X), np.ones((TILE, X.shape[1]), np.int64)])
    A, B = pad(A), pad(B)
    if A2 is not None:
        A2, B2 = pad(A2), pad(B2)
    nty, ntx = (I + TILE - 1) // TILE, (J + TILE - 1) // TILE
    load_stride = 64 if fault in ("stride64_load", "stride64_both") else STRIDE
    read_stride = 64 if fault == "stride64_both" else STRIDE
    lane = np.arange(TILE)
    parts = np.zeros((nty * ntx, 7), np.int64)
    for by in range(nty):
        for bx in range(ntx):
            i0, j0 = TILE * by, TILE * bx
            At, Bt = np.zeros(TILE * STRIDE, np.int64), np.zeros(TILE * STRIDE, np.int64)       # (they keep what a pass left)
            ii, jj = i0 + lane, j0 + lane

            def guard(use_mask=True):
                gi = ii <= I if fault == "i_le" else ii < I
                gj = jj <= J if fault == "j_le" else jj < J
                g = gi[:, None] & gj[None, :]
                flat = np.where(g, ii[:, None] * J + jj[None, :], 0)
                return (g & (Mf[flat] != 0)) if use_mask else g, flat

            def load(X, Y, k0, kc):
                k = np.arange(kc)
                at = lane[:, None] * load_stride + k[None, :]
                At[at] = np.where((ii < I)[:, None], X[ii][:, k0:k0 + kc], 0)
                b_bound = I if fault == "b_bound_swapped" else J
                Bt[at] = np.where((jj < b_bound)[:, None], Y[jj][:, k0:k0 + kc], 0)

            def tiles_of(kk):
                at = lane[:, None] * read_stride + np.arange(kk)[None, :]
                return At[at], Bt[at]

            pr, sq = np.zeros((TILE, TILE), np.int64), np.zeros((TILE, TILE), np.int64)
            for k0 in range(0, K, CHUNK):
                kc = min(CHUNK, K - k0)
                if fault == "drop_partial_chunk" and kc < CHUNK:
                    continue
                load(A, B, k0, kc)
                Am, Bm = tiles_of(CHUNK if fault == "stale_columns" and k0 else kc)
                g, _ = guard()
                pr += np.where(g, Am @ Bm.T, 0)
                sq += np.where(g, (Am * Am) @ (Bm * Bm).T, 0)
            g, flat = guard()
            if fault == "drop_last_rowgroup":
                g = g.copy(); g[8 * (ROWGROUPS - 1):] = False
            r = Rf[flat]
            s = [g.sum(), (r * g).sum(), (r * r * g).sum(), (pr * g).sum(), (pr * pr * g).sum(), (r * pr * g).sum(), -(sq * g).sum()]
            if A2 is not None:
                load(A2, B2, 0, K)
                Am, Bm = tiles_of(K)
                g2, _ = guard(use_mask=fault != "second_moment_ignores_mask")
                s[6] += ((Am @ Bm.T) * g2).sum()
            parts[by * ntx + bx] = s
    if fault == "fold_stops_at_256":
        parts = parts[:FOLD]
    return [int(v) for v in parts.sum(axis=0)]


def model_outputs(p, name, fault=None):
    """what a test compares, from the model's seven sums: the six sums; vb: + {sum (R - P)^2, second-moment sum}"""
    s = kernel_model(p, name, fault)
    return s[:6] + ([s[2] - 2 * s[5] + s[4], s[6]] if p.varA is not None else [])


# ------------------------------------------------------------------ the real-valued case
class RealCase:
    """A near-exact fit off the integer grid: R = fp32(U V^T + a residual near 1e-2), values near 90, so that sum R^2 -
    2 sum R P + sum P^2 cancels six digits.  The reference is the residual form, sum (R - P)^2, with math.fsum from the fp32 R
    and the fp64 factors.  The allowed difference is derived: any summation order of N terms errs by at most (N - 1) u sum|term|
    to first order, each P carries at most K fma roundings, so |device - reference| <= 2 (N + 2 K + 2) u (sum R^2 + sum P^2 +
    2 sum |R P|) with u = 2^-53."""
    I, J, K = 97, 103, 8

    def __init__(self):
        rs = np.random.RandomState(SEED + 5)
        I, J, K = self.I, self.J, self.K
        self.U = rs.uniform(3.0, 3.7, size=(I, K))
        self.V = rs.uniform(3.0, 3.7, size=(J, K))
        self.R = (self.U @ self.V.T + rs.normal(0.0, 1.2e-2, size=(I, J))).astype(np.float32)
        self.M = np.ones((I, J), np.uint8)
        self.Mp = (rs.random_sample((I, J)) < 0.9).astype(np.uint8)
        ij = np.argwhere(self.Mp != 0)
        U, V, R = self.U, self.V, self.R.astype(np.float64)
        P = [math.fsum(U[i] * V[j]) for i, j in ij]
        r = [float(R[i, j]) for i, j in ij]
        self.N = len(ij)
        self.sse = math.fsum((a - b) * (a - b) for a, b in zip(r, P))
        mags = math.fsum(a * a for a in r) + math.fsum(b * b for b in P) + 2.0 * math.fsum(abs(a * b) for a, b in zip(r, P))
        self.bound = 2.0 * (self.N + 2 * K + 2) * 2.0 ** -53 * mags


_real = []


def real_case():
    if not _real:
        _real.append(RealCase())
    return _real[0]
