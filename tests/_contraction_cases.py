"""Cases of the exact tests of the masked contraction  P = R~.V / Pv = R~^T.U  (K1 / K2: csrc/kernel_gemm.hip,
gemm_bf16x3_body) and a NumPy emulation of its three-term bf16 operand split (split3).

Every case puts integers on a grid where each partial sum of the contraction -- in any order -- is an integer below 2^24 in
magnitude, so the only correct fp32 result is the exact one.  The conditional hook (bnmf_cond_params / bnmtf_cond_params: the
real K1 / K2 launch, then the generic sweep for one column) reads the contraction back as

    numer = fmaf(tau, P_ik + corr_ik, -lambda)       tau = 1, lambda = 0.5

with corr = 0 when the unit's own factor is zero (families A, B, C, E) and the Gram / missing-entry correction of the sweep
otherwise (family D).

Families (a = the factor operand, the MFMA's A; b = R~, its B; h / m / l = the hi / mid / lo bf16 terms of the split):
  A  dense, R below 2^24 / m, factor in {0, 1}: b's hi and mid terms over whole inner extents (and the mask: R at masked-out
     entries holds LEAK, so a leak shows as a wrong integer);
  B  R of 18 significant bits (b's lo term), factor 0/1 with disjoint column supports of at most 30 rows, rotated over states
     so that every inner row is probed;
  C  R in {1, 2, 4}, factor of 18 bits on supports of at most 8 rows (a's mid and lo terms), and C2: both 10-bit on
     supports of at most 16 rows (the only family with a nonzero a_m.b_m).
     (18 bits, not 17: the residuals are signed, so each bf16 term carries 9 bits of an integer and 17 bits split into hi + mid
     exactly -- the lo term of a 17-bit integer is always zero);
  D  the whole conditional: nonzero small-integer U and V (q, corr and the Gram C of the sweep);
  E  the tri-factorisation's F / G steps: F = 0 (or G = 0) and S a scaled partial permutation, so that the effective factor
     G.S^T / F.S of small_product_kernel is exact.
"""
import numpy as np

TWO24 = float(1 << 24)
LAM = 0.5
LEAK = 3.0 * 2 ** 20          # R at masked-out entries

# the kernel's six retained products (a = factor, b = R~), in its order; and the three it drops
PRODUCTS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
DROPPED = (("m", "l"), ("l", "m"), ("l", "l"))


def _ru(x, q):
    return -(-x // q) * q


def launch(n, m, W):
    """The launch parameters build_dir (csrc/api.hip) picks for one direction: n units, m inner rows, W factor columns."""
    KP = 32 if W <= 32 else 64
    n_pad = _ru(max(n, 1), 128)
    tw = 2 if KP == 64 and n_pad <= 2048 else 4
    split = min(max(1, 256 // (n_pad // (32 * tw))), max(1, m // 256))
    ipw = _ru(-(-m // (split * 4)), 32)
    return dict(KP=KP, tw=tw, n_pad=n_pad, split=split, ipw=ipw, nsteps=ipw // 16)


def instantiation(p):
    """gemm_bf16x3_kernel<MT, NSET, TW> of a launch: (MT, TW)"""
    return (p["KP"] // 32, p["tw"])


class Case:
    def __init__(self, I, J, K, mask, fams, rows, cols, L=0):
        self.I, self.J, self.K, self.L, self.mask, self.fams = I, J, K, L, mask, fams
        self.expect = {"rows": rows, "cols": cols}        # (KP, tw, n_pad, split, ipw, nsteps) or None: direction not checked

    @property
    def id(self):
        return "%dx%dx%d%s-%s-%s" % (self.I, self.J, self.K, "x%d" % self.L if self.L else "", self.mask, "".join(self.fams))

    def dirs(self):
        return [d for d in ("rows", "cols") if self.expect[d] is not None]

    def launch(self, d):
        W = self.K if d == "rows" else (self.L or self.K)
        return launch(self.I, self.J, W) if d == "rows" else launch(self.J, self.I, W)


_F = ("KP", "tw", "n_pad", "split", "ipw", "nsteps")

# (I, J, K), mask, families, then the launch each direction must get: (KP, tw, n_pad, split, ipw, nsteps)
CASES = [
    Case(1, 200, 5, "dense", "AB", (32, 4, 128, 1, 64, 4), (32, 4, 256, 1, 32, 2)),              # one unit; fewest steps
    Case(127, 255, 32, "single", "ABCD", (32, 4, 128, 1, 64, 4), (32, 4, 256, 1, 32, 2)),         # K = KP = 32
    Case(129, 257, 33, "sparse", "ABC", (64, 2, 256, 1, 96, 6), (64, 2, 384, 1, 64, 4)),          # K = 33: pad columns
    Case(130, 385, 64, "edge", "AB", (64, 2, 256, 1, 128, 8), None),                              # tw = 2, nsteps mod 3 = 2
    Case(2048, 1000, 64, "dense", "AB", (64, 2, 2048, 3, 96, 6), (64, 2, 1024, 8, 64, 4)),        # tw = 2 at n_pad = 2048
    Case(2049, 700, 64, "sparse", "ABC", (64, 4, 2176, 2, 96, 6), (64, 2, 768, 8, 96, 6)),        # tw = 4 just past the switch
    Case(2100, 7711, 64, "edge", "AB", (64, 4, 2176, 15, 160, 10), None),                         # tw = 4, nsteps mod 3 = 1
    Case(2047, 5000, 40, "single", "ABD", (64, 2, 2048, 8, 160, 10), (64, 4, 5120, 6, 96, 6)),    # mixed
    Case(300, 12000, 20, "sparse", "ABD", (32, 4, 384, 46, 96, 6), (32, 4, 12032, 1, 96, 6)),     # whole inner slices in the pad
    Case(4096, 4096, 32, "dense", "AB", (32, 4, 4096, 8, 128, 8), (32, 4, 4096, 8, 128, 8)),      # cfg2 shape, no pad
    Case(8192, 8192, 64, "edge", "AB", (64, 4, 8192, 4, 512, 32), (64, 4, 8192, 4, 512, 32)),     # headline shape
    # tri-factorisations (family E): the F step (rows, W = K) and the G step (cols, W = L)
    Case(2049, 700, 40, "sparse", "E", (64, 4, 2176, 2, 96, 6), (32, 4, 768, 8, 96, 6), L=20),
    Case(129, 257, 33, "edge", "E", (64, 2, 256, 1, 96, 6), (32, 4, 384, 1, 64, 4), L=7),
]
for _c in CASES:
    for _d in ("rows", "cols"):
        if _c.expect[_d] is not None:
            _c.expect[_d] = dict(zip(_F, _c.expect[_d]))
HEAVY = 1 << 24          # I * J above this: the CPU pins leave the per-product analysis to the smaller cases


# ------------------------------------------------------------------ split3 emulation
def _rne_bf16(x):
    """fp32 -> the fp32 value of its round-to-nearest-even bf16 (v_cvt_pk_bf16_f32 on finite values)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).astype(np.uint32)
    return r.view(np.float32)


def split3(x):
    """x (fp32) = h + m + l as the kernel splits it (each residual exact in fp32)"""
    x = np.asarray(x, dtype=np.float32)
    h = _rne_bf16(x)
    b = x - h
    m = _rne_bf16(b)
    l = _rne_bf16(b - m)
    return {"h": h, "m": m, "l": l}


# ------------------------------------------------------------------ data
def _mask(kind, I, J, rs):
    if kind == "dense":
        M = np.ones((I, J), dtype=np.uint8)
    elif kind == "sparse":                                 # about 90 % missing
        M = (rs.random_sample((I, J)) < 0.1).astype(np.uint8)
    elif kind == "single":                                 # rows and columns with exactly one observed entry
        M = (rs.random_sample((I, J)) < 0.6).astype(np.uint8)
        for i in range(0, I, 3):
            M[i] = 0
            M[i, rs.randint(J)] = 1
        for j in range(1, J, 5):
            M[:, j] = 0
            M[rs.randint(I), j] = 1
    elif kind == "edge":                                   # observed entries in the last inner rows before the pad
        M = (rs.random_sample((I, J)) < 0.8).astype(np.uint8)
        M[:, -1] = 1; M[-1, :] = 1
    else:
        raise ValueError(kind)
    for i in np.flatnonzero(M.sum(axis=1) == 0):           # (no fully unobserved row or column: the models refuse them)
        M[i, rs.randint(J)] = 1
    for j in np.flatnonzero(M.sum(axis=0) == 0):
        M[rs.randint(I), j] = 1
    return M


def _ints(rs, shape, lo, hi, dtype=np.float32):
    """uniform integers in [lo, hi]"""
    return rs.randint(lo, hi + 1, size=shape).astype(dtype)


def _supports(m, W, rows, rs):
    """Disjoint column supports of at most `rows` inner rows, rotated over states so that every inner row is in one:
    list over states of an (m,) array: the column whose support holds the row, or -1."""
    per = W * rows
    nst = -(-m // per)
    perm = rs.permutation(m)                               # (scattered: every step and slice of the inner extent is hit)
    out = []
    for s in range(nst):
        col = np.full(m, -1, dtype=np.int64)
        mine = perm[s * per:(s + 1) * per]
        col[mine] = np.arange(len(mine)) % W
        out.append(col)
    return out


class Problem:
    """One model: R, M (I x J) and its states.  A state is (direction, U, V) -- for a tri-factorisation (direction, F, S, G)."""

    def __init__(self, fam, R, M, states):
        self.fam, self.R, self.M, self.states = fam, R, M, states


def problems(case):
    seed = (case.I * 7919 + case.J * 104729 + case.K * 31 + case.L) % (2 ** 31)
    for fam in case.fams:
        for p in _family(case, fam, np.random.RandomState([seed, ord(fam)])):
            yield p


def _family(case, fam, rs):
    I, J, K, L = case.I, case.J, case.K, case.L
    M = _mask(case.mask, I, J, rs)
    dims = {"rows": (J, I), "cols": (I, J)}                # direction -> (inner extent m, units n)

    def with_leak(R):
        return np.where(M == 1, R, np.float32(LEAK)).astype(np.float32)

    def states_01(dense_or_supports):
        st = []
        for d in case.dirs():
            m, n = dims[d]
            zeros = np.zeros((n, K), dtype=np.float32)
            for X in dense_or_supports(m):
                st.append((d, zeros, X) if d == "rows" else (d, X, zeros))
        return st

    def on_supports(rows, values):
        def gen(m):
            out = []
            for col in _supports(m, K, rows, rs):
                X = np.zeros((m, K), dtype=np.float32)
                hit = np.flatnonzero(col >= 0)
                X[hit, col[hit]] = values(len(hit))
                out.append(X)
            return out
        return gen

    if fam == "A":
        rmax = int(TWO24 / max(I, J) / 1.01) - 1
        R = with_leak(_ints(rs, (I, J), 0, min(rmax, (1 << 17) - 1)))
        yield Problem("A", R, M, states_01(lambda m: [_ints(rs, (m, K), 0, 1)]))
    elif fam == "B":
        R = with_leak(_ints(rs, (I, J), 1 << 17, (1 << 18) - 1))
        yield Problem("B", R, M, states_01(on_supports(30, lambda c: 1.0)))
    elif fam == "C":
        R = with_leak((2.0 ** _ints(rs, (I, J), 0, 2)).astype(np.float32))
        yield Problem("C", R, M, states_01(on_supports(8, lambda c: _ints(rs, c, 1 << 17, (1 << 18) - 1))))
        R = with_leak(_ints(rs, (I, J), 512, 1000))
        yield Problem("C2", R, M, states_01(on_supports(16, lambda c: _ints(rs, c, 512, 1000))))
    elif fam == "D":
        R = with_leak(_ints(rs, (I, J), 0, 255))
        st = []
        for d in case.dirs():
            U = _ints(rs, (I, K), 0, 2); V = _ints(rs, (J, K), 0, 2)
            st.append((d, U, V))
        yield Problem("D", R, M, st)
    elif fam == "E":
        R = with_leak(_ints(rs, (I, J), 0, 511))
        S = np.zeros((K, L), dtype=np.float32)             # a scaled partial permutation: at most one power of two per row and column
        ks = rs.permutation(K)[:min(K, L) - 1]; ls = rs.permutation(L)[:min(K, L) - 1]
        S[ks, ls] = 2.0 ** _ints(rs, len(ks), 0, 2)
        st = []
        if "rows" in case.dirs():
            st.append(("rows", np.zeros((I, K), np.float32), S, _ints(rs, (J, L), 0, 3)))
        if "cols" in case.dirs():
            st.append(("cols", _ints(rs, (I, K), 0, 3), S, np.zeros((J, L), np.float32)))
        yield Problem("E", R, M, st)
    else:
        raise ValueError(fam)


# ------------------------------------------------------------------ what the contraction sees, and the exact answer
class View:
    """One direction of a problem as the contraction sees it: R~ (n x m, zero at masked-out entries) and the mask in fp64, and
    R~'s split -- computed once for all the states of the direction."""

    def __init__(self, Rd, Md):
        self.Mf = Md.astype(np.float64)
        Rt = np.where(Md == 1, Rd, 0).astype(np.float32)
        self.split = split3(Rt)
        self.abs_split = _abs_split(self.split)
        self.Rt = Rt.astype(np.float64)


def view(p, d):
    if not hasattr(p, "_views"):
        p._views = {}
    if d not in p._views:
        p._views[d] = View(p.R, p.M) if d == "rows" else View(p.R.T, p.M.T)
    return p._views[d]


def operands(p, state):
    """(the direction's View, X: the factor operand m x W, Y: the units' own factor n x W)"""
    d = state[0]
    if len(state) == 4:                                    # tri-factorisation: X = G S^T (F step) or F S (G step)
        _, F, S, G = state
        if d == "rows":
            return view(p, d), (G.astype(np.float64) @ S.T.astype(np.float64)).astype(np.float32), F
        return view(p, d), (F.astype(np.float64) @ S.astype(np.float64)).astype(np.float32), G
    _, U, V = state
    return (view(p, d), V, U) if d == "rows" else (view(p, d), U, V)


def exact(v, X, Y):
    """fp64 (exact on these grids) conditional of every unit and column:
         num_ik = sum_j M_ij (R_ij - sum_{l != k} Y_il X_jl) X_jk ,  tau_ik = sum_j M_ij X_jk^2
    -> (numer as the fp32 fmaf(1, num, -0.5), num, tau, sum of |terms| per output, tau exact?)"""
    Mf = v.Mf
    X = X.astype(np.float64); Y = Y.astype(np.float64)
    X2 = Mf @ (X * X)
    num = v.Rt @ X + Y * X2
    budget = v.abs_split @ _abs_split(split3(X))
    if np.any(Y):
        num -= (Mf * (Y @ X.T)) @ X
        aY, aX = np.abs(Y), np.abs(X)
        miss = 1.0 - Mf
        budget = budget + aY @ (aX.T @ aX) + (miss * (aY @ aX.T)) @ aX + aY * (miss @ (aX * aX))
    numer = (num - LAM).astype(np.float32)
    tau_ok = bool((X * X).sum(axis=0).max(initial=0.0) < TWO24)
    return numer, num, X2, budget, tau_ok


def _abs_split(s):
    return np.abs(s["h"].astype(np.float64)) + np.abs(s["m"]) + np.abs(s["l"])
