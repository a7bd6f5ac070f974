"""Cases of the exact tests of the tri-factorisation's S system (csrc/kernel_ssys.hip) and a NumPy model of it.

For K, L <= 32 the S step solves one dense K.L x K.L system (a = (k, l) = k L + l):

    A[a][a'] = sum_j W_j[k][k'] Gc_j[l][l'] ,   W_j = C~f - sum_{i in miss(j)} F_i F_i^T ,   Gc_j = G_j G_j^T
    b[a]     = sum_j Pv_jk G_jl ,               Pv = R~^T F
    r        = b - A S ,                        numer_a = fmaf(tau, r_a + S_a A_aa, -lambdaS) ,  tauS_a = tau A_aa

built by six launches: the contraction Pv (already exact-tested: _contraction_cases.py), scol_gram_kernel<VB, 1> (W_j on the
bf16 matrix cores with a three-term split, walking the 64-wide missing-entry slots; gamma_pack and ssys_b ride in the same
launch), ssys_gemm_bf16_kernel (one packed K(K+1)/2 x J x L(L+1)/2 product over nsplit column ranges, its own copy of the
split), ssys_reduce_kernel (the slabs in two halves, the mirror write for k != k'), ssys_b (one partial per 64 columns) and
ssys_residual_kernel.  The hook bnmtf_cond_params(which = 1) returns (numer_a, tauS_a) (kernel_ssys.hip, ssys_chain_kernel's
cond >= 0 branch); with BNMTF_SSYS=0 the per-row path (kernel_bnmtf.hip: srow_*) answers the same hook.

Every case puts F, S, G, R on integer grids with tau = 1, lambdaS = 0.5.  An output is CHECKED when every intermediate that
feeds it is an integer whose sum of |terms| -- in any order -- is below 2^24 (System.budget, System.ok), so that its only
correct fp32 value is the exact one; and the three split products the kernels drop (m.l, l.m, l.l) are zero on it.

Families (a state is one (F, S, G); h / m / l = the hi / mid / lo bf16 terms of split3):
  X   indexing: F, G 0/1 with one (sometimes two) ones per row, S distinct nonzero integers -- a wrong A[a][a'] for any a'
      moves numer_a.  Packing, the tri_pos interleave, the mirror write, ranges, slabs, b blocks and the missing lists.
  W   scol_gram's lo terms: a few missing rows of F carry an 18-bit value in column k0 and powers of two elsewhere (F = 0 on
      the other rows), G 0/1 on the columns those rows are missing in (0 elsewhere).  Entries k != k0 are checked: W_j[k][k0]
      has h.h, h.m, h.l (k < k0) and l.h, m.h (k > k0) terms; in ssys_gemm it is an 18-bit operand (its l.h, m.h).
  W2  scol_gram's m.m: missing rows with 10-bit values in two columns.
  G   ssys_gemm's lo terms of Gc: the same construction on G (an 18-bit value in column l0 of a few rows of G), F 0/1 sparse.
  GM  ssys_gemm's m.m: a 10-bit F value (column k0) against a 10-bit G value (column l0).
  XV  (VB only) X's F and G with integer variances varF, varG and S in 1..3: the diagonal terms of the second moments.
(18 bits, not 17: the residuals are signed, so a 17-bit integer splits exactly into hi + mid.)
"""
import numpy as np

from _contraction_cases import DROPPED, LAM, PRODUCTS, TWO24, _abs_split, _ru, split3

# ------------------------------------------------------------------ the host's launch (csrc/api_models.inc, kernels.h)
def tri_count(K):
    return K * (K + 1) // 2


def tri_padded(K):
    return _ru(tri_count(K), 64)


def tri_index(k, kp, K):
    return k * K - k * (k - 1) // 2 + (kp - k)


def tri_pos(p):
    return (p & ~63) + 2 * (p & 31) + ((p >> 5) & 1)


def ssys_gemm_wave_tiles(K, L):
    return (tri_padded(K) // 64) * (tri_padded(L) // 64)


def ssys_gemm_range(n, nsplit):
    return ((n + nsplit - 1) // nsplit + 15) & ~15


def ssys_b_blocks(n):
    return max((n + 63) // 64, 1)


def ssys_launch(K, L, J):
    """What bnmtf_alloc_extras / enqueue_ssys_build pick for a K x L system over J columns (one GPU)."""
    wt = ssys_gemm_wave_tiles(K, L)
    by_tiles = 512 // max((wt + 3) // 4, 1)
    nsplit = max(1, min(by_tiles, max(J // 64, 1), 32))
    per = ssys_gemm_range(J, nsplit)
    ranges = [(s * per, min(J, (s + 1) * per)) for s in range(nsplit)]
    nonempty = [r for r in ranges if r[0] < r[1]]
    return dict(on=int(K <= 32 and L <= 32), tri_padded=(tri_padded(K), tri_padded(L)), wave_tiles=wt, nsplit=nsplit,
                limit="tiles" if nsplit == by_tiles < min(max(J // 64, 1), 32) else ("cap" if nsplit == 32 else
                                                                                    ("J/64" if nsplit > 1 else "one")),
                range=per, ranges=ranges, empty=len(ranges) - len(nonempty), last=nonempty[-1][1] - nonempty[-1][0],
                bblocks=ssys_b_blocks(J))


def slots(nmiss):
    """64-wide missing-entry slots of a column (missing_lists_kernel: the missing rows in order, padded with the zero row)"""
    return _ru(nmiss, 64)


# ------------------------------------------------------------------ cases
MISS_CLASSES = (0, 1, 63, 64, 65, 128, "I-1")       # missing entries per column ("I-1": one observed entry)


class Case:
    def __init__(self, I, J, K, L, fams, expect, classes=MISS_CLASSES, vb=False):
        self.I, self.J, self.K, self.L, self.fams, self.vb = I, J, K, L, fams, vb
        self.classes = [c for c in classes if (I - 1 if c == "I-1" else c) < I]
        self.expect = expect            # (tri_padded K, tri_padded L, nsplit, range, empty ranges, bblocks) or None (per-row only)

    @property
    def id(self):
        return "%dx%dx%dx%d-%s" % (self.I, self.J, self.K, self.L, "".join(self.fams))

    @property
    def dense(self):
        return self.K <= 32 and self.L <= 32

    def launch(self):
        return ssys_launch(self.K, self.L, self.J)


_X = ("X",)
_ALL = ("X", "W", "W2", "G", "GM")
# I x J, K x L, families, then the launch the dense system must get: (tri_padded K, tri_padded L, nsplit, range, empty, bblocks)
CASES = [
    Case(130, 1, 1, 1, _X, (64, 64, 1, 16, 0, 1)),                        # everything of size one
    Case(140, 17, 10, 11, _ALL, (64, 128, 1, 32, 0, 1), vb=True),          # J < 64: one range, J mod 16 = 1
    Case(150, 2047, 11, 3, _ALL, (128, 64, 31, 80, 5, 32)),               # five empty trailing ranges, J mod 16 = 15
    Case(135, 2049, 16, 20, _ALL, (192, 256, 32, 80, 6, 33), vb=True),     # nsplit capped at 32, six empty ranges, last b block of 1 column
    Case(160, 700, 23, 25, _ALL, (320, 384, 10, 80, 1, 11)),
    Case(131, 3000, 28, 30, _ALL, (448, 512, 32, 96, 0, 47)),
    Case(200, 4096, 32, 32, _ALL, (576, 576, 24, 176, 0, 64), vb=True),    # nsplit limited by wave tiles, short last range (48)
    Case(140, 9000, 32, 1, ("X", "W", "W2"), (576, 64, 32, 288, 0, 141)),
    Case(133, 65, 3, 32, _ALL, (64, 576, 1, 80, 0, 2)),                   # one range longer than J, J mod 64 = 1
    Case(129, 15, 5, 2, ("X", "W", "G"), (64, 64, 1, 16, 0, 1)),            # J < 16
    Case(137, 2063, 32, 31, ("X", "W", "GM"), (576, 512, 28, 80, 2, 33)),  # 72 wave tiles: nsplit 28 by tiles, J mod 16 = 15
    Case(141, 1000, 22, 24, ("X", "G", "W2"), (256, 320, 15, 80, 2, 16)),
    Case(139, 513, 27, 16, ("X", "W"), (384, 192, 8, 80, 1, 9)),          # J mod 64 = 1
    Case(136, 1100, 30, 28, ("X", "GM"), (512, 448, 17, 80, 3, 18)),
    # K or L in 33..64: always the per-row path
    Case(140, 300, 40, 6, ("X", "W"), None),
    Case(133, 129, 4, 64, ("X", "G"), None),
    Case(150, 1000, 33, 33, ("X",), None),
]
_FE = ("tri_padded", "nsplit", "range", "empty", "bblocks")
for _c in CASES:
    if _c.expect is not None:
        _c.expect = dict(zip(_FE, ((_c.expect[0], _c.expect[1]),) + _c.expect[2:]))


def describe_fields(launch):
    """the `ssys[...]` field describe() reports for a launch"""
    if not launch["on"]:
        return dict(on=0)
    return dict(on=1, nsplit=launch["nsplit"], range=launch["range"], bblocks=launch["bblocks"])


# ------------------------------------------------------------------ data
def _mask(case, rs):
    """~10 % missing, and the missing-count classes on columns spread over J (the last column among them); the single missing
    entry of class 1 sits at row I - 1, class 63 starts at row 0.  No fully unobserved row or column (_base.py refuses them)."""
    I, J = case.I, case.J
    M = (rs.random_sample((I, J)) >= 0.1).astype(np.uint8)
    cols = {}
    if J > 1:
        where = np.unique(np.linspace(J - 1, 0, len(case.classes)).round().astype(int))
        for c, j in zip(case.classes, where):
            n = I - 1 if c == "I-1" else c
            M[:, j] = 1
            if c == 1:
                rows = np.array([I - 1])
            elif c == 63:
                rows = np.concatenate([[0], 1 + rs.permutation(I - 1)[:62]])
            else:
                rows = rs.permutation(I)[:n]
            M[rows, j] = 0
            cols[c] = int(j)
    else:
        M[:] = 1                                            # (one column: every row needs its one observed entry there)
    for i in np.flatnonzero(M.sum(axis=1) == 0):
        free = [j for j in range(J) if j not in cols.values()] or [0]
        M[i, free[rs.randint(len(free))]] = 1
    for j in np.flatnonzero(M.sum(axis=0) == 0):
        M[rs.randint(I), j] = 1
    return M, cols


def _onehot(rs, n, W, two=0.2):
    X = np.zeros((n, W), np.float32)
    X[np.arange(n), rs.randint(W, size=n)] = 1
    if W > 1:
        extra = np.flatnonzero(rs.random_sample(n) < two)
        X[extra, rs.randint(W, size=len(extra))] = 1
    return X


def _odd_bits(rs, n, bits):
    """integers of exactly `bits` significant bits whose split has a nonzero last term (lo for 18, mid for 10)"""
    v = rs.randint(1 << (bits - 1), 1 << bits, size=n) | 1
    s = split3(v.astype(np.float32))
    last = "l" if bits >= 18 else "m"
    bad = s[last] == 0
    while bad.any():
        v[bad] = rs.randint(1 << (bits - 1), 1 << bits, size=int(bad.sum())) | 1
        s = split3(v.astype(np.float32)); bad = s[last] == 0
    return v.astype(np.float32)


class State:
    def __init__(self, fam, F, S, G, varF=None, varG=None):
        self.fam, self.F, self.S, self.G, self.varF, self.varG = fam, F, S, G, varF, varG


class Problem:
    """One model: R, M (I x J), the class columns, and its states."""

    def __init__(self, case, R, M, cols, states):
        self.case, self.R, self.M, self.cols, self.states = case, R, M, cols, states


def problem(case):
    rs = np.random.RandomState((case.I * 7919 + case.J * 104729 + case.K * 31 + case.L) % (2 ** 31))
    M, cols = _mask(case, rs)
    R = rs.randint(1, 8, size=(case.I, case.J)).astype(np.float32)
    return Problem(case, R, M, cols, [st for fam in case.fams for st in _family(case, fam, M, cols, rs)])


def _special(M, cols, rs, nrows):
    """a few (row, column) missing entries to carry the large values: in the class columns, rows 0 and I - 1 first"""
    I, J = M.shape
    js = [j for c, j in sorted(cols.items(), key=lambda t: str(t[0])) if c != 0][:2] or list(range(J))[:2]
    out = []
    for j in js:
        miss = np.flatnonzero(M[:, j] == 0)
        if len(miss):
            pick = [i for i in (0, I - 1) if i in miss][:1] + list(rs.permutation(miss)[:nrows])
            out += [(int(i), int(j)) for i in pick]
    if not out:                                             # (no missing entry at all: the rows are still checked as observed)
        out = [(int(i), 0) for i in rs.permutation(I)[:nrows]]
    seen, uniq = set(), []
    for i, j in out:
        if i not in seen:
            seen.add(i); uniq.append((i, j))
    return uniq[:nrows]


def _family(case, fam, M, cols, rs):
    I, J, K, L = case.I, case.J, case.K, case.L
    if fam == "X":
        F = _onehot(rs, I, K)
        G = _onehot(rs, J, L)
        S = (rs.permutation(K * L) + 1).reshape(K, L).astype(np.float32)
        yield State("X", F, S, G)
        if case.vb:                                         # XV: the same F, G with integer variances, S of 1..3 (the VB states)
            varF = np.where(rs.random_sample((I, K)) < 0.3, rs.randint(1, 3, (I, K)), 0).astype(np.float32)
            varG = np.where(rs.random_sample((J, L)) < 0.3, rs.randint(1, 3, (J, L)), 0).astype(np.float32)
            yield State("XV", F, rs.randint(1, 4, size=(K, L)).astype(np.float32), G, varF, varG)
        return
    S = rs.randint(1, 4, size=(K, L)).astype(np.float32)
    if fam in ("W", "W2"):
        if K < 2 and fam == "W2":
            return
        sp = _special(M, cols, rs, 4 if fam == "W" else 3)
        F = np.zeros((I, K), np.float32)
        G = np.zeros((J, L), np.float32)
        k0 = K // 2
        for i, j in sp:
            if fam == "W":
                F[i] = 2.0 ** rs.randint(0, 2, size=K)
                F[i, k0] = _odd_bits(rs, 1, 18)[0]
            else:
                ks = rs.permutation(K)[:2]
                F[i, ks] = _odd_bits(rs, 2, 10)
            G[j] = _onehot(rs, 1, L)[0]
        yield State(fam, F, S, G)
    elif fam in ("G", "GM"):
        sp = _special(M, cols, rs, 3 if fam == "G" else 1)
        F = np.zeros((I, K), np.float32)
        for i, _ in sp:
            F[i] = _onehot(rs, 1, K)[0]
        js = sorted({j for _, j in sp} | set(rs.permutation(J)[:2 if fam == "G" else 1].tolist()))
        G = np.zeros((J, L), np.float32)
        l0 = L // 2
        for j in js:
            if fam == "G":
                G[j] = 2.0 ** rs.randint(0, 2, size=L)
                G[j, l0] = _odd_bits(rs, 1, 18)[0]
            else:
                G[j] = 1.0
                G[j, l0] = _odd_bits(rs, 1, 10)[0]
        if fam == "GM":
            k0 = K // 2
            for i, _ in sp:
                F[i] = 1.0
                F[i, k0] = _odd_bits(rs, 1, 10)[0]
        # (a few more observed rows of F so that W_j is not only the special rows)
        extra = rs.permutation(I)[:3]
        F[extra] = np.maximum(F[extra], _onehot(rs, len(extra), K, 0.0))
        yield State(fam, F, S, G)
    else:
        raise ValueError(fam)


# ------------------------------------------------------------------ the model: exact values and budgets
def _pairs(K):
    """(k, k') of every packed index p (k <= k'), and p of every full (k, k')"""
    kk = np.array([(k, kp) for k in range(K) for kp in range(k, K)], dtype=np.int64).reshape(-1, 2)
    full = np.zeros((K, K), np.int64)
    for p, (k, kp) in enumerate(kk):
        full[k, kp] = full[kp, k] = p
    return kk, full


def _split_abs(x):
    return _abs_split(split3(x))


def _prod_cols(X, kk, which):
    """[n][p]: for each packed pair (k, k') the product of split term which[0] of X[:, k] with which[1] of X[:, k']"""
    s = split3(X)
    return s[which[0]][:, kk[:, 0]].astype(np.float64) * s[which[1]][:, kk[:, 1]]


class System:
    """Everything the device forms for one (problem, state), in fp64 (exact on these grids), with the budgets."""

    def __init__(self, p, st, vb=False):
        c = p.case
        K, L, J = c.K, c.L, c.J
        self.K, self.L, self.n2 = K, L, K * L
        F, G, S = st.F.astype(np.float64), st.G.astype(np.float64), st.S.astype(np.float64)
        varF = st.varF.astype(np.float64) if vb else np.zeros_like(F)
        varG = st.varG.astype(np.float64) if vb else np.zeros_like(G)
        self.S = S
        Mf = p.M.astype(np.float64)
        miss = 1.0 - Mf
        self.miss = miss
        self.kk, self.kfull = _pairs(K)
        self.ll, self.lfull = _pairs(L)
        kk, ll = self.kk, self.ll
        dk = (kk[:, 0] == kk[:, 1]).astype(np.float64)
        dl = (ll[:, 0] == ll[:, 1]).astype(np.float64)
        # C~f (fp64 Gram, cast to fp32) and W_j = C~f - sum_miss (F_i F_i^T + diag varF_i), packed [J][PK]
        FF = F[:, kk[:, 0]] * F[:, kk[:, 1]] + varF[:, kk[:, 0]] * dk
        self.FF = FF
        self.Cf = FF.sum(axis=0)
        self.Wmiss = miss.T @ FF
        self.W = self.Cf[None, :] - self.Wmiss
        # scol_gram's split products over the missing rows: all six (budget), and the three it drops
        self.gram_prod = {pr: _prod_cols(st.F, kk, pr) for pr in PRODUCTS + DROPPED}
        absF = _split_abs(st.F)
        gram_abs = absF[:, kk[:, 0]] * absF[:, kk[:, 1]] + np.abs(varF[:, kk[:, 0]]) * dk
        gram_budget = miss.T @ gram_abs
        gram_drop = miss.T @ sum(np.abs(self.gram_prod[pr]) for pr in DROPPED)
        # Gc_j = G_j G_j^T + diag varG_j (one fmaf)
        self.Gc = G[:, ll[:, 0]] * G[:, ll[:, 1]] + varG[:, ll[:, 0]] * dl
        # ssys_gemm: Ap = W^T Gc over the columns, split products of its operands
        W32, Gc32 = self.W.astype(np.float32), self.Gc.astype(np.float32)
        self.sW, self.sG = split3(W32), split3(Gc32)
        self.Ap = self.W.T @ self.Gc
        gemm_budget = _split_abs(W32).T @ _split_abs(Gc32)
        gemm_drop = sum(np.abs(self.sW[a].astype(np.float64)).T @ np.abs(self.sG[b].astype(np.float64)) for a, b in DROPPED)
        # b: Pv = R~^T F (the contraction), then sum_j Pv_jk G_jl
        Rt = np.where(p.M == 1, p.R, 0).astype(np.float32)
        self.Pv = Rt.T.astype(np.float64) @ F
        pv_budget = _split_abs(Rt).T @ _split_abs(st.F)
        self.PvG = self.Pv[:, :, None] * G[:, None, :]                     # [J][K][L]
        self.b = self.PvG.sum(axis=0).reshape(-1)
        b_budget = (np.abs(self.Pv).T @ np.abs(G)).reshape(-1)
        # the full system
        self.A = self.unpack(self.Ap)
        s = S.reshape(-1)
        self.num = self.b - self.A @ s + np.diag(self.A) * s
        self.tau = np.diag(self.A).copy()
        r_budget = np.abs(self.b) + np.abs(self.A) @ np.abs(s)
        # which entries are exact: everything on row k of W, row l of Gc, row a of A, b_a and r_a within 2^24, nothing dropped
        kok = np.ones(K, bool); lok = np.ones(L, bool)
        for q, (k, kp) in enumerate(kk):
            bad = (abs(self.Cf[q]) >= TWO24 or gram_budget[:, q].max(initial=0) >= TWO24 or np.abs(self.W[:, q]).max(initial=0) >= TWO24
                   or gram_drop[:, q].max(initial=0) > 0)
            if bad:
                kok[k] = kok[kp] = False
        for q, (l, lp) in enumerate(ll):
            if np.abs(self.Gc[:, q]).max(initial=0) >= TWO24:
                lok[l] = lok[lp] = False
        Abud, Adrop = self.unpack(gemm_budget), self.unpack(gemm_drop)
        a_k, a_l = np.divmod(np.arange(self.n2), L)
        pv_ok = pv_budget.max(axis=0, initial=0) < TWO24
        self.ok = (kok[a_k] & lok[a_l] & (Abud.max(axis=1) < TWO24) & (Adrop.max(axis=1) == 0) & pv_ok[a_k]
                   & (b_budget < TWO24) & (r_budget < TWO24))
        self.numer = (self.num - LAM).astype(np.float32)
        self.budget = dict(cf=np.abs(self.Cf), gram=gram_budget, W=np.abs(self.W), Gc=np.abs(self.Gc), gemm=gemm_budget,
                           pv=pv_budget, b=b_budget, r=r_budget)
        self._G, self._F, self._varF, self._varG = G, F, varF, varG

    def unpack(self, Ap):
        """packed [PK][PL] -> the full n2 x n2 system (ssys_reduce_kernel's writes, both of them)"""
        K, L = self.K, self.L
        rows = self.kfull[:, None, :, None]
        cols = self.lfull[None, :, None, :]
        return Ap[rows, cols].reshape(K * L, K * L)

    # -------- outputs under a change
    def moved(self, dnum=None, dtau=None):
        """does a change of the exact num (and tau) by these amounts change a checked fp32 output?"""
        got = False
        if dnum is not None:
            got |= bool(np.any(((self.num + dnum - LAM).astype(np.float32) != self.numer)[self.ok]))
        if dtau is not None:
            got |= bool(np.any((dtau != 0)[self.ok]))
        return got

    def moved_by_A(self, dA, db=None):
        s = self.S.reshape(-1)
        dnum = -(dA @ s) + np.diag(dA) * s
        if db is not None:
            dnum = dnum + db
        return self.moved(dnum, np.diag(dA))

    def moved_by_Ap(self, dAp):
        return self.moved_by_A(self.unpack(dAp))

    def moved_by_W(self, dW):
        """dW: [J][PK] change of the packed column Grams"""
        return self.moved_by_Ap(dW.T @ self.Gc)


# ------------------------------------------------------------------ the per-row path's intermediates (kernel_bnmtf.hip:7-15)
def row_path_ok(p, st, sysm):
    """Entries of the per-row path (BNMTF_SSYS=0) whose intermediates are all exact: w_kj, Omega_ll, h_kj, q, CfS, eta."""
    c = p.case
    K, L = c.K, c.L
    F, G, S = sysm._F, sysm._G, sysm.S
    aF, aG, aS = np.abs(F), np.abs(G), np.abs(S)
    miss = sysm.miss
    Cf = F.T @ F
    w = Cf.diagonal()[None, :] - miss.T @ (F * F)                          # [J][K]
    w_budget = Cf.diagonal()[None, :] + miss.T @ (F * F)
    om_budget = np.abs(w).T @ (G * G)                                      # [K][L]: Omega^k_ll
    CfS_budget = np.abs(Cf) @ aS                                           # [K][L]
    Ueff_abs = aF @ aS                                                     # [I][L]
    q_abs = Ueff_abs @ aG.T                                                # [I][J]: |terms| of q_ij
    qF = (miss * q_abs).T @ aF                                             # [J][K]: sum_miss |q| |F|
    r3 = aG @ CfS_budget.T                                                 # [J][K]: sum_l' |G_jl'| |CfS_kl'|
    h_abs = np.abs(sysm.Pv) + r3 + qF                                      # [J][K]
    eta_budget = h_abs.T @ aG                                              # [K][L]
    ok = ((w_budget.max(axis=0) < TWO24)[:, None] & (om_budget < TWO24) & (CfS_budget.max(initial=0) < TWO24)
          & (q_abs[miss == 1].max(initial=0) < TWO24) & (h_abs.max(axis=0) < TWO24)[:, None] & (eta_budget < TWO24)
          & (eta_budget + aS * om_budget < TWO24))
    return sysm.ok & ok.reshape(-1)


# ------------------------------------------------------------------ VB: muS = numer * (1 / tau_p) in fp32 (ssys_chain_vb_kernel)
MU_ULPS = 2          # |muS - numer / tauS| in ulps of the fp32 quotient: one rounding of the reciprocal, one of the product
VB_NUMER_MAX = 2.0 ** 20     # |numer| below this: an error of one unit in numer moves muS by more than 2 MU_ULPS ulps


def vb_states(p):
    return [st for st in p.states if st.varF is not None]


def gibbs_states(p):
    return [st for st in p.states if st.varF is None]
