"""Cases of the exact test of the tri-factorisation's S system on the observed-entry layout (csrc/kernel_obs_tri.hip handing over
to csrc/kernel_ssys.hip; tests/test_obs_tri_gpu.py), and a NumPy model of what the device forms.

For a state (F, S, G) and a = (k, l) = k L + l the hook bnmtf_otri_cond_params(which = 1) rebuilds

    W_j  = sum_{i in Omega_j} F_i F_i^T            obs_tri_gram_kernel: one wave per column, 16 entries a trip, two per MFMA
    Pv_j = sum_{i in Omega_j} R_ij F_i             the same launch
    Gc_j = G_j G_j^T                               gamma_pack_kernel
    b    = sum_j Pv_j (x) G_j                      ssys_b_kernel: one partial per 64 columns
    A    = sum_j W_j (x) Gc_j                      ssys_gemm_bf16_kernel over nsplit ranges of 16-column steps, ssys_reduce_kernel
    r    = b - A S                                 ssys_residual_kernel
    numer_a = fmaf(tau, r_a + S_a A_aa, -lambdaS), tauS_a = tau A_aa          ssys_chain_kernel's cond branch

Every case puts F, S, G, R on integer grids with tau = 1 and lambdaS = 0.5.  An output is CHECKED when every intermediate that feeds
it is an integer whose sum of |terms| -- in any order -- is below 2^24 (System.ok), so that its only correct fp32 value is the
exact one, and when the three bf16 split products that the packed GEMM drops (m.l, l.m, l.l: _contraction_cases.DROPPED) are zero
on its operands.  F is 0/1 with one or two ones per row, so W_j counts rows (at most the column's entry count, below 2^16: hi and
mid terms only); G is 0/1/2, so Gc_j is at most 4 (a hi term only); S holds distinct nonzero integers, so a wrong A[a][a'] for
any a' moves numer_a; R holds integers 0 .. 7, zero among them.

EDGES says which case covers which launch edge; tests/test_obs_tri_cases_cpu.py checks that list against the cases themselves."""
import numpy as np

from _contraction_cases import DROPPED, LAM, TWO24, split3
from _obs_cases import _counts_mask
from _ssys_cases import ssys_launch, tri_count

GRAM_WAVES = 4          # csrc/kernels.h kObsTriGramWaves: columns per block of obs_tri_gram_kernel
GRAM_TRIP = 16          # entries per trip of its loop (eight per half wave)
COL_COUNTS = (1, 63, 64, 65, 129, 513)      # entries per column, beside full columns: one below / at / above the 64-entry steps, odd trips, 33 trips


class Case:
    def __init__(self, name, I, J, K, L, counts=(), note=""):
        self.name, self.I, self.J, self.K, self.L, self.counts, self.note = name, I, J, K, L, tuple(counts), note

    @property
    def id(self):
        return "%s-%dx%dx%dx%d" % (self.name, self.I, self.J, self.K, self.L)

    def launch(self):
        return ssys_launch(self.K, self.L, self.J)


def _mask(case):
    """The mask of a case.  With column counts: _obs_cases._counts_mask transposed -- column u has counts[u] entries at seeded rows,
    the columns behind them are full -- widened with full columns to J.  Without: every entry observed."""
    if not case.counts:
        return np.ones((case.I, case.J))
    M = _counts_mask(list(case.counts), case.I, 40 + case.J).T.copy()          # [I][len(counts) + 2]
    assert M.shape[1] <= case.J
    return np.concatenate([M, np.ones((case.I, case.J - M.shape[1]))], axis=1)


# I x J, K x L; the (K, L) pairs of the issue, every J of its list, I at 1 and 5, the column counts beside full columns
CASES = [
    Case("one", 1, 1, 1, 1, note="everything of size one: I = 1, J = 1, K = L = 1"),
    Case("i5", 5, 15, 2, 3, note="I = 5, J = 15: less than one 16-column step, full columns of 5 entries (one partial trip)"),
    Case("j16", 5, 16, 31, 32, note="J = 16: exactly one step; K = 31 (a tile with one empty row and column), L = 32"),
    Case("j17", 1, 17, 32, 1, note="I = 1 again with J = 17: a second step of one column; K = 32 with L = 1"),
    Case("j63", 40, 63, 2, 3, note="J = 63: one b block, short of its 64 columns"),
    Case("j64", 40, 64, 32, 32, note="J = 64: one full b block; K = L = 32, all 528 packed pairs on both sides"),
    Case("j65", 40, 65, 31, 32, note="J = 65: a second b block of one column"),
    Case("counts", 520, 130, 32, 32, COL_COUNTS, note="columns of 1, 63, 64, 65, 129 and 513 entries beside full ones (520); J = 130: two ranges, three b blocks"),
    Case("counts_small", 520, 17, 2, 3, COL_COUNTS, note="the same columns at K = 2, L = 3"),
    Case("counts_32x1", 520, 15, 32, 1, COL_COUNTS, note="the same columns at K = 32, L = 1"),
]

# which case covers which edge of the launches (tests/test_obs_tri_cases_cpu.py checks every line against edges_of)
EDGES = {
    "K,L=(1,1)": "one", "K,L=(2,3)": "i5", "K,L=(31,32)": "j16", "K,L=(32,1)": "j17", "K,L=(32,32)": "j64",
    "I=1": "one", "I=5": "i5",
    "J=1": "one", "J=15": "i5", "J=16": "j16", "J=17": "j17", "J=63": "j63", "J=64": "j64", "J=65": "j65", "J=130": "counts",
    "column of 1": "counts", "column of 63": "counts", "column of 64": "counts", "column of 65": "counts", "column of 129": "counts",
    "column of 513": "counts", "column of I": "counts",
    "entry value 0": "counts",
    "last gram block of 1 column": "j17", "last gram block of 2 columns": "counts", "last gram block of 3 columns": "i5", "gram blocks all full": "j16",
    "last trip of 1 entry": "one", "last trip of 8 entries": "j63", "last trip of 15 entries": "counts", "last trip of 16 entries": "counts",
    "trips: 1": "i5", "trips: 33": "counts",
    "GEMM ranges: 1": "j65", "GEMM ranges: 2": "counts", "last range short of its steps": "counts",
    "b blocks: 1": "j64", "b blocks: 2": "j65", "b blocks: 3": "counts", "last b block of 1 column": "j65", "last b block of 63 columns": "j63",
}


def edges_of(case):
    """The launch edges a case hits: what EDGES names, computed from the case's mask and the launch rules of kernels.h / api_obs_tri.inc."""
    M = _mask(case)
    R = problem(case).R
    cols = (M != 0).sum(axis=0).astype(int)
    la = case.launch()
    e = {"K,L=(%d,%d)" % (case.K, case.L), "I=%d" % case.I, "J=%d" % case.J}
    e |= {"column of %d" % c for c in set(cols.tolist())}
    if case.I in set(cols.tolist()) and len(set(cols.tolist())) > 1:
        e.add("column of I")
    if ((R == 0) & (M != 0)).any():
        e.add("entry value 0")
    last = case.J % GRAM_WAVES
    e.add("gram blocks all full" if last == 0 else "last gram block of %d column%s" % (last, "" if last == 1 else "s"))
    e |= {"last trip of %d entr%s" % ((c - 1) % GRAM_TRIP + 1, "y" if (c - 1) % GRAM_TRIP == 0 else "ies") for c in set(cols.tolist())}
    e |= {"trips: %d" % (-(-c // GRAM_TRIP)) for c in set(cols.tolist())}
    e.add("GEMM ranges: %d" % la["nsplit"])
    if la["last"] < la["range"]:
        e.add("last range short of its steps")
    e.add("b blocks: %d" % la["bblocks"])
    e.add("last b block of %d column%s" % ((case.J - 1) % 64 + 1, "" if (case.J - 1) % 64 == 0 else "s"))
    return e


class State:
    def __init__(self, F, S, G):
        self.F, self.S, self.G = F, S, G


class Problem:
    def __init__(self, case, R, M, states):
        self.case, self.R, self.M, self.states = case, R, M, states


def _onehot(rs, n, W, two=0.3):
    X = np.zeros((n, W), np.float32)
    X[np.arange(n), rs.randint(W, size=n)] = 1
    if W > 1:
        extra = np.flatnonzero(rs.random_sample(n) < two)
        X[extra, rs.randint(W, size=len(extra))] = 1
    return X


def problem(case):
    rs = np.random.RandomState((case.I * 7919 + case.J * 104729 + case.K * 31 + case.L) % (2 ** 31))
    M = _mask(case)
    R = rs.randint(0, 8, size=(case.I, case.J)).astype(np.float32)            # (0 among the values: an entry that is there and adds nothing)
    K, L = case.K, case.L
    states = []
    for _ in range(2):
        F = _onehot(rs, case.I, K)
        G = _onehot(rs, case.J, L) * rs.randint(1, 3, size=(case.J, 1)).astype(np.float32)
        S = (rs.permutation(K * L) + 1).reshape(K, L).astype(np.float32)
        states.append(State(F, S, G))
    return Problem(case, R, M, states)


def _pairs(K):
    kk = np.array([(k, kp) for k in range(K) for kp in range(k, K)], dtype=np.int64).reshape(-1, 2)
    full = np.zeros((K, K), np.int64)
    for p, (k, kp) in enumerate(kk):
        full[k, kp] = full[kp, k] = p
    return kk, full


def _abs3(x):
    s = split3(np.asarray(x, dtype=np.float32))
    return sum(np.abs(s[t].astype(np.float64)) for t in "hml")


class System:
    """Everything the device forms for one (problem, state), in fp64 (exact on these grids), with the budgets of every intermediate."""

    def __init__(self, p, st):
        c = p.case
        K, L = c.K, c.L
        self.K, self.L, self.n2 = K, L, K * L
        F, G, S = st.F.astype(np.float64), st.G.astype(np.float64), st.S.astype(np.float64)
        Mf = (p.M != 0).astype(np.float64)
        kk, self.kfull = _pairs(K)
        ll, self.lfull = _pairs(L)
        assert len(kk) == tri_count(K) and len(ll) == tri_count(L)
        FF = F[:, kk[:, 0]] * F[:, kk[:, 1]]                                   # [I][PK]
        self.W = Mf.T @ FF                                                     # [J][PK] the observed rows' outer products
        self.Gc = G[:, ll[:, 0]] * G[:, ll[:, 1]]                              # [J][PL]
        Rm = np.where(Mf == 1, p.R.astype(np.float64), 0.0)
        self.Pv = Rm.T @ F                                                     # [J][K]
        self.Ap = self.W.T @ self.Gc
        self.A = self.unpack(self.Ap)
        self.b = (self.Pv[:, :, None] * G[:, None, :]).sum(axis=0).reshape(-1)
        s = S.reshape(-1)
        self.num = self.b - self.A @ s + np.diag(self.A) * s
        self.tau = np.diag(self.A).copy()
        self.numer = (self.num - LAM).astype(np.float32)
        # budgets: sums of |terms| of every intermediate, in any order (all terms are non-negative integers here but S's products)
        W32, Gc32 = self.W.astype(np.float32), self.Gc.astype(np.float32)
        sW, sG = split3(W32), split3(Gc32)
        gemm_budget = self.unpack(_abs3(W32).T @ _abs3(Gc32))
        gemm_drop = self.unpack(sum(np.abs(sW[a].astype(np.float64)).T @ np.abs(sG[b].astype(np.float64)) for a, b in DROPPED))
        b_budget = (np.abs(self.Pv).T @ np.abs(G)).reshape(-1)
        r_budget = np.abs(self.b) + np.abs(self.A) @ np.abs(s)
        self.budget = dict(W=self.W.max(initial=0), Pv=np.abs(self.Pv).max(initial=0), Gc=self.Gc.max(initial=0), gemm=gemm_budget.max(initial=0),
                           dropped=gemm_drop.max(initial=0), b=b_budget.max(initial=0), r=r_budget.max(initial=0),
                           numer=np.abs(self.num).max(initial=0) + np.abs(np.diag(self.A) * s).max(initial=0) + LAM)
        self.ok = ((gemm_budget.max(axis=1) < TWO24) & (gemm_drop.max(axis=1) == 0) & (b_budget < TWO24) & (r_budget < TWO24)
                   & (r_budget + np.abs(np.diag(self.A) * s) < TWO24) & bool(self.W.max(initial=0) < TWO24) & bool(np.abs(self.Pv).max(initial=0) < TWO24))

    def unpack(self, Ap):
        """packed [PK][PL] -> the full n2 x n2 system (ssys_reduce_kernel's writes, both of them)"""
        K, L = self.K, self.L
        return Ap[self.kfull[:, None, :, None], self.lfull[None, :, None, :]].reshape(K * L, K * L)


# ------------------------------------------------------------------ the runs that tests/test_obs_tri_gpu.py's child processes repeat
PRI_TRI = dict(alpha=1., beta=1., lambdaF=0.5, lambdaS=0.5, lambdaG=0.5)


def long_problem():
    """Rows of 555 .. 578 entries: every unit of the F half sweep is beyond the register form's 512."""
    from bnmtf_amd.synthetic import generate_bnmtf
    R, M, _, _, _ = generate_bnmtf(40, 600, 3, 2, 0.05, seed_data=3, seed_mask=0)
    M = M.astype(float)
    rs = np.random.RandomState(17)
    return R.astype(np.float64), M, rs.exponential(0.5, (40, 3)) + 0.1, rs.exponential(0.5, (3, 2)) + 0.1, rs.exponential(0.5, (600, 2)) + 0.1


def long_form_runs():
    """One mode iteration and three drawn ones on long_problem(): samples, tau, metrics, and what describe() says."""
    from bnmtf_amd import bnmtf_gibbs_optimised
    R, M, F0, S0, G0 = long_problem()
    out = {}
    for tag, kw, n, update in (("mode", {}, 1, 'mode'), ("draw", dict(seed=123), 3, 'draw')):
        b = bnmtf_gibbs_optimised(R, M, 3, 2, PRI_TRI, verbose=False, layout='observed', **kw)
        b.F, b.S, b.G, b.tau = F0.copy(), S0.copy(), G0.copy(), 1.3
        b.run(n, update=update)
        out.update({tag + "_" + k: v for k, v in dict(F=b.all_F.copy(), S=b.all_S.copy(), G=b.all_G.copy(), tau=b.all_tau.copy(),
                                                      perf=np.array([b.all_performances[m] for m in ("MSE", "R^2", "Rp")])).items()})
        desc = b.describe()
        b.close()
    return out, desc
