"""Shared by tests/test_elbo_terms_cases_cpu.py and tests/test_elbo_terms_gpu.py: the eight factor sums of a variational
iteration's record (all_elbo_terms[:, 2:10]) restated on the host, and the cases with the producer and the fold each is there for.

Per iteration every variational model records exp_square_diff, beta_s and, for each of its two outer factors (U, V or F, G),
    [0] sum tau/2 (Var + (E - mu)^2)   [1] sum log(1/2 erfc(-mu sqrt(tau/2)))   [2] sum log tau   [3] sum lambda E
(bnmf_vb_optimised.py:163-177).  Five pieces of device code produce them -- the generic sweep (kernel_sweep.hip), vb_pieces_kernel,
its list form vb_pieces_many, vb_pieces_slabs_kernel (kernel_sweep_vb.hip) and obs_vb_pieces<COV> (kernel_obs_vb.hip) -- and four
fold them: vb_finish_body / vb_finish_many (kernel_misc.hip), obs_vb_finish_kernel, obs_trivb_finish_kernel.  The device forms
every term in fp64 from the fp32 state it stores and run() hands that same state back, so the restatement on the returned state
differs from the record by the order of the additions and a few ulp of erfc / log.

An entry is classified by w = -mu sqrt(tau / 2), the argument of its erfc: ordinary below 26, dead above 28 (erfc is exactly 0 in
fp64: the term is -inf on both sides), and the band between, where erfc is subnormal or about to underflow and two libraries need
not agree on the point at which they flush.  No case may have an entry in the band: a condition on the inputs, not a tolerance."""
import math
from types import SimpleNamespace

import numpy as np
import scipy.special

import _handover_cases as H
import _obs_trivb_cases as TC
from _obs_cases import SHAPES as OBS_SHAPES, _problem, _random_mask

BAND = (26.0, 28.0)
# the three sums whose terms are a few fp64 multiplications of the same fp32 inputs on both sides: the two sides differ in the
# order of the additions and in fma contraction, N 2^-53 sum |terms| with N <= 520 x 130 entries is 7e-12; 1e-9 is the project's
# margin for such sums (tests/test_heldout_gpu.py RTOL)
TOL_SUM = 1e-9
# sum log(1/2 erfc): the device library's fp64 erfc / log against SciPy's.  Two decades above the largest |device - reference| /
# sum |terms| over all finite cases, measured on an MI355X: 2.46e-14 (tests/test_elbo_terms_gpu.py's docstring).  Two decades,
# not three: the same few-ulp difference recurs in every term and does not average out
TOL_ERFC = 2.5e-12
SUM_NAMES = ("quad", "log_erfc", "log_tau", "lambda_E")
TOLS = (TOL_SUM, TOL_ERFC, TOL_SUM, TOL_SUM)
PLANTED = 1e4                   # lambda of the two planted entries of the dead variant ...
# ... but w = (lambda - E[tau] num) / sqrt(2 tau) and the precision tau of an entry grows with the entries its unit observes and
# with the rank: on the two largest tri-factorisation shapes (units of ~2000 observed entries) 1e4 leaves one planted entry at
# w = 36 and the other alive, 1e6 puts both in the hundreds and beyond
PLANTED_LARGE = {(2304, 2100, 32, 32): 1e6, (700, 2500, 5, 32): 1e6}
EXPTAU0 = 1.3
ITERATIONS = 3                  # run(1) three times


# ------------------------------------------------------------------------------------------------ the reference
def widen(x):
    """what the device holds: the fp32 value, as fp64"""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def erfc_argument(mu, tau):
    """w = -mu sqrt(tau / 2) per entry"""
    return -widen(mu) * np.sqrt(widen(tau) / 2.0)


def factor_terms(mu, tau, ex, var, lam):
    """[4][entries]: every entry's term of the four sums, fp64 of the fp32 inputs, each as the reference writes it"""
    mu, tau, ex, var, lam = (widen(x).ravel() for x in (mu, tau, ex, var, lam))
    with np.errstate(all="ignore"):
        return np.array([tau / 2. * (var + (ex - mu) ** 2),
                         np.log(0.5 * scipy.special.erfc(-mu * np.sqrt(tau) / math.sqrt(2))),
                         np.log(tau),
                         lam * ex])


def _fsum(t):
    if np.isnan(t).any():
        return float("nan")
    if np.isinf(t).any():
        assert not (t == np.inf).any() or not (t == -np.inf).any()
        return float("-inf") if (t == -np.inf).any() else float("inf")
    return math.fsum(t)


def factor_sums(mu, tau, ex, var, lam):
    """(the four sums, the four sums of absolute values): math.fsum of factor_terms; a term of -inf gives a sum of -inf (its sum
    of absolute values then runs over the finite terms)"""
    t = factor_terms(mu, tau, ex, var, lam)
    return np.array([_fsum(r) for r in t]), np.array([math.fsum(np.abs(r[np.isfinite(r)])) for r in t])


def classify(mu, tau, margin=0.0):
    """(ordinary, band, dead) boolean arrays of the entries; margin widens the band on both sides"""
    w = erfc_argument(mu, tau)
    band = (w >= BAND[0] - margin) & (w <= BAND[1] + margin)
    return w < BAND[0] - margin, band, w > BAND[1] + margin


# ------------------------------------------------------------------------------------------------ the cases
class TermsCase:
    """name; kind "vb" / "vb_obs" / "tri" / "tri_obs"; mask() -> M; K (and L); env: the switches to set (every other one of
    _handover_cases.SWITCHES is cleared); expect: what describe() must say after a run; nw: sweep_nw of (rows, cols) or None;
    producer: the device code whose sums the case is there for; seed: of the tri-factorisation's state; starved: its key in STARVED;
    problem_key: cases of one key have one problem (the CPU file runs its oracle once); planted: lambda of the dead variant's
    planted entries (PLANTED unless given)."""

    def __init__(self, name, kind, mask, K, L=None, env=None, expect=(), nw=None, producer="", seed=5, starved=False, problem_key=None, planted=None):
        self.name, self.kind, self.mask, self.K, self.L, self.nw, self.producer = name, kind, mask, K, L, nw, producer
        self.seed, self.starved, self.problem_key, self.planted = seed, starved, problem_key or name, planted or PLANTED
        self.env, self.expect = dict(env or {}), tuple(expect)
        self.tri = kind.startswith("tri")
        self.first, self.second = ("F", "G") if self.tri else ("U", "V")

    def __repr__(self):
        return self.name

    def setenv(self, monkeypatch):
        for name in H.SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, v in self.env.items():
            monkeypatch.setenv(name, v)

    def widths(self):
        """columns of the first and of the second factor"""
        return (self.K, self.L) if self.tri else (self.K, self.K)

    def problem(self, variant):
        """R, M, the priors and the seeded state of the variant "finite" or "dead".  Two factors: _obs_vb_cases.vb_problem's state
        (exp = the seeded factors, var seeded, mu = exp, tau = 1), above 32 columns scaled so that E[U] E[V]^T stays of the size
        of R (unscaled, a state of 64 columns is sixteen times R and the first sweep sends dozens of entries past w = 26).  Three
        factors: _obs_trivb_cases.problem's.  dead: lambda of (last unit, last column) of the first factor and of (unit 0, column
        0) of the second is PLANTED, every other one 0.5 -- those two entries end every sweep at w in the hundreds or beyond."""
        assert variant in ("finite", "dead")
        M = np.asarray(self.mask(), dtype=np.float64)
        I, J = M.shape
        Ka, Kb = self.widths()
        lam_a, lam_b = 0.5 * np.ones((I, Ka)), 0.5 * np.ones((J, Kb))
        if variant == "dead":
            lam_a[-1, -1] = self.planted; lam_b[0, 0] = self.planted
        if self.tri:
            R, state = TC.problem(M, self.K, self.L, self.seed)
            pri = dict(alpha=1., beta=1., lambdaF=lam_a, lambdaS=0.5, lambdaG=lam_b)
        else:
            R, U0, V0 = _problem(M, self.K, 5)
            rs = np.random.RandomState(9)
            varU = rs.exponential(0.05, (I, self.K)); varV = rs.exponential(0.05, (J, self.K))
            s = 1.0 if self.K <= 32 else 1.0 / math.sqrt(0.04 * self.K)      # (E[U] E[V]^T is 0.16 K per entry, R is 4)
            U0, V0, varU, varV = U0 * s, V0 * s, varU * s * s, varV * s * s
            state = dict(muU=U0.copy(), tauU=np.ones((I, self.K)), expU=U0.copy(), varU=varU,
                         muV=V0.copy(), tauV=np.ones((J, self.K)), expV=V0.copy(), varV=varV)
            pri = dict(alpha=1., beta=1., lambdaU=lam_a, lambdaV=lam_b)
        planted = ((I - 1, Ka - 1), (0, 0)) if variant == "dead" else (None, None)
        return SimpleNamespace(R=R, M=M, K=self.K, L=self.L, pri=pri, state=state, lam=(lam_a, lam_b), planted=planted,
                               orders=TC.orders(self.K, self.L, ITERATIONS, True) if self.tri else None)

    def oracle(self, p):
        """the fp64 oracle of the case's model at the problem's state"""
        from oracle import bnmtf_oracle as O
        o = O.BNMTFVBOracle(p.R, p.M, p.K, p.L, p.pri) if self.tri else O.BNMFVBOracle(p.R, p.M, p.K, p.pri)
        seed_state(o, p.state)
        return o

    def oracle_sweep(self, o, p, it):
        """one iteration of the oracle; the tri-factorisation's large shapes in the residual form below (the as-written oracle's
        update_S is a pass over R per entry of S: two minutes per iteration at 2304 x 2100, K = L = 32)"""
        if self.tri:
            (tri_sweep_residual_form if p.M.size > RESIDUAL_FORM_FROM else type(o).sweep)(o, *TC.oracle_orders(p.orders[it], p.K, p.L))
        else:
            o.sweep()


RESIDUAL_FORM_FROM = 200000        # entries of R


def tri_sweep_residual_form(o, order_S, order_F, order_G):
    """BNMTFVBOracle.sweep (bnmtf_vb_optimised.py:172-192, 241-273) restated so that no update is a pass over R per entry of S:
    tests/test_elbo_terms_cases_cpu.py pins it to the as-written oracle.  With E = M (R - F S G^T) on the expectations,
      S pass (F, G fixed): F_k^T E G_l is kept as a K x L matrix A; a step of S_kl by d moves A[k', l'] by -d T[k, k', l, l'],
        T = sum_ij M_ij F_ik F_ik' G_jl G_jl'; the two covariance terms are contractions of S with
        P[k, k', l] = (F_k F_k')^T M varG_l and Q[k, l, l'] = varF_k^T M (G_l G_l');
      F and G passes: E kept current by one rank-one update per column (tests/_residual_form.py), the precision and the
        covariance term from M S2G, M G^2, M varG (their transposes for G), which a pass does not change."""
    from oracle.bnmtf_oracle import tn_expectation, tn_variance
    M, R, K, L, I, J, xt = o.M, o.R, o.K, o.L, o.I, o.J, o.exptau
    F, G, S = o.expF, o.expG, o.expS
    FF = (F[:, :, None] * F[:, None, :]).reshape(I, K * K)
    GG = (G[:, :, None] * G[:, None, :]).reshape(J, L * L)
    MGG = M @ GG
    T = (FF.T @ MGG).reshape(K, K, L, L)
    P = (FF.T @ (M @ o.varG)).reshape(K, K, L)
    Q = (o.varF.T @ MGG).reshape(K, L, L)
    tauS = xt * ((o.varF + F ** 2).T @ M @ (o.varG + G ** 2))
    A = F.T @ (M * (R - F @ S @ G.T)) @ G
    for k, l in order_S:
        o.tauS[k, l] = tauS[k, l]
        diff = A[k, l] + S[k, l] * T[k, k, l, l]
        cov_G = S[:, l] @ P[k, :, l] - S[k, l] * P[k, k, l]
        cov_F = S[k, :] @ Q[k, l, :] - S[k, l] * Q[k, l, l]
        o.muS[k, l] = 1.0 / o.tauS[k, l] * (-o.lambdaS[k, l] + xt * diff - xt * cov_G - xt * cov_F)
        new = float(tn_expectation(o.muS[k, l], o.tauS[k, l]))
        o.varS[k, l] = tn_variance(o.muS[k, l], o.tauS[k, l])
        A -= (new - S[k, l]) * T[k, :, l, :]
        S[k, l] = new
    S2S = o.varS + S ** 2
    E = M * (R - F @ S @ G.T)
    MvG, MS2G, MG2 = M @ o.varG, M @ (o.varG + G ** 2), M @ (G ** 2)
    for k in order_F:
        sg = S[k] @ G.T
        Msg2 = M @ sg ** 2
        o.tauF[:, k] = xt * (MS2G @ S2S[k] - MG2 @ S[k] ** 2 + Msg2)
        diff = E @ sg + F[:, k] * Msg2
        cov = ((S[k] * (F @ S)) * MvG).sum(axis=1) - F[:, k] * (MvG @ S[k] ** 2)
        o.muF[:, k] = 1.0 / o.tauF[:, k] * (-o.lambdaF[:, k] + xt * diff - xt * cov)
        new = tn_expectation(o.muF[:, k], o.tauF[:, k])
        o.varF[:, k] = tn_variance(o.muF[:, k], o.tauF[:, k])
        E -= M * np.outer(new - F[:, k], sg)
        F[:, k] = new
    Mt, Et = np.ascontiguousarray(M.T), np.ascontiguousarray(E.T)
    MvF, MS2F, MF2 = Mt @ o.varF, Mt @ (o.varF + F ** 2), Mt @ (F ** 2)
    for l in order_G:
        fs = F @ S[:, l]
        Mfs2 = Mt @ fs ** 2
        o.tauG[:, l] = xt * (MS2F @ S2S[:, l] - MF2 @ S[:, l] ** 2 + Mfs2)
        diff = Et @ fs + G[:, l] * Mfs2
        cov = ((S[:, l] * (G @ S.T)) * MvF).sum(axis=1) - G[:, l] * (MvF @ S[:, l] ** 2)
        o.muG[:, l] = 1.0 / o.tauG[:, l] * (-o.lambdaG[:, l] + xt * diff - xt * cov)
        new = tn_expectation(o.muG[:, l], o.tauG[:, l])
        o.varG[:, l] = tn_variance(o.muG[:, l], o.tauG[:, l])
        Et -= Mt * np.outer(new - G[:, l], fs)
        G[:, l] = new
    o.update_tau(); o.update_exp_tau()


def seed_state(model, state, exptau=EXPTAU0):
    for n, v in state.items():
        setattr(model, n, np.array(v, dtype=float))
    model.exptau = exptau


def factor_state(model, f):
    """(mu, tau, exp, var) of factor f ("U", "V", "F", "G") of a model of this package or of the oracle"""
    return tuple(getattr(model, n + f) for n in ("mu", "tau", "exp", "var"))


def _mask(I, J, frac, seed):
    return lambda: _random_mask(I, J, frac, seed)


def _handover_mask(c):
    return lambda: (~c.missing()).astype(np.float64)


# 1. the generic sweep kernel (kernel_sweep.hip, one row of pieces per unit): unit counts with n mod 4 = 0 .. 3, both KP, K = KP and K < KP
_GEN = {"BNMTF_VB_GENERIC": "1"}
GENERIC_CASES = [TermsCase("generic_%dx%d_K%d" % (I, J, K), "vb", _mask(I, J, 0.6, 100 + I), K, env=_GEN, expect=("vb_sweep=generic",),
                           producer="sweep_kernel")
                 for I, J, K in ((5, 7, 3), (4, 9, 1), (13, 6, 32), (9, 11, 33), (10, 7, 64))]


# 2. the pair-panel kernel (vb_pieces_kernel) and the on-chip kernel (vb_pieces_slabs_kernel) in both block shapes: the four
# variational cases of _handover_cases.py and, of each, the mask drawn again with I and J moved by (+1, +3) and (+3, +1) -- and
# (+2, +6) for the 8-wave on-chip case -- so that n mod 4 takes every value in both directions of both kernels
def _moved(c, dI, dJ):
    # (H.Case.__init__ adds BNMTF_HANDOVER=1 and BNMTF_HANDOVER_REFRESH to whatever it is given: they are taken out here only so
    # that it does not get them twice -- every panel case, moved or not, runs with the hand-over switched on)
    return H.Case("%s_p%dp%d" % (c.name, dI, dJ), "vb", c.I + dI, c.J + dJ, c.K, c.mask,
                  {k: v for k, v in c.env.items() if not k.startswith("BNMTF_HANDOVER")}, c.nw, None, "")


HANDOVER_BASE = list(H.VB_CASES)
HANDOVER_MOVED = [_moved(c, dI, dJ) for c in H.VB_CASES for dI, dJ in ((1, 3), (3, 1))] + [_moved(H.VB_CASES[3], 2, 6)]


def _panel_case(c):
    path = c.env["BNMTF_VB_PATH"]
    return TermsCase(c.name, "vb", _handover_mask(c), c.K, env=c.env, expect=("vb_sweep=" + path,), nw=c.nw,
                     producer="vb_pieces_kernel" if path == "pairs" else "vb_pieces_slabs_kernel")


# ... and, since those all have K <= 6, both kernels once at KP = 64: K < KP on the pair panels, K = KP on the on-chip kernel
HANDOVER_KP64 = [H.Case("vb_pairs_K33", "vb", 69, 91, 33, ("uniform", 0.2, 0), {"BNMTF_WIDE": "1", "BNMTF_VB_PATH": "pairs"}, (16, 16), None, ""),
                 H.Case("vb_masked_K64", "vb", 73, 91, 64, ("uniform", 0.2, 0), {"BNMTF_WIDE": "1", "BNMTF_VB_PATH": "masked"}, (16, 16), None, "")]
PANEL_CASES = [_panel_case(c) for c in HANDOVER_BASE + HANDOVER_MOVED + HANDOVER_KP64]

# 3. the list form (vb_pieces_many, vb_finish_many): three models of one run_many call, I mod 4 = 1, 2, 0, different K
MANY_SPECS = ((69, 90, 4), (70, 90, 7), (72, 90, 12))
MANY_CASES = [TermsCase("many_%dx%d_K%d" % (I, J, K), "vb", _mask(I, J, 0.8, 200 + I), K, expect=("vb_sweep=pairs",), nw=(8, 8),
                        producer="vb_pieces_many")
              for I, J, K in MANY_SPECS]

# 4. the observed-entry layout, two factors: every launch shape of _obs_cases.py
LONG_UNITS = {"row_counts": "3/0", "col_counts": "0/3", "full_matrix_long": "3/0"}


# With fewer than four units in a direction a dead entry starves the other factor: E of the planted entry is ~1e-8, so a unit of
# the other factor that observes nothing else in that column gets a precision near zero there and w in the thousands -- dead as
# well, as the model has it (no other planted position avoids it: with one unit, column k of the other factor depends on that
# unit's entry k alone).  The dead entries beside the planted ones, per iteration (first factor, second factor), as the fp64
# oracle has them (w above 1000; every other entry below 2): the CPU file holds the oracle to this list, the GPU file the device
_COL = lambda n, k: tuple((u, k) for u in range(n))
STARVED = {
    "I1": 3 * (((), _COL(7, 2)),),                      # U[0, 2] is the only entry V's column 2 sees
    "I3": 3 * (((), ((2, 2),)),),                       # unit 2 of V observes row 2 alone
    "J1": (((), ()),) + 2 * ((_COL(7, 0), ()),),        # V[0, 0] is the only entry U's column 0 sees, from the second iteration on
}


def _obs_case(name):
    return TermsCase("obs_" + name, "vb_obs", lambda: OBS_SHAPES[name]()[0], OBS_SHAPES[name]()[1], starved=name if name in STARVED else None,
                     expect=("layout=observed", "long_form_units=%s" % LONG_UNITS.get(name, "0/0")), producer="obs_vb_pieces<0>")


OBS_CASES = [_obs_case(n) for n in sorted(OBS_SHAPES)]

# 5. the tri-factorisation: the generic kernel (units with n mod 4 = 0 .. 3, K = KP = 32 and below) and the pair-panel kernel with
# the covariance term (vb_pieces_kernel behind it), both on the three fast-versus-generic shapes of tests/test_bnmtf_vb_gpu.py --
# (2304, 2100, 32, 32) is vb_pieces_kernel at K = KP for F and for G, (700, 2500, 5, 32) for G alone -- whose unit counts are all
# multiples of four, so the pair-panel kernel also runs on the smallest shapes that keep it with n mod 4 = 1 .. 3 in both
# directions; and the observed layout on _obs_trivb_cases.py's shapes
TRI_SHARED = ((1100, 900, 10, 7), (2304, 2100, 32, 32), (700, 2500, 5, 32))
TRI_GENERIC = [TermsCase("tri_generic_%dx%d_K%d_L%d" % (I, J, K, L), "tri", _mask(I, J, 0.6 if I < 100 else 0.85, 400 + I), K, L, env=_GEN,
                         expect=("tri_vb_sweeps=generic",), producer="sweep_kernel", problem_key="tri_%dx%d" % (I, J),
                         planted=PLANTED_LARGE.get((I, J, K, L)))
               for I, J, K, L in ((5, 7, 2, 3), (6, 11, 1, 1), (7, 8, 4, 5), (8, 7, 32, 32)) + TRI_SHARED]
TRI_PAIRS = [TermsCase("tri_pairs_%dx%d_K%d_L%d" % (I, J, K, L), "tri", _mask(I, J, 0.85, 400 + I), K, L,
                       expect=("tri_vb_sweeps=pairs+cov",), producer="vb_pieces_kernel", problem_key="tri_%dx%d" % (I, J),
                       planted=PLANTED_LARGE.get((I, J, K, L)))
             for I, J, K, L in TRI_SHARED + ((210, 150, 6, 9), (211, 153, 6, 9), (213, 151, 6, 9))]
# seeds of the state at which no entry comes near the band in three iterations (a search over seeds with the fp64 oracle; at
# _obs_trivb_cases.problem's own seed 5, KL1x32 has dozens of dead and band entries by itself and rows one entry at w = 28.2)
TRI_OBS_SEEDS = {"KL1x32": 24, "rows": 9}


def _obs_tri_case(name):
    return TermsCase("obs_tri_" + name, "tri_obs", lambda: TC.CASES[name]()[0], TC.CASES[name]()[1], TC.CASES[name]()[2], seed=TRI_OBS_SEEDS.get(name, 5),
                     expect=("layout=observed", "long_form_units=%s" % TC.LONG_UNITS.get(name, "0/0")), producer="obs_vb_pieces<1>")


OBS_TRI_CASES = [_obs_tri_case(n) for n in sorted(TC.CASES)]

SINGLE_CASES = GENERIC_CASES + PANEL_CASES + OBS_CASES + TRI_GENERIC + TRI_PAIRS + OBS_TRI_CASES
ALL_CASES = SINGLE_CASES + MANY_CASES
VARIANTS = ("finite", "dead")


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ the statements both files make
def check_entries(case, p, variant, model, margin, where, it):
    """The condition on the inputs, on the state of a model or an oracle after iteration it (from 1): no entry of either factor in
    the band (widened by margin), the dead entries exactly the planted ones (none in the finite variant; a starved shape: and the
    ones STARVED lists for the iteration)."""
    for side, (f, planted) in enumerate(zip((case.first, case.second), p.planted)):
        mu, tau = factor_state(model, f)[:2]
        _, band, dead = classify(mu, tau, margin)
        w = erfc_argument(mu, tau)
        assert not band.any(), "%s %s %s: %d entries of %s in the band, w = %s" % (case.name, variant, where, band.sum(), f, w[band][:8])
        want = np.zeros(dead.shape, dtype=bool)
        if planted is not None:
            want[planted] = True
            for at in (STARVED[case.starved][it - 1][side] if case.starved else ()):
                want[at] = True
        assert (dead == want).all(), "%s %s %s: dead entries of %s at %s, planted %s (w = %s)" % (
            case.name, variant, where, f, np.argwhere(dead).tolist()[:8], planted, w[dead][:8])


def reference_sums(case, p, model):
    """[8] sums and [8] sums of absolute values (the first factor's four, the second's) from the model's returned state"""
    a = factor_sums(*factor_state(model, case.first), p.lam[0])
    b = factor_sums(*factor_state(model, case.second), p.lam[1])
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def compare_sums(got, ref, ref_abs, label):
    """|device - reference| <= tol sum |terms| for each of the eight sums; where the reference is -inf the device value is
    exactly -inf.  Returns the eight ratios |device - reference| / sum |terms| (nan where the reference is -inf) and the list of
    the sums that miss, for the caller to print the one and assert the other is empty."""
    ratio = np.full(8, np.nan)
    bad = []
    for c in range(8):
        name = "%s[%d] %s" % (label, 2 + c, SUM_NAMES[c % 4])
        if ref[c] == -np.inf:
            if not got[c] == -np.inf:
                bad.append("%s: device %r where the reference is -inf" % (name, got[c]))
            continue
        assert np.isfinite(ref[c]), (name, ref[c])
        ratio[c] = abs(got[c] - ref[c]) / ref_abs[c] if ref_abs[c] > 0 else abs(got[c] - ref[c])
        if not (np.isfinite(got[c]) and abs(got[c] - ref[c]) <= TOLS[c % 4] * ref_abs[c]):
            bad.append("%s: device %.17g reference %.17g sum |terms| %.6g (ratio %.3g, tol %.1g)" % (name, got[c], ref[c], ref_abs[c], ratio[c], TOLS[c % 4]))
    return ratio, bad
