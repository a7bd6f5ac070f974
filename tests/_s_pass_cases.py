"""Cases and checks of the step-by-step tests of the variational S pass (csrc/kernel_trivb.hip: ssys_chain_vb_kernel and
ssys_chain_vb_blocked_kernel; csrc/device_rng.h: tn_moments_f32, tn_mean_f32_regime; csrc/tn_mean_table.h).

A pass walks the K.L entries of S in a given order; step a forms

    tauS_a = tau A_aa ,   muS_a = (tau s_a - lambda_a) / tauS_a ,   s_a = b_a - sum_{t != a} A_at E_t ,   E_a <- E[TN(muS_a, tauS_a)]

on the dense second-moment system (A, b) of kernel_ssys.hip, and every later step sees the new E_a.

THE SYSTEM IS EXACT.  F, G, R and the initial E[S] lie on small integer grids (the construction of _ssys_cases.py: System(p, st,
vb=True) with System.ok.all() required), so A, b and r0 = b - A E0 are integers below 2^24 and their only correct fp32 values are
the exact ones; exptau is a power of two, so tauS_a = tau A_aa has one correct value too.  A carries two all-ones rows of F and two
all-ones rows of G observed against each other: every A_at >= 1, so every step's delta reaches every later step.

THE PASS IS STEERED.  lambdaS is a K x L matrix without a sign check (_base.broadcast_lambda), and muS_a is linear in lambda_a.  An
fp64 replay walks the pass in its order; at step a it picks lambda_a so that x_a = -muS_a sqrt(tauS_a) hits the step's target,
rounds lambda_a to fp32 and goes on with the rounded value.  So the arithmetic path of every step is chosen here:
    fast     x <= -6         the kernels' two-FMA shortcut, E = sigma |x|
    neg      -6 < x <= 0     the blocked kernel's segment table (segments 0..11), the routine's x <= 0 branch
    tab      0 < x < 26      the table (segments 12..63), the routine's polynomial branch
    far      26 <= x <= 30   beyond the table: tn_mean_f32_regime<true> inside the wave
    beyond   x > 30          the -30 sigma fall-back 1 / (|mu| tau)
Targets keep 0.05 from the switches at -6, 0, 26, 30 and from the segment boundaries (the replay's x keeps MARGIN = 1e-3), except
the deliberate EDGE steps aimed at -6, 26 and 30 themselves, where either side is right.
The kseg = -1 edge of the blocked kernel (a step that fails nm >= thr and still lands below segment 0) is NOT reachable with
finite inputs: thr = RN(6 / hh) is a correctly rounded quotient (the library is built without fast-math), an fp32 nm < RN(y) is
<= y, so nm (2 hh) <= 12 exactly, the FMA's exact value 12 - nm (2 hh) is >= 0 and so is its rounding: kseg >= 0.  Only a NaN
reaches that branch.  The edge steps at -6 walk both sides of the switch itself.

WHICH KERNEL (launch_ssys_chain_vb, restated in chain_kernel): the blocked kernel for a whole pass with 64 <= K.L <= 1024 that
also writes the moments, unless BNMTF_VB_CHAIN=steps; the barrier-per-step kernel otherwise (K.L < 64, the single-step hook).

CHECKS, for every entry of every case (u = 2^-24):
 (a) check_moments: expS, varS against the fp64 truncated-normal moments of the RETURNED (muS, tauS) -- written with
     scipy.special.erfcx (x > 0: lam = sqrt(2/pi) / erfcx(x / sqrt 2); x <= 0: the complementary form; loss ~ x^2 2^-53), beyond
     the -30 sigma switch the reference's fall-back 1 / (|mu| tau) and its square; within 1e-5 relative of that switch either
     side.  Tolerances: the project's own for this routine against the formula (test_tn_moments_coeffs_cpu.py), rtol 2e-6 (mean),
     5e-6 (variance).
 (b) check_steps: an fp64 replay in the pass's order that takes the DEVICE's own E after every step and carries a running bound
     of the roundings (see there).  tauS bit for bit, muS within the bound.
Nothing in a bound is measured.  The CPU side (test_s_pass_cases_cpu.py) feeds both checks a NumPy fp32 restatement of the two
kernels (chain_steps_f32, chain_blocked_f32), and the same restatement with one fault at a time (FAULTS), which must fail."""
import functools
import importlib.util
import os
import re

import numpy as np
from scipy.special import erfcx

from _ssys_cases import Case, Problem, State, System, _mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
MARGIN = 1e-3                       # the replay's x of a non-edge step keeps this from -6, 0, 26, 30
RTOL_MEAN, RTOL_VAR = 2e-6, 5e-6    # test_tn_moments_coeffs_cpu.py: the fp32 routine against the reference formula
SWITCH_BAND = 1e-5                  # relative distance from the -30 sigma switch within which either side is accepted
TABLE_VS_ROUTINE = 1e-6             # 3e-7 (table) + 2.5e-7 (routine) + six ulps (rsq, rcp, exp2): in-wave mean against the stored one
SWITCHES = (-6.0, 0.0, 26.0, 30.0)
NSEG, X0, WSEG = 64, -6.0, 0.5


# ------------------------------------------------------------------ the host's launch (kernel_trivb.hip: launch_ssys_chain_vb)
def chain_kernel(K, L, n_order=None, only_params=False, steps_switch=False):
    n_order = K * L if n_order is None else n_order
    blocked = not (only_params or n_order < 64 or n_order > 1024 or n_order != K * L or steps_switch)
    return "blocked" if blocked else "steps"


STEP_SHAPES = [(1, 1), (3, 4), (1, 13), (5, 5), (7, 9)]
BLOCKED_SHAPES = [(8, 8), (5, 13), (6, 11), (13, 15), (12, 16), (16, 16), (31, 31), (31, 32), (32, 32)]
OBSERVED_SHAPES = [(5, 13), (16, 16), (31, 32)]
TAUS = (1.0, 0.25, 8.0)             # variant 0: exptau = 1; variant 1: the other two in turn


class PassCase:
    """One steered pass: the shape, the order (variant 0: the identity, 1: a shuffle), exptau, the layout it runs on."""

    def __init__(self, K, L, variant, layout="dense"):
        self.K, self.L, self.n, self.variant, self.layout = K, L, K * L, variant, layout
        shape_no = (STEP_SHAPES + BLOCKED_SHAPES).index((K, L))
        self.tau = TAUS[0] if variant == 0 else TAUS[1 + shape_no % 2]
        self.kernel = chain_kernel(K, L)
        self.seed = 1000 * shape_no + variant

    @property
    def id(self):
        return "%dx%d-%s-tau%g%s" % (self.K, self.L, "id" if self.variant == 0 else "shuffled", self.tau,
                                     "-observed" if self.layout == "observed" else "")

    @property
    def key(self):
        return (self.K, self.L, self.variant)


CASES = [PassCase(K, L, v) for K, L in STEP_SHAPES + BLOCKED_SHAPES for v in (0, 1)]
OBSERVED_CASES = [PassCase(K, L, 1, "observed") for K, L in OBSERVED_SHAPES]


# ------------------------------------------------------------------ the exact system
SIZE_I = 140


def size_J(L):
    return max(17, 2 * L + 3)


@functools.lru_cache(maxsize=None)
def system(K, L):
    """(Problem, State, System) of a shape: F and G 0/1 with up to three ones a row and every column used, two all-ones rows each,
    integer variances, E0[S] in 1..3."""
    I, J = SIZE_I, size_J(L)
    case = Case(I, J, K, L, ("XV",), None, vb=True)
    rs = np.random.RandomState(77 + 131 * K + L)
    M, cols = _mask(case, rs)
    R = rs.randint(1, 8, size=(I, J)).astype(np.float32)

    def factor(n, W):
        X = np.zeros((n, W), np.float32)
        X[np.arange(n), np.arange(n) % W] = 1
        for _ in range(2):
            X[np.arange(n), rs.randint(W, size=n)] = 1
        return X

    F, G = factor(I, K), factor(J, L)
    free = [j for j in range(J) if j not in cols.values()] or [0]
    istar, jstar = [3, I // 2], [free[0], free[len(free) // 2]]
    F[istar] = 1
    G[jstar] = 1
    M[np.ix_(istar, jstar)] = 1
    varF = np.where(rs.random_sample((I, K)) < 0.3, rs.randint(1, 3, (I, K)), 0).astype(np.float32)
    varG = np.where(rs.random_sample((J, L)) < 0.3, rs.randint(1, 3, (J, L)), 0).astype(np.float32)
    S0 = rs.randint(1, 4, size=(K, L)).astype(np.float32)
    st = State("XV", F, S0, G, varF, varG)
    p = Problem(case, R, M, cols, [st])
    return p, st, System(p, st, vb=True)


def residual0(s):
    return s.b - s.A @ s.S.reshape(-1)


# ------------------------------------------------------------------ fp64 truncated-normal moments (the reference of check (a))
def tn_moments_ref(mu, tau):
    """(E, Var, x, beyond) of TN(mu, tau) on [0, inf) in fp64; beyond: mu < -30 sigma, the reference's fall-back applies"""
    mu, tau = np.asarray(mu, np.float64), np.asarray(tau, np.float64)
    with np.errstate(all="ignore"):
        sig = 1.0 / np.sqrt(tau)
        x = -mu * np.sqrt(tau)
        ax = np.abs(x)
        e = erfcx(ax / np.sqrt(2.0))
        p = np.exp(-0.5 * ax * ax)
        lam = np.where(x > 0, np.sqrt(2.0 / np.pi) / e, p / np.sqrt(2.0 * np.pi) / (1.0 - 0.5 * p * e))
        r = np.where(x > 0, lam - x, lam + ax)
        h = 1.0 - lam * r
        fe = 1.0 / (np.abs(mu) * tau)
    return sig * r, sig * sig * h, x, fe, fe * fe


def regime(x):
    x = np.asarray(x, np.float64)
    return np.select([x <= -6, x <= 0, x < 26, x <= 30], ["fast", "neg", "tab", "far"], "beyond")


def segment(x):
    return np.floor((np.asarray(x, np.float64) - X0) / WSEG).astype(np.int64)


# ------------------------------------------------------------------ targets and the steering replay
def targets(case):
    """per position of the order: the target x, and whether the step is a deliberate edge step"""
    n, rs = case.n, np.random.RandomState(case.seed)
    x = rs.uniform(-30.0, -6.5, n)
    edge = np.zeros(n, bool)
    slow = np.zeros(n, bool)
    if case.kernel == "blocked":
        nblk = (n + 63) // 64
        for b in range(nblk):
            lo, hi = 64 * b, min(n, 64 * b + 64)
            if nblk >= 3 and b == 1:
                slow[lo:hi] = True                                  # a block of 64 slow steps
            elif nblk >= 4 and b == 2:
                continue                                            # a block without one
            else:
                slow[lo:hi] = rs.random_sample(hi - lo) < 0.25
                slow[lo] = slow[hi - 1] = True                      # lane 0, the block's last lane (63, or the pass's last step)
                slow[min(lo + 1, hi - 1)] = True                    # two in a row
    elif n == 1:
        slow[0] = case.variant == 0
    else:
        slow = rs.random_sample(n) < 0.5
        slow[-1] = slow[n // 2] = True
    neg, pos = 5 * case.seed, 11 * case.seed
    for j, i in enumerate(np.flatnonzero(slow)):
        kind = (j + case.variant) % 5
        if j == 0:
            x[i] = -4.2                                             # (what a shortcut taken down to x <= -4 would get wrong beyond the tolerance)
        elif case.variant == 1 and j in (5, 6, 7) and slow.sum() >= 10:
            x[i] = (-6.0, 26.0, 30.0)[j - 5]
            edge[i] = True
        elif kind == 0:
            x[i] = X0 + WSEG * (neg % 12 + rs.uniform(0.1, 0.9)); neg += 1
        elif kind == 1:
            x[i] = rs.uniform(26.1, 29.9)
        elif kind == 2:
            x[i] = rs.uniform(30.1, 40.0)
        else:
            x[i] = X0 + WSEG * (12 + pos % 52 + rs.uniform(0.1, 0.9)); pos += 1
    return x, edge


def order_of(case):
    n = case.n
    return np.arange(n) if case.variant == 0 else np.random.RandomState(case.seed + 7).permutation(n)


class Steered:
    """The fp64 replay of a case: order, lam = lambdaS (fp32 values, K x L), and per POSITION of the order the target, x, mu, tauS,
    E (the new mean) and the edge flags."""


@functools.lru_cache(maxsize=None)
def _steered(K, L, variant):
    case = PassCase(K, L, variant)
    _, _, s = system(K, L)
    tau, n = case.tau, case.n
    order = order_of(case)
    xt, edge = targets(case)
    A, E0 = s.A, s.S.reshape(-1).astype(np.float64)
    r = residual0(s)
    lam = np.zeros(n, np.float32)
    out = Steered()
    out.x, out.mu, out.E = np.zeros(n), np.zeros(n), np.zeros(n)
    for i, a in enumerate(order):
        tp = tau * A[a, a]
        sa = r[a] + A[a, a] * E0[a]
        lam[a] = np.float32(tau * sa + xt[i] * np.sqrt(tp))            # mu = -x / sqrt(tauS)
        mu = (tau * sa - float(lam[a])) / tp
        e, _, x, fe, _ = tn_moments_ref(mu, tp)
        enew = float(np.float32(fe if x > 30 else e))
        out.x[i], out.mu[i], out.E[i] = x, mu, enew
        r = r - (enew - E0[a]) * A[a]
    out.order, out.edge, out.lam, out.tauS, out.target = order, edge, lam.reshape(K, L), tau * np.diag(A)[order], xt
    return out


def steered(case):
    return _steered(*case.key)


def orders_row(case):
    """run()'s orders argument: [1][K L + K + L]"""
    return np.concatenate([order_of(case), np.arange(case.K), np.arange(case.L)]).astype(np.int32)[None, :]


# ------------------------------------------------------------------ coverage conditions
def case_conditions(case):
    """what must hold for one case (asserted on the CPU and at the start of the case's GPU test)"""
    _, _, s = system(case.K, case.L)
    assert s.ok.all(), "%s: %d entries of the system are not exact" % (case.id, int((~s.ok).sum()))
    assert np.diag(s.A).min() >= 1 and s.A.min() >= 1
    assert np.float32(case.tau) == case.tau and np.log2(case.tau) == np.round(np.log2(case.tau))
    assert case.kernel == ("blocked" if 64 <= case.n <= 1024 else "steps")
    st = steered(case)
    d = np.abs(st.x[:, None] - np.array(SWITCHES)[None, :]).min(axis=1)
    assert (d[~st.edge] >= MARGIN).all(), "%s: a step within %g of a switch" % (case.id, MARGIN)
    assert (np.abs(st.x - st.target)[~st.edge] < 0.04).all()          # (the rounding of lambda to fp32 moved no step far from its target)
    got = set(regime(st.x[~st.edge]).tolist())
    if case.kernel == "blocked":
        assert got == {"fast", "neg", "tab", "far", "beyond"}, (case.id, got)
    E0 = s.S.reshape(-1)[st.order]
    move = np.abs(st.E - E0) / E0
    assert np.median(move) > 0.25, "%s: the pass leaves E[S] where it was (median move %.3f)" % (case.id, np.median(move))
    return st


def slow_map(st):
    return regime(st.x) != "fast"


def global_coverage(cases=None):
    """the conditions over all shapes; returns what was found (the CPU test prints it)"""
    cases = CASES if cases is None else cases
    segs, places, patterns = set(), set(), set()
    for c in cases:
        st = steered(c)
        slow = slow_map(st) & ~st.edge
        table = slow & (st.x < 26)
        segs |= set(segment(st.x[table]).tolist())
        if c.kernel != "blocked":
            continue
        n, nblk = c.n, (c.n + 63) // 64
        pos = np.flatnonzero(slow)
        if (pos % 64 == 0).any(): places.add("lane 0")
        if (pos % 64 == 63).any(): places.add("lane 63")
        if (pos < 64).any(): places.add("first block")
        if n % 64 and (pos >= 64 * (nblk - 1)).any(): places.add("last, partial block")
        if slow[-1]: places.add("last step")
        if (slow[1:] & slow[:-1]).any(): patterns.add("two consecutive slow steps")
        allslow = slow_map(st)
        for b in range(nblk):
            blk = allslow[64 * b:64 * b + 64]
            if not blk.any(): patterns.add("a block with no slow step")
            if blk.size == 64 and blk.all(): patterns.add("a block of 64 slow steps")
    assert segs == set(range(NSEG)), "table segments never hit: %s" % sorted(set(range(NSEG)) - segs)
    assert places == {"lane 0", "lane 63", "first block", "last, partial block", "last step"}, places
    assert patterns == {"two consecutive slow steps", "a block with no slow step", "a block of 64 slow steps"}, patterns
    return segs, places, patterns


# ------------------------------------------------------------------ check (a)
def check_moments(mu, tau, E, V):
    """Returns (largest |diff| / tolerance of the mean, of the variance, indices that fail)."""
    mu, tau, E, V = (np.asarray(v, np.float64).reshape(-1) for v in (mu, tau, E, V))
    e, v, x, fe, fv = tn_moments_ref(mu, tau)
    with np.errstate(all="ignore"):
        main = np.stack([np.abs(E - e) / (RTOL_MEAN * e), np.abs(V - v) / (RTOL_VAR * v)])
        fall = np.stack([np.abs(E - fe) / (RTOL_MEAN * fe), np.abs(V - fv) / (RTOL_VAR * fv)])
    beyond = mu < -30.0 / np.sqrt(tau)
    ratio = np.where(beyond[None, :], fall, main)
    band = np.abs(x - 30.0) <= 30.0 * SWITCH_BAND
    ratio = np.where(band[None, :], np.minimum(main.max(axis=0), fall.max(axis=0))[None, :], ratio)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    bad = np.flatnonzero((ratio > 1).any(axis=0))
    return float(ratio[0].max()), float(ratio[1].max()), bad


# ------------------------------------------------------------------ check (b)
def check_steps(case, lam, mu_dev, tau_dev, E_dev):
    """The pass explained step by step by the device's own earlier results.  In the pass's order, in fp64, with E_cur = E0, r = r0,
    acc = 0: at step a
        s = b_a - sum_{t != a} A_at E_cur_t = r_a + A_aa E0_a ,      mu_ref = (tau s - lambda_a) / (tau A_aa)
        |muS[a] - mu_ref| <= [tau acc_a + 8 u (tau (|A_aa E0_a| + |r_a|) + |lambda_a| + |tau s - lambda_a|)] / (tau A_aa)
            (8 u: the roundings of c = fma(tau A_aa, E0, -lambda), nm = fma(tau, r, c) -- or fma(tau, fma(A_aa, E0, r), -lambda) --,
            1 / tauS and the product, each relative to a quantity that is listed)
        tauS[a] == tau A_aa
    then, with the DEVICE's E:  delta = expS[a] - E0_a ;  r <- r - delta A[a, :] ;
        acc_t += u (|r_t| + 2 |delta A_at|) + |A_at| eta_a        (the FMA's rounding of r_t; the product's; delta's own error)
        eta_a = 2 u max(E0_a, expS[a])     (delta = fl(E_new - E_old) against the stored fl(E_new))
              + TABLE_VS_ROUTINE expS[a]   on the blocked kernel for -6.01 < x_a < 26.01: the step's own wave took the table's mean
    Returns (largest |diff| / bound, positions that fail, positions whose tauS is not exact)."""
    _, _, s = system(case.K, case.L)
    A, tau = s.A, case.tau
    order = order_of(case)
    lam, mu_dev, tau_dev, E_dev = (np.asarray(v, np.float64).reshape(-1) for v in (lam, mu_dev, tau_dev, E_dev))
    E0 = s.S.reshape(-1).astype(np.float64)
    r = residual0(s)
    acc = np.zeros(case.n)
    ratio = np.zeros(case.n)
    tau_bad = []
    blocked = case.kernel == "blocked"
    for i, a in enumerate(order):
        aaa = A[a, a]
        tp = tau * aaa
        if tau_dev[a] != float(np.float32(tp)):
            tau_bad.append(i)
        sa = r[a] + aaa * E0[a]
        num = tau * sa - lam[a]
        bound = (tau * acc[a] + 8 * U * (tau * (abs(aaa * E0[a]) + abs(r[a])) + abs(lam[a]) + abs(num))) / tp
        diff = abs(mu_dev[a] - num / tp)
        ratio[i] = diff / bound if np.isfinite(diff) else np.inf
        delta = E_dev[a] - E0[a]
        eta = 2 * U * max(E0[a], E_dev[a])
        x = -mu_dev[a] * np.sqrt(tau_dev[a])
        if blocked and -6.01 < x < 26.01:
            eta += TABLE_VS_ROUTINE * E_dev[a]
        dA = delta * A[a]
        r = r - dA
        acc += U * (np.abs(r) + 2 * np.abs(dA)) + np.abs(A[a]) * eta
    return float(ratio.max()), np.flatnonzero(ratio > 1), np.array(tau_bad, dtype=np.int64)


def check_all(case, lam, mu, tau, E, V):
    """both checks; returns (ratio of (a): mean, variance; ratio of (b); list of what failed)"""
    ra_e, ra_v, bad_a = check_moments(mu, tau, E, V)
    rb, bad_b, tau_bad = check_steps(case, lam, mu, tau, E)
    fails = []
    order = order_of(case)
    if bad_a.size:
        fails.append("(a) moments: %d entries, first (k, l) %s" % (bad_a.size, [divmod(int(a), case.L) for a in bad_a[:4]]))
    if tau_bad.size:
        fails.append("(b) tauS not exact at steps %s" % tau_bad[:4].tolist())
    if bad_b.size:
        fails.append("(b) muS beyond its bound at steps %s (entries %s)" % (bad_b[:4].tolist(), order[bad_b[:4]].tolist()))
    return (ra_e, ra_v, rb), fails


# ------------------------------------------------------------------ the kernels in NumPy fp32 (the CPU side)
def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def routine():
    """(the generator module of the fp32 routine, its three committed coefficient lists, the table's generator, the committed table)"""
    g = _load("gen_tn_moments_f32_coeffs")
    txt = open(os.path.join(ROOT, "bnmtf_amd", "csrc", "tn_moments_f32_coeffs.h")).read()
    P = []
    for name in ("kTnF32R", "kTnF32H", "kTnF32E"):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", txt, re.S).group(1)
        P.append([float(v.strip().rstrip("f")) for v in body.replace("\n", " ").split(",") if v.strip()])
    gt = _load("gen_tn_mean_table")
    rows = re.findall(r"^\s*\{(.*?)\},\s*$", open(os.path.join(ROOT, "bnmtf_amd", "csrc", "tn_mean_table.h")).read(), re.M)
    tab = np.array([[float(v.strip().rstrip("f")) for v in r.split(",")] for r in rows], dtype=np.float32)
    assert tab.shape == (NSEG, 6) and (gt.X0, gt.W, gt.NSEG) == (X0, WSEG, NSEG)
    return g, P, gt, tab


def moments_f32(mu, tau_p, no_fallback=False):
    g, P, _, _ = routine()
    mu, tau_p = np.atleast_1d(np.asarray(mu, np.float32)), np.atleast_1d(np.asarray(tau_p, np.float32))
    e, v = g.moments_f32(mu, tau_p, *P)
    if no_fallback:                                   # (FAULT: the routine's x > 0 polynomials where the -30 sigma fall-back belongs)
        with np.errstate(all="ignore"):
            sig = np.float32(1) / np.sqrt(tau_p)
            ax = np.abs(-mu * (tau_p * sig))
            sv = (ax - np.float32(g.A)) / (ax + np.float32(g.A))
            e2 = sig * (g.horner32(P[0], sv) / (np.float32(1) + ax))
            v2 = sig * sig * (g.horner32(P[1], sv) / (np.float32(1) + ax * ax))
        far = mu < np.float32(-30) * sig
        return np.where(far, e2, e).astype(np.float32), np.where(far, v2, v).astype(np.float32)
    return e, v


def table_mean(x, shift=0):
    """r(x) out of the committed table as the project's evaluator reads it (shift: FAULT, the neighbouring segment's coefficients)"""
    _, _, gt, tab = routine()
    return gt.eval_f32(np.roll(tab, -shift, axis=0) if shift else tab, np.atleast_1d(np.asarray(x, np.float32)))


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


f32 = np.float32

# one fault at a time; each must fail a check on every case it can occur on (fault_applies)
FAULTS = ("skip_fold", "skip_last", "drop_tail_step", "wrong_row", "stale_lds", "segment_off_by_one", "fast_to_minus_4",
          "no_fallback", "stored_from_table")


def fault_applies(fault, case):
    """Can the fault occur on this case?  (skip_last: the pass ends one step early and the last entry keeps the values that were
    pushed -- dropping only the last step's in-wave delta changes nothing, no lane is behind it; drop_tail_step: the in-wave delta
    of the partial block's second-to-last step is lost, what a wrong tail of the x4 loop does.)"""
    st = steered(case)
    n, blocked, nblk = case.n, case.kernel == "blocked", (case.n + 63) // 64
    reg = regime(st.x)
    return {
        "skip_fold": blocked and nblk >= 2,
        "skip_last": True,
        "drop_tail_step": blocked and n % 64 >= 2,
        "wrong_row": n >= 2,
        "stale_lds": blocked and nblk >= 4,
        "segment_off_by_one": blocked and bool(((reg[:-1] == "neg") | (reg[:-1] == "tab")).any()),
        "fast_to_minus_4": bool(((st.x > -4.6) & (st.x <= -4.0)).any()),
        "no_fallback": bool((st.x > 30 + 0.05).any()),
        "stored_from_table": blocked and bool(((st.x >= 26.05) & (st.x < 29.95)).any()),
    }[fault]


def _inputs(case, lam, order=None):
    _, _, s = system(case.K, case.L)
    order = order_of(case) if order is None else np.asarray(order)
    A = s.A.astype(np.float32)
    return s, order, A, residual0(s).astype(np.float32), s.S.reshape(-1).astype(np.float32), np.asarray(lam, np.float32).reshape(-1)


def chain_steps_f32(case, lam, fault=None, order=None):
    """ssys_chain_vb_kernel: thread t owns entry t; returns (mu, tauS, E, var) per entry (untouched entries: the pushed ones)"""
    s, order, A, r, e, lam = _inputs(case, lam, order)
    n2, tau = case.n, f32(case.tau)
    if fault == "skip_last":
        order = order[:-1]
    aaa = np.diag(A).copy()
    tau_p = (tau * aaa).astype(np.float32)
    inv_tp = (f32(1) / tau_p).astype(np.float32)
    sig = (f32(1) / np.sqrt(tau_p)).astype(np.float32)
    xs = (tau_p * sig).astype(np.float32)
    mu_out, tau_out, var_out = np.ones(n2, np.float32), np.ones(n2, np.float32), np.ones(n2, np.float32)
    cut = f32(-4.0) if fault == "fast_to_minus_4" else f32(-6.0)
    for i, a in enumerate(order):
        numer = fma32(tau, fma32(aaa[a], e[a], r[a]), -lam[a])
        mu = f32(numer * inv_tp[a])
        x = f32(-mu * xs[a])
        if x <= cut:
            enew = f32(sig[a] * -x)
        else:
            enew = moments_f32(mu, tau_p[a], fault == "no_fallback")[0][0]
        d = f32(enew - e[a])
        e[a] = enew
        row = A[order[i + 1] if i + 1 < len(order) else order[i - 1]] if fault == "wrong_row" and i == 0 else A[a]
        r = fma32(-d, row, r)
        mu_out[a], tau_out[a] = mu, tau_p[a]
    done = np.zeros(n2, bool); done[order] = True
    var_out[done] = moments_f32(mu_out[done], tau_out[done], fault == "no_fallback")[1]
    return mu_out, tau_out, e, var_out


def chain_blocked_f32(case, lam, fault=None):
    """ssys_chain_vb_blocked_kernel: lane p owns STEP p; nm = fma(tau, r, c); inside a wave the delta of a slow step comes from the
    table (the routine beyond it), the stored E and the delta the other waves fold from tn_moments_f32."""
    s, order, A, r0, e0, lam = _inputs(case, lam)
    n, tau = case.n, f32(case.tau)
    nblk = (n + 63) // 64
    Ap = A[np.ix_(order, order)]
    r, e_old, lam = r0[order].copy(), e0[order], lam[order]
    aaa = np.diag(Ap).copy()
    tau_p = (tau * aaa).astype(np.float32)
    inv_tp = (f32(1) / tau_p).astype(np.float32)
    sig = (f32(1) / np.sqrt(tau_p)).astype(np.float32)
    xs = (tau_p * sig).astype(np.float32)
    c = fma32(tau * aaa, e_old, -lam)
    hh = (inv_tp * xs).astype(np.float32)
    g = (hh * sig).astype(np.float32)
    thr = ((f32(4.0) if fault == "fast_to_minus_4" else f32(6.0)) / hh).astype(np.float32)
    nofb = fault == "no_fallback"
    mu_out, E_out, var_out = np.ones(n, np.float32), e_old.copy(), np.ones(n, np.float32)
    n_on = n - 1 if fault == "skip_last" else n
    table_fault_at = None
    for blk in range(nblk):
        lo, hi = 64 * blk, min(n, 64 * blk + 64)
        src = lo - 3 * 64 if fault == "stale_lds" and blk == 3 else lo             # the diagonal block read out of LDS
        for p in range(lo, hi):
            if p + 1 >= hi:
                break                                                              # (no lane behind the block's last step)
            if fault == "drop_tail_step" and blk == nblk - 1 and p == hi - 2:
                continue
            nm = fma32(tau, r[p], c[p])
            if nm >= thr[p]:
                d = fma32(nm, g[p], -e_old[p])
            else:
                x = f32(-nm * hh[p])
                if x < f32(26.0):
                    en = f32(sig[p] * table_mean(x, 1 if fault == "segment_off_by_one" else 0)[0])
                else:
                    en = moments_f32(f32(nm * inv_tp[p]), tau_p[p], nofb)[0][0]
                d = f32(en - e_old[p])
            row = Ap[src + (p - lo), src + (p - lo) + 1:src + (hi - lo)]
            if fault == "wrong_row" and p == 0:
                row = Ap[1, p + 1:hi]
            r[p + 1:hi] = fma32(-d, row, r[p + 1:hi])
        # behind the block: every lane's mu, E and delta once more from its frozen residual
        sl = slice(lo, hi)
        nm = fma32(tau, r[sl], c[sl])
        mu = (nm * inv_tp[sl]).astype(np.float32)
        ef, vf = moments_f32(mu, tau_p[sl], nofb)
        if fault == "stored_from_table" and table_fault_at is None:
            x = (-nm * hh[sl]).astype(np.float32)
            far = np.flatnonzero((x >= 26.0) & (x < 30.0))
            if far.size:
                table_fault_at = lo + far[0]
                ef[far[0]] = f32(sig[sl][far[0]] * table_mean(x[far[0]])[0])
        fast = nm >= thr[sl]
        en = np.where(fast, (nm * g[sl]).astype(np.float32), ef).astype(np.float32)
        dl = np.where(fast, fma32(nm, g[sl], -e_old[sl]), (ef - e_old[sl]).astype(np.float32)).astype(np.float32)
        on = np.arange(lo, hi) < n_on
        dl = np.where(on, dl, f32(0))
        mu_out[sl] = np.where(on, mu, mu_out[sl]); E_out[sl] = np.where(on, en, E_out[sl]); var_out[sl] = np.where(on, vf, var_out[sl])
        # the waves of later blocks fold the 64 deltas, one FMA each, in the block's order
        for j in range(hi - lo):
            first = hi + 64 if fault == "skip_fold" and blk == 0 else hi          # (block 0's deltas never reach wave 1)
            row = Ap[1 if fault == "wrong_row" and lo + j == 0 else lo + j]
            r[hi:] = np.concatenate([r[hi:first], fma32(-dl[j], row[first:], r[first:])])
    out = [np.ones(n, np.float32) for _ in range(4)]
    tau_o = np.where(np.arange(n) < n_on, tau_p, f32(1)).astype(np.float32)
    for dst, src_ in zip(out, (mu_out, tau_o, E_out, var_out)):
        dst[order] = src_
    return tuple(out)


def chain_f32(case, lam, fault=None):
    return (chain_blocked_f32 if case.kernel == "blocked" else chain_steps_f32)(case, lam, fault)


# ------------------------------------------------------------------ (c) the single-step hook over a grid of x
HOOK_SHAPE = (3, 5)
HOOK_X = (-40.0, -12.0, -6.0 - 1e-3, -6.0 + 1e-3, -1e-3, 0.0, 1e-3, 3.0, 12.0, 25.9, 26.1, 29.9, 30.1, 35.0)
HOOK_TAUS = (2.0 ** -21, 2.0 ** -14, 2.0 ** -7, 1.0, 2.0 ** 5, 2.0 ** 10)      # A_aa ~ 2^10..2^11 on HOOK_SHAPE: tauS from below 2^-10 to above 2^20


class HookCase:
    def __init__(self, tau):
        (self.K, self.L), self.tau = HOOK_SHAPE, tau
        self.n = self.K * self.L


def hook_f32(tau, lam):
    """the hook in NumPy fp32: one step per entry, each from the pushed state"""
    n = HOOK_SHAPE[0] * HOOK_SHAPE[1]
    steps = [chain_steps_f32(HookCase(tau), lam, order=[a]) for a in range(n)]
    return tuple(np.array([steps[a][q][a] for a in range(n)]) for q in range(4))


def hook_lambda(tau):
    """lambdaS for update_S + update_exp_S of each entry from the SAME pushed state: entry a is steered to HOOK_X[a mod 14].
    Returns (lambdaS as fp32 values, the x each entry gets in fp64, tauS)."""
    K, L = HOOK_SHAPE
    _, _, s = system(K, L)
    E0 = s.S.reshape(-1).astype(np.float64)
    r0, d = residual0(s), np.diag(s.A)
    xt = np.array([HOOK_X[a % len(HOOK_X)] for a in range(K * L)])
    sa = r0 + d * E0
    lam = (tau * sa + xt * np.sqrt(tau * d)).astype(np.float32)
    mu = (tau * sa - lam.astype(np.float64)) / (tau * d)
    return lam.reshape(K, L), -mu * np.sqrt(tau * d), tau * d
