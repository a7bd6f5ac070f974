"""Explain every truncated-normal draw of a Gibbs run by the oracle's candidate sequence (NumPy fp64, no GPU).

The sampler is a first-accepted-candidate rule (oracle/rng.py): the draw of (element, column, iteration, stream) walks the Philox
candidates c = 0, 1, 2, ... and takes the first one its acceptance test lets through.  A device chain compared with an oracle
chain that runs on its own decouples at the first accept decision that rounds the other way, so such tests allow a share of
mismatches -- the same size as the share of draws that go past a kernel's first candidate batch.  Here nothing cascades: every
draw is conditioned on the device's OWN samples.  Given sample t-1 and the part of sample t already drawn, (mu, tau_p) of a
single draw is an fp64 function of numbers the run returned, and the draw

  * must be the value of a candidate the oracle's sequence ADMITS: any candidate that is not surely rejected, up to and
    including the first one that is surely accepted;
  * where no decision is near a rounding boundary that set has ONE element: the candidate the oracle accepts.

Tolerance model (derived, not fitted; a draw outside it is a finding -- name the fp32 term it misses here before widening it):

  dmu   bound the conditional-parameter tests hold the device's mu to (test_bnmf_gibbs_gpu.py: 2e-5 scale + 1e-6 with scale the
        absolute-value sum of the cancelling terms; test_bnmtf_gibbs_gpu.py: 3e-5 sc + 1e-6 for F, S and G)
  da    uncertainty of the standardised bound a = -mu sqrt(tau_p):  dmu sqrt(tau_p) + 2e-6 |a| + HW
        (2e-6: the tests' relative bound on tau_p; HW = 1e-4 stands for the hardware log / cos / sqrt / rcp, in standardised
        units -- hundreds of fp32 ulps at |z| ~ 1)
  normal regime  (a < 0.25):  z = sqrt(-2 ln u1) cos(2 pi u2), accept z >= a, x = mu + z / sqrt(tau_p)
        marginal: |z - a| <= da            value: dmu + HW / sqrt(tau_p) + 1e-5 |x|
  tail regime    (a >= 0.25): s = sqrt(a^2 + 4), d = 2 / (s + a), lam = a + d, e = -ln u1 / lam, accept u2 <= exp(-(e - d)^2 / 2),
        i.e. |e - d| <= sqrt(-2 ln u2) (the form the chip kernels test, sweep_common.h), x = e / sqrt(tau_p)
        d(e - d)/da = -(e - d) / s and de/da = -e / s, so
        marginal: |sqrt(-2 ln u2) - |e - d|| <= |e - d| da / s + HW      value: (e da / s + HW) / sqrt(tau_p) + 1e-5 |x|
  regime choice  |a - 0.25| <= da admits the walks of both regimes
  tau_p <= 0 or a non-finite a admits only 0; a negative or non-finite candidate value maps to 0 (tn_guard).
"""
import numpy as np

from oracle import rng

HW = 1e-4
REL_TAU = 2e-6
REL_X = 1e-5
NORMAL, TAIL = 0, 1


def explain_tn(x, mu, tau_p, dmu, elem, col, it, stream, seed, max_cand=1024, trace=None):
    """Vectorised over the draws of one column.  Returns a dict of arrays, one entry per draw:
    explained, n_adm (size of the admissible set), cand (matched candidate index, -1 for the guarded 0), regime (of the match),
    err (|x - x_c| in units of its tolerance, for the best admissible candidate), a, da.
    trace: a list that receives (draw, regime, candidate, value, 'accept' | 'marginal') for every admissible candidate."""
    x, mu, tau_p, dmu, elem, col = np.broadcast_arrays(
        np.asarray(x, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(tau_p, dtype=np.float64),
        np.asarray(dmu, dtype=np.float64), np.asarray(elem), np.asarray(col))
    x = x.ravel(); mu = mu.ravel(); tau_p = tau_p.ravel(); dmu = dmu.ravel()
    elem = elem.ravel().astype(np.uint64); col = col.ravel().astype(np.uint64)
    n = x.size
    n_adm = np.zeros(n, dtype=np.int64)
    cand = np.full(n, -1, dtype=np.int64)
    regime = np.full(n, -1, dtype=np.int64)
    err = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        live = tau_p > 0.0
        rt = np.sqrt(np.where(live, tau_p, 1.0))
        a = -mu * rt
        live &= np.isfinite(a)
        da = dmu * rt + REL_TAU * np.abs(a) + HW
    dead = ~live
    n_adm[dead] = 1
    err[dead] = np.where(x[dead] == 0.0, 0.0, np.inf)
    if trace is not None:
        trace.extend((int(i), -1, -1, 0.0, "accept") for i in np.nonzero(dead)[0])
    for reg in (NORMAL, TAIL):
        todo = np.nonzero(live & ((a < rng.TN_A0 + da) if reg == NORMAL else (a >= rng.TN_A0 - da)))[0]
        c = 0
        while todo.size and c < max_cand:
            r0, r1, _, _ = rng.philox4x32_10(elem[todo], col[todo], it, int(stream) + 16 * c, seed)
            u1 = rng.u23(r0); u2 = rng.u23(r1)
            nl = -np.log(u1)
            at, dat, rtt = a[todo], da[todo], rt[todo]
            with np.errstate(all="ignore"):
                if reg == NORMAL:
                    z = np.sqrt(2.0 * nl) * np.cos(rng.TWO_PI * u2)
                    m = z - at
                    tol_m = dat
                    xc = mu[todo] + z / rtt
                    vtol = dmu[todo] + HW / rtt
                else:
                    s = np.sqrt(at * at + 4.0)
                    d = 2.0 / (s + at)
                    e = nl / (at + d)
                    t = np.abs(e - d)
                    m = np.sqrt(-2.0 * np.log(u2)) - t
                    tol_m = t * dat / s + HW
                    xc = e / rtt
                    vtol = (e * dat / s + HW) / rtt
            xc = np.where(np.isfinite(xc) & (xc >= 0.0), xc, 0.0)
            vtol = vtol + REL_X * np.abs(xc)
            sure_acc = m > tol_m
            adm = ~(m < -tol_m)
            ia = todo[adm]
            n_adm[ia] += 1
            ev = np.abs(x[ia] - xc[adm]) / vtol[adm]
            better = ev < err[ia]
            ib = ia[better]
            err[ib] = ev[better]; cand[ib] = c; regime[ib] = reg
            if trace is not None:
                trace.extend((int(i), reg, c, float(v), "accept" if sa else "marginal")
                             for i, v, sa in zip(ia, xc[adm], sure_acc[adm]))
            todo = todo[~sure_acc]
            c += 1
        n_adm[todo] += 1                         # the walk was cut short: what lies beyond is not known to be excluded
    return dict(explained=err <= 1.0, n_adm=n_adm, cand=cand, regime=regime, err=err, a=a, da=da, mu=mu, tau_p=tau_p, dmu=dmu)


class Explained:
    """Per-draw records of one run, over its factors, iterations and columns."""

    def __init__(self, seed=0):
        self.seed = seed
        self._parts = []
        self.tau_rel = []            # |tau - expected| / expected, one per iteration
        self._cat = None

    def add(self, factor, it, elem, col, x, res, stream=0):
        n = np.size(x)
        part = dict(res)
        part["factor"] = np.full(n, factor)
        part["stream"] = np.full(n, stream, dtype=np.int64)
        part["it"] = np.full(n, it, dtype=np.int64)
        part["elem"] = np.broadcast_to(np.asarray(elem, dtype=np.int64), (n,)).copy()
        part["col"] = np.broadcast_to(np.asarray(col, dtype=np.int64), (n,)).copy()
        part["x"] = np.asarray(x, dtype=np.float64).ravel()
        self._parts.append(part)
        self._cat = None

    def __getitem__(self, key):
        if self._cat is None:
            self._cat = {k: np.concatenate([p[k] for p in self._parts]) for k in self._parts[0]}
        return self._cat[key]

    @property
    def draws(self):
        return int(self["x"].size)

    @property
    def unexplained(self):
        return int((~self["explained"]).sum())

    @property
    def ambiguous(self):
        return int((self["n_adm"] > 1).sum())

    def unique(self, factors=None):
        """mask of the explained draws whose admissible set has one element: the oracle's accepted candidate"""
        m = self["explained"] & (self["n_adm"] == 1)
        if factors is not None:
            m &= np.isin(self["factor"], factors)
        return m

    def past(self, index, factors=None, cols=None):
        """uniquely explained draws whose accepted candidate index is >= index"""
        m = self.unique(factors) & (self["cand"] >= index)
        if cols is not None:
            m &= (self["col"] >= cols[0]) & (self["col"] < cols[1])
        return int(m.sum())

    def regime_shares(self, factors=None):
        u = self.unique(factors) & (self["regime"] >= 0)
        n = max(1, int(u.sum()))
        return [int((u & (self["regime"] == r)).sum()) / float(n) for r in (NORMAL, TAIL)]

    def offenders(self, limit=10):
        """the first unexplained draws: factor, iteration, element, column, device value, a, da and the admissible candidates
        (regime, index, value, surely accepted or marginal)"""
        out = []
        for i in np.nonzero(~self["explained"])[0][:limit]:
            o = dict((k, self[k][i].item()) for k in ("factor", "it", "elem", "col", "x", "a", "da", "mu", "tau_p", "dmu", "n_adm"))
            tr = []
            explain_tn(o["x"], o["mu"], o["tau_p"], o["dmu"], o["elem"], o["col"], o["it"], int(self["stream"][i]), self.seed, trace=tr)
            o["admissible"] = [(("normal", "tail", "guard")[t[1]], t[2], t[3], t[4]) for t in tr]
            out.append(o)
        return out

    def summary(self):
        """what profiles/draws_explained.json records per case"""
        ok = self["explained"] & (self["cand"] >= 0)
        hist = np.bincount(self["cand"][self.unique() & (self["cand"] >= 0)]).tolist()
        out = dict(draws=self.draws, unexplained=self.unexplained, ambiguous_share=self.ambiguous / float(max(1, self.draws)),
                   unique=int(self.unique().sum()), accepted_index_histogram=hist,
                   tau_rel_max=float(max(self.tau_rel)) if self.tau_rel else None)
        for r, name in ((NORMAL, "normal"), (TAIL, "tail")):
            e = self["err"][ok & (self["regime"] == r)]
            out["err_max_" + name] = float(e.max()) if e.size else None
            out["err_p999_" + name] = float(np.percentile(e, 99.9)) if e.size else None
        return out


def gamma_unit(shape, it, seed):
    """the Gamma(shape, 1) variate of iteration `it` (oracle/rng.gamma_draw with rate 1): tau = gamma_unit / beta_s"""
    return rng.gamma_draw(shape, 1.0, it, seed)


TAU_REL = 2e-5          # the suite's bound for the Gram-identity SSE (test_bnmf_gibbs_gpu.py), here without a chain in between


def _factor_pass(out, name, X, Y, E, Mm, MR, lam, tau, new, elem0, col0, it, stream, seed, c_mu, check=True):
    """Columns of X (rows of E) given Y, conditioned on `new`, the device's sample of X: column k sees new[:, :k] and X[:, k:].
    E = Mm * (R - X Y^T) is kept current by rank-one updates.  dmu = c_mu * scale / tau_p + 1e-6 with the absolute-value sums of
    test_bnmf_gibbs_gpu._mu_scale."""
    n, K = X.shape
    elem = np.arange(n) + elem0
    for k in range(K):
        y = Y[:, k]
        g = Mm @ (y * y)
        tau_p = tau * g
        numer = -lam[:, k] + tau * (E @ y + X[:, k] * g)
        with np.errstate(all="ignore"):
            mu = numer / tau_p
            scale = tau * (MR @ np.abs(y) + np.abs(X) @ np.abs(Y.T @ y))
            dmu = np.where(tau_p > 0, c_mu * scale / tau_p, 0.0) + (1e-6 if c_mu else 0.0)
        x = new[:, k].astype(np.float64)
        if check:
            out.add(name, it, elem, col0 + k, x, explain_tn(x, mu, tau_p, dmu, elem, col0 + k, it, stream, seed), stream)
        E -= Mm * np.outer(x - X[:, k], y)
        X[:, k] = x


def explain_bnmf_run(R, M, lambdaU, lambdaV, alpha, beta, seed, init_state, all_U, all_V, all_tau, it0=0, col0=0, elem0=0, c_mu=2e-5,
                     iterations=None):
    """Every U and V draw and every tau of a two-factor run.  init_state = (U, V, tau) the run started from (as the device holds
    it: fp32 factors); all_U[t], all_V[t], all_tau[t] its samples.  it0: the iteration word of sample 0; col0: the column word of
    column 0 (a column block explained by itself); elem0: the element word of row / column 0.  c_mu = 0: the floor terms only."""
    R = np.asarray(R, dtype=np.float64); M = np.asarray(M, dtype=np.float64)
    I, J = R.shape
    K = np.asarray(all_U[0]).shape[1]
    lamU = np.broadcast_to(np.asarray(lambdaU, dtype=np.float64), (I, K)); lamV = np.broadcast_to(np.asarray(lambdaV, dtype=np.float64), (J, K))
    U = np.array(init_state[0], dtype=np.float64); V = np.array(init_state[1], dtype=np.float64); tau = float(init_state[2])
    MR = M * np.abs(R); Mt = np.ascontiguousarray(M.T); MRt = np.ascontiguousarray(MR.T)
    alpha_s = alpha + M.sum() / 2.0
    out = Explained(seed)
    for t in (range(len(all_tau)) if iterations is None else iterations):
        it = it0 + t
        if t > 0:
            U = np.array(all_U[t - 1], dtype=np.float64); V = np.array(all_V[t - 1], dtype=np.float64); tau = float(all_tau[t - 1])
        E = M * (R - U @ V.T)
        _factor_pass(out, "U", U, V, E, M, MR, lamU, tau, np.asarray(all_U[t]), elem0, col0, it, rng.STREAM_ROWS, seed, c_mu)
        Et = np.ascontiguousarray(E.T)
        _factor_pass(out, "V", V, U, Et, Mt, MRt, lamV, tau, np.asarray(all_V[t]), elem0, col0, it, rng.STREAM_COLS, seed, c_mu)
        expected = gamma_unit(alpha_s, it, seed) / (beta + 0.5 * (Et * Et).sum())
        out.tau_rel.append(abs(float(all_tau[t]) - expected) / expected)
    return out


def explain_bnmtf_run(R, M, lambdaF, lambdaS, lambdaG, alpha, beta, seed, init_state, all_F, all_S, all_G, all_tau, it0=0, c_mu=3e-5):
    """Every F, S and G draw and every tau of a tri-factorisation run (F columns, S row-major, G columns: bnmtf_gibbs_optimised.py
    :152-167).  dmu = c_mu * sc / tau_p + 1e-6 with sc of test_bnmtf_gibbs_gpu.py:30-44: the cancelling terms are |R| + |F||S||G|^T
    against the column's regressor."""
    R = np.asarray(R, dtype=np.float64); M = np.asarray(M, dtype=np.float64)
    I, J = R.shape
    K, L = np.asarray(all_S[0]).shape
    lamF = np.broadcast_to(np.asarray(lambdaF, dtype=np.float64), (I, K)); lamS = np.broadcast_to(np.asarray(lambdaS, dtype=np.float64), (K, L))
    lamG = np.broadcast_to(np.asarray(lambdaG, dtype=np.float64), (J, L))
    F, S, G = (np.array(a, dtype=np.float64) for a in init_state[:3]); tau = float(init_state[3])
    aR = np.abs(R)
    alpha_s = alpha + M.sum() / 2.0
    floor = 1e-6 if c_mu else 0.0
    out = Explained(seed)
    rows = np.arange(I); cols = np.arange(J)
    for t in range(len(all_tau)):
        it = it0 + t
        if t > 0:
            F, S, G, tau = (np.array(all_F[t - 1], dtype=np.float64), np.array(all_S[t - 1], dtype=np.float64),
                            np.array(all_G[t - 1], dtype=np.float64), float(all_tau[t - 1]))
        E = M * (R - F @ S @ G.T)
        P = np.abs(F) @ np.abs(S) @ np.abs(G).T
        SG = S @ G.T                                   # K x J
        for k in range(K):
            sg = SG[k]
            g = M @ (sg * sg)
            tau_p = tau * g
            with np.errstate(all="ignore"):
                mu = (-lamF[:, k] + tau * (E @ sg + F[:, k] * g)) / tau_p
                dmu = np.where(tau_p > 0, c_mu * tau * ((M * (aR + P)) @ np.abs(sg)) / tau_p, 0.0) + floor
            x = np.asarray(all_F[t])[:, k].astype(np.float64)
            out.add("F", it, rows, k, x, explain_tn(x, mu, tau_p, dmu, rows, k, it, rng.STREAM_ROWS, seed), rng.STREAM_ROWS)
            E -= M * np.outer(x - F[:, k], sg)
            P += np.outer(np.abs(x) - np.abs(F[:, k]), np.abs(S[k]) @ np.abs(G).T)
            F[:, k] = x
        # S, row-major: the conditionals in sequence (each sees the device's new entries before it), then one vectorised walk
        Snew = np.asarray(all_S[t], dtype=np.float64)
        mus = np.zeros(K * L); tps = np.zeros(K * L); dmus = np.zeros(K * L)
        aF = np.abs(F); aG = np.abs(G)
        for k in range(K):
            for l in range(L):
                fg = np.outer(F[:, k], G[:, l])
                mfg = M * fg
                g = float((mfg * fg).sum())
                tau_p = tau * g
                e = k * L + l
                tps[e] = tau_p
                if tau_p > 0:
                    mus[e] = (-lamS[k, l] + tau * (float((E * fg).sum()) + S[k, l] * g)) / tau_p
                    dmus[e] = c_mu * tau * float(((aR + P) * np.abs(mfg)).sum()) / tau_p
                x = Snew[k, l]
                E -= (x - S[k, l]) * mfg
                P += (abs(x) - abs(S[k, l])) * np.outer(aF[:, k], aG[:, l])
                S[k, l] = x
        words = np.arange(K * L)
        out.add("S", it, 0, words, Snew.ravel(), explain_tn(Snew.ravel(), mus, tps, dmus + floor, 0, words, it, rng.STREAM_S, seed), rng.STREAM_S)
        FS = F @ S                                     # I x L
        for l in range(L):
            fs = FS[:, l]
            g = (fs * fs) @ M
            tau_p = tau * g
            with np.errstate(all="ignore"):
                mu = (-lamG[:, l] + tau * (fs @ E + G[:, l] * g)) / tau_p
                dmu = np.where(tau_p > 0, c_mu * tau * (np.abs(fs) @ (M * (aR + P))) / tau_p, 0.0) + floor
            x = np.asarray(all_G[t])[:, l].astype(np.float64)
            out.add("G", it, cols, l, x, explain_tn(x, mu, tau_p, dmu, cols, l, it, rng.STREAM_COLS, seed), rng.STREAM_COLS)
            E -= M * np.outer(fs, x - G[:, l])
            P += np.outer(np.abs(F) @ np.abs(S[:, l]), np.abs(x) - np.abs(G[:, l]))
            G[:, l] = x
        expected = gamma_unit(alpha_s, it, seed) / (beta + 0.5 * (E * E).sum())
        out.tau_rel.append(abs(float(all_tau[t]) - expected) / expected)
    return out


# ---- steered inputs: prior rates that put a = -mu sqrt(tau_p) of the first sweep's draws on chosen targets
TARGETS = (-3.0, -1.0, 0.0, 0.26, 0.3, 1.0, 5.0, 30.0)
LAMBDA_FLOOR = 1e-3


def draw_targets(rs, n):
    """half uniform in [0.10, 0.24] (acceptance ~ 0.42: long candidate walks), the rest from TARGETS"""
    t = rs.uniform(0.10, 0.24, size=n)
    other = rs.rand(n) < 0.5
    t[other] = np.asarray(TARGETS)[rs.randint(len(TARGETS), size=n)][other]
    return t


def _steer(rs, tauN, tau_p, dmu):
    """lambda = tau * numer + a_target sqrt(tau_p), floored; targets kept at least 10 da from the regime switch"""
    rt = np.sqrt(np.maximum(tau_p, 0.0))
    at = draw_targets(rs, np.size(tauN))
    da = dmu * rt + REL_TAU * np.abs(at) + HW
    near = np.abs(at - rng.TN_A0) < 10.0 * da
    at = np.where(near, rng.TN_A0 + np.where(at < rng.TN_A0, -10.0, 10.0) * da, at)
    return np.maximum(tauN + at * rt, LAMBDA_FLOOR)


def steer_lambda(R, M, init_state, seed, rs, c_mu=None):
    """Runs the oracle's first sweep column by column from init_state -- (U, V, tau) or (F, S, G, tau) -- and sets every column's
    prior rates just before it is drawn.  Returns (lambdaU, lambdaV) or (lambdaF, lambdaS, lambdaG).  A device chain that leaves
    the oracle's after a flipped accept only moves those rows' a; the explainer conditions on the device's state and does not care."""
    R = np.asarray(R, dtype=np.float64); M = np.asarray(M, dtype=np.float64)
    if len(init_state) == 3:
        c_mu = 2e-5 if c_mu is None else c_mu
        U, V = (np.array(a, dtype=np.float64) for a in init_state[:2]); tau = float(init_state[2])
        MR = M * np.abs(R)
        lams = []
        E = M * (R - U @ V.T)
        for X, Y, Mm, MRm, stream, tr in ((U, V, M, MR, rng.STREAM_ROWS, False), (V, U, M.T, MR.T, rng.STREAM_COLS, True)):
            lam = np.zeros(X.shape)
            elem = np.arange(X.shape[0])
            for k in range(X.shape[1]):
                y = Y[:, k]
                g = Mm @ (y * y)
                tau_p = tau * g
                tauN = tau * ((E.T if tr else E) @ y + X[:, k] * g)
                with np.errstate(all="ignore"):
                    dmu = np.where(tau_p > 0, c_mu * tau * (MRm @ np.abs(y) + np.abs(X) @ np.abs(Y.T @ y)) / tau_p, 0.0) + 1e-6
                    lam[:, k] = _steer(rs, tauN, tau_p, dmu)
                    x = rng.tn_draw((tauN - lam[:, k]) / tau_p, tau_p, elem, k, 0, stream, seed)
                d = np.outer(x - X[:, k], y)
                E -= M * (d.T if tr else d)
                X[:, k] = x
            lams.append(lam)
        return tuple(lams)
    c_mu = 3e-5 if c_mu is None else c_mu
    F, S, G = (np.array(a, dtype=np.float64) for a in init_state[:3]); tau = float(init_state[3])
    I, J = R.shape; K, L = S.shape
    aR = np.abs(R)
    lamF = np.zeros((I, K)); lamS = np.zeros((K, L)); lamG = np.zeros((J, L))
    E = M * (R - F @ S @ G.T)
    for k in range(K):
        sg = S[k] @ G.T
        g = M @ (sg * sg); tau_p = tau * g
        tauN = tau * (E @ sg + F[:, k] * g)
        P = np.abs(F) @ np.abs(S) @ np.abs(G).T
        with np.errstate(all="ignore"):
            dmu = np.where(tau_p > 0, c_mu * tau * ((M * (aR + P)) @ np.abs(sg)) / tau_p, 0.0) + 1e-6
            lamF[:, k] = _steer(rs, tauN, tau_p, dmu)
            x = rng.tn_draw((tauN - lamF[:, k]) / tau_p, tau_p, np.arange(I), k, 0, rng.STREAM_ROWS, seed)
        E -= M * np.outer(x - F[:, k], sg)
        F[:, k] = x
    for k in range(K):
        for l in range(L):
            fg = np.outer(F[:, k], G[:, l]); mfg = M * fg
            g = float((mfg * fg).sum()); tau_p = tau * g
            tauN = tau * (float((E * fg).sum()) + S[k, l] * g)
            P = np.abs(F) @ np.abs(S) @ np.abs(G).T
            dmu = (c_mu * tau * float(((aR + P) * np.abs(mfg)).sum()) / tau_p if tau_p > 0 else 0.0) + 1e-6
            lamS[k, l] = float(_steer(rs, np.array([tauN]), np.array([tau_p]), np.array([dmu]))[0])
            x = float(rng.tn_draw((tauN - lamS[k, l]) / tau_p if tau_p > 0 else 0.0, tau_p, 0, k * L + l, 0, rng.STREAM_S, seed))
            E -= (x - S[k, l]) * mfg
            S[k, l] = x
    for l in range(L):
        fs = F @ S[:, l]
        g = (fs * fs) @ M; tau_p = tau * g
        tauN = tau * (fs @ E + G[:, l] * g)
        P = np.abs(F) @ np.abs(S) @ np.abs(G).T
        with np.errstate(all="ignore"):
            dmu = np.where(tau_p > 0, c_mu * tau * (np.abs(fs) @ (M * (aR + P))) / tau_p, 0.0) + 1e-6
            lamG[:, l] = _steer(rs, tauN, tau_p, dmu)
            x = rng.tn_draw((tauN - lamG[:, l]) / tau_p, tau_p, np.arange(J), l, 0, rng.STREAM_COLS, seed)
        E -= M * np.outer(fs, x - G[:, l])
        G[:, l] = x
    return lamF, lamS, lamG
