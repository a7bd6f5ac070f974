"""Drop-in for code/models/bnmf_vb_optimised.py (class bnmf_vb_optimised): variational Bayes for
Bayesian NMF, with the column updates, TN moments and exp_square_diff evaluated by libbnmtf_hip.so.

    BNMF = bnmf_vb_optimised(R, M, K, priors)
    BNMF.initialise(init='exp', tauUV={})
    BNMF.run(iterations)
"""
import ctypes as C
import math

import numpy as np
import scipy.special

from . import _lib
from ._base import check_binary, check_rank, check_R_M, metrics_from_sums
from ._blocked import BLOCK, MAX_BLOCKS, VBColumnBlocks
from ._variational import Variational, q_names
from .distributions import gamma_expectation, gamma_expectation_log


class bnmf_vb_optimised(Variational):
    _FACTORS = ("U", "V")
    _NAMES = q_names(_FACTORS)
    _DENSE = {"set_state": "bnmf_vb_set_state", "get_state": "bnmf_vb_get_state", "run": "bnmf_vb_run", "update": "bnmf_vb_update",
              "exp_square_diff": "bnmf_vb_exp_square_diff", "run_many": "bnmf_vb_run_many", "set_tau": "bnmtf_set_tau"}
    _ONES_IN_ESD = tuple(n for n in _NAMES if n[:-1] in ("mu", "tau"))      # the test-suite sets exp / var only

    def __init__(self, R, M, K, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None):
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K = K
        check_R_M(self.R, self.M)
        check_rank("bnmf_vb_optimised", BLOCK * MAX_BLOCKS, K=self.K)
        (self.I, self.J) = self.R.shape
        self.size_Omega = self.M.sum()
        self._init_priors(priors, device, verbose, rank, world, comm_id)
        # ranks above 64 (the reference has no limit, :53-77): column blocks of at most 64, one device model each (_blocked.py)
        self._blocks = None
        if self.K > BLOCK:
            assert world == 1, "ranks above %d run on one GPU (column blocks: DESIGN.md section 8)" % BLOCK
            self._blocks = VBColumnBlocks(self, bnmf_vb_optimised)

    def _factor_shapes(self):
        return [(self.I, self.K), (self.J, self.K)]

    def close(self):
        if getattr(self, "_blocks", None) is not None:
            self._blocks.close()
        super(bnmf_vb_optimised, self).close()

    def _handle(self):
        if getattr(self, "_blocks", None) is not None:       # shape-only entry points: the first block's handle
            return self._blocks.handles()[0]
        return super(bnmf_vb_optimised, self)._handle()

    def _metric_sums(self, M_pred, A, S, B):
        if self._blocks is not None:
            if M_pred is not None:
                check_binary(M_pred, "M_pred")
            return self._blocks.metric_sums(M_pred, self.expU if A is None else A, self.expV if B is None else B)
        return super(bnmf_vb_optimised, self)._metric_sums(M_pred, A, S, B)

    def describe(self):
        if self._blocks is not None:
            self._blocks._prepare()
            return "column blocks %s: " % (self._blocks.ranges,) + " | ".join(ch.describe() for ch in self._blocks.children)
        return super(bnmf_vb_optimised, self).describe()

    def initialise(self, init='exp', tauUV={}):
        """bnmf_vb_optimised.py:93-117."""
        self.tauU = np.array(tauUV['tauU'], dtype=float) if 'tauU' in tauUV else np.ones((self.I, self.K))
        self.tauV = np.array(tauUV['tauV'], dtype=float) if 'tauV' in tauUV else np.ones((self.J, self.K))
        assert init in ['exp', 'random'], "Unrecognised init option for F,G: %s." % init
        self.muU, self.muV = 1. / self.lambdaU, 1. / self.lambdaV
        if init == 'random':
            self.muU = self._rng().exponential(scale=1.0 / self.lambdaU)
            self.muV = self._rng().exponential(scale=1.0 / self.lambdaV)
        self._initial_moments()            # (update_exp_U(k) / update_exp_V(k) of every column, :111-115)
        self.update_tau()
        self.update_exp_tau()

    def run(self, iterations, *, M_test=None):
        """:121-153.  all_elbo (the value the reference only prints) is kept as an extra attribute.  M_test: the held-out metrics
        of E[U] E[V]^T behind every iteration, in all_performances_test (see bnmf_gibbs_optimised.run)."""
        Mt = self._check_heldout(M_test)
        it = int(iterations)
        if self._blocks is not None:
            return self._run_blocked(it)
        self._run(it, Mt)

    def _run_device(self, it, exptau, perf, terms, times):
        """The device call of run(), either layout's."""
        _lib.check(self._entry("run")(self._handle(), it, _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times)))

    def _take_elbo_terms(self, terms):
        self.all_elbo_terms = terms
        self._all_elbo = None              # (all_elbo: finished from the terms when somebody reads it -- a model search reads the last state only)

    def _iteration_line(self, i, perf):
        return "Iteration %s. ELBO: %s. MSE: %s. R^2: %s. Rp: %s." % (i + 1, self.all_elbo[i], perf[i, 0], perf[i, 1], perf[i, 2])

    def _run_blocked(self, it):
        """run() of a model wider than 64 columns (_blocked.py): per iteration the blocks' half sweeps in turn (:134-141), then
        update_tau / update_exp_tau (:143-144) from the full-width exp_square_diff, the metrics and the ELBO (:146-150)."""
        import time
        blocks = self._blocks
        self._push()
        self.all_exp_tau, self.all_times, self.all_elbo = [], [], []
        self.all_performances = {'MSE': [], 'R^2': [], 'Rp': []}
        t0 = time.time()
        for i in range(it):
            blocks.sweep_both()
            self._pull()
            esd, s = blocks.esd(self.expU, self.expV)
            self.alpha_s = self.alpha + self.size_Omega / 2.0
            self.beta_s = self.beta + 0.5 * esd
            self.update_exp_tau()
            blocks.set_tau(self.exptau)
            self._device_state = (None, float(self.exptau), self._device_state[2])
            perf = metrics_from_sums(s)
            elbo = self._elbo_given_esd(esd)
            for m in ('MSE', 'R^2', 'Rp'):
                self.all_performances[m].append(perf[m])
            self.all_exp_tau.append(self.exptau); self.all_elbo.append(elbo); self.all_times.append(time.time() - t0)
            if self.verbose:
                print("Iteration %s. ELBO: %s. MSE: %s. R^2: %s. Rp: %s." % (i + 1, elbo, perf['MSE'], perf['R^2'], perf['Rp']))
        return

    def train(self, iterations, init_UV='random'):
        """:157-159, as written in the reference (initialise has no init_UV keyword -> TypeError there too)."""
        self.initialise(init_UV=init_UV)
        self.run(iterations=iterations)

    # -- ELBO -------------------------------------------------------------------
    def _elbo_scalar_part(self, esd, alpha_s, beta_s, exptau, explogtau, sums_u, sums_v):
        quad_u, lerfc_u, ltau_u, lamx_u = sums_u
        quad_v, lerfc_v, ltau_v, lamx_v = sums_v
        return self.size_Omega / 2. * (explogtau - math.log(2 * math.pi)) - exptau / 2. * esd \
            + np.log(self.lambdaU).sum() - lamx_u + np.log(self.lambdaV).sum() - lamx_v \
            + self.alpha * math.log(self.beta) - scipy.special.gammaln(self.alpha) \
            + (self.alpha - 1.) * explogtau - self.beta * exptau \
            - alpha_s * math.log(beta_s) + scipy.special.gammaln(alpha_s) \
            - (alpha_s - 1.) * explogtau + beta_s * exptau \
            - .5 * ltau_u + self.I * self.K / 2. * math.log(2 * math.pi) + lerfc_u + quad_u \
            - .5 * ltau_v + self.J * self.K / 2. * math.log(2 * math.pi) + lerfc_v + quad_v

    @property
    def all_elbo(self):
        """The ELBO of every iteration of the last run() (the value the reference prints, :148-150)."""
        if getattr(self, "_all_elbo", None) is None:
            terms = getattr(self, "all_elbo_terms", None)
            self._all_elbo = [] if terms is None else [self._elbo_from_terms(t) for t in terms]
        return self._all_elbo

    @all_elbo.setter
    def all_elbo(self, value):
        self._all_elbo = value

    def _elbo_from_terms(self, t):
        esd, beta_s = t[0], t[1]
        alpha_s = self.alpha + self.size_Omega / 2.0
        return self._elbo_scalar_part(esd, alpha_s, beta_s, gamma_expectation(alpha_s, beta_s),
                                      gamma_expectation_log(alpha_s, beta_s), t[2:6], t[6:10])

    def elbo(self):
        """:163-177 for the current attributes: exp_square_diff on the device, the O((I+J)K) sums on the host."""
        return self._elbo_given_esd(self.exp_square_diff())

    def _elbo_given_esd(self, esd):
        def sums(mu, tau, ex, var, lam):
            with np.errstate(all='ignore'):
                return ((tau / 2. * (var + (ex - mu) ** 2)).sum(),
                        np.log(0.5 * scipy.special.erfc(-mu * np.sqrt(tau) / math.sqrt(2))).sum(),
                        np.log(tau).sum(), (lam * ex).sum())
        return self._elbo_scalar_part(esd, self.alpha_s, self.beta_s, self.exptau, self.explogtau,
                                      sums(self.muU, self.tauU, self.expU, self.varU, self.lambdaU),
                                      sums(self.muV, self.tauV, self.expV, self.varV, self.lambdaV))

    # -- hooks and updates -------------------------------------------------------
    def masked_sums(self, which):
        """Hook (tests): sum over the MISSING entries of a unit of the other factor's S2 = var + exp^2 and of its exp^2, per column --
        the chain-independent parts of tauU / muU (which = 0) or tauV / muV (which = 1), from the matrix-core product run() uses."""
        assert self._blocks is None, "masked_sums is a hook of the single-block model (K <= %d)" % BLOCK
        self._push()
        n = self.I if which == 0 else self.J
        asq = np.zeros((n, self.K)); vsq = np.zeros((n, self.K))
        _lib.check(_lib.lib().bnmf_vb_masked_sums(self._handle(), int(which), asq.ctypes.data, vsq.ctypes.data))
        return asq, vsq

    def column_maxima(self, which):
        """Hook (tests), read-only: the column maxima of [S2 | exp^2] of U (which = 0) or V (which = 1) -- the fixed-point grid of the
        masked product's digit planes -- as fp32 bit patterns: (posted, own, was_posted), [2][K] uint32 each (row 0: S2 = var + exp^2,
        row 1: exp^2).  posted: what the factor's last relayout left; was_posted: whether the next on-chip half sweep takes them as
        they are; own: a pass of the fall-back kernel over the factor."""
        assert self._blocks is None, "column_maxima is a hook of the single-block model (K <= %d)" % BLOCK
        self._push()
        KP = 32 if self.K <= 32 else 64
        posted = np.zeros(2 * KP, dtype=np.uint32); own = np.zeros(2 * KP, dtype=np.uint32)
        flag = C.c_int(-1)
        _lib.check(_lib.lib().bnmf_vb_column_maxima(self._handle(), int(which), posted.ctypes.data, own.ctypes.data, C.byref(flag)))
        assert not posted.reshape(2, KP)[:, self.K:].any() and not own.reshape(2, KP)[:, self.K:].any(), "a padding column has a maximum"
        return posted.reshape(2, KP)[:, :self.K].copy(), own.reshape(2, KP)[:, :self.K].copy(), bool(flag.value)

    def update_U(self, k):
        """:189-191."""
        self._update(0, k, 0)

    def update_V(self, k):
        """:193-195."""
        self._update(1, k, 0)

    def update_exp_U(self, k):
        """:199-204."""
        self._update_exp("U", np.s_[:, k])

    def update_exp_V(self, k):
        """:206-211."""
        self._update_exp("V", np.s_[:, k])


bnmf_vb = bnmf_vb_optimised
