"""Drop-in for code/models/bnmtf_vb_optimised.py (class bnmtf_vb_optimised): variational Bayes for
Bayesian non-negative matrix tri-factorisation R ~ F.S.G^T on an MI355X.

    BNMTF = bnmtf_vb_optimised(R, M, K, L, priors)
    BNMTF.initialise(init_S, init_FG, tauFSG={})     # init_S: 'random'|'exp'; init_FG: 'random'|'exp'|'kmeans'
    BNMTF.run(iterations)

Per iteration (bnmtf_vb_optimised.py:170-192): the K.L entries of S, the K columns of F and the L columns of G are
each updated in a freshly shuffled order.  The orders are drawn HERE with `random.shuffle` -- the same three calls on
the same lists as the reference, so `random.seed(s)` reproduces its trajectory -- and handed to the device, which
runs all iterations in one call.  K, L <= 32."""
import itertools
import math
import random

import numpy as np
import scipy.special

from . import _lib
from ._base import check_rank, check_R_M
from ._variational import Variational, q_names
from .kmeans import KMeans


class bnmtf_vb_optimised(Variational):
    _FACTORS = ("F", "S", "G")
    _NAMES = q_names(_FACTORS)
    # (esd_rest: bnmtf_vb_exp_square_diff also offers the six sums of the training mask -- nobody takes them)
    _DENSE = {"set_state": "bnmtf_vb_set_state", "get_state": "bnmtf_vb_get_state", "run": "bnmtf_vb_run", "update": "bnmtf_vb_update",
              "exp_square_diff": "bnmtf_vb_exp_square_diff", "esd_rest": (None,), "run_many": "bnmtf_vb_run_many"}
    _KEEPS_DEVICE_STATE = False         # (with the record the device would keep derived state across calls: not compared yet)
    _ONES_IN_PUSH = _NAMES              # the reference's tests set only some of the attributes

    def __init__(self, R, M, K, L, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None):
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K, self.L = K, L
        check_R_M(self.R, self.M)
        check_rank("bnmtf_vb_optimised", 32, K=self.K, L=self.L)
        (self.I, self.J) = self.R.shape
        self.size_Omega = self.M.sum()
        self._init_priors(priors, device, verbose, rank, world, comm_id)

    def _factor_shapes(self):
        return [(self.I, self.K), (self.K, self.L), (self.J, self.L)]

    # -- initialise / run -------------------------------------------------------
    def train(self, init_S, init_FG, iterations):
        """:100-102."""
        self.initialise(init_S, init_FG)
        return self.run(iterations)

    def initialise(self, init_S='random', init_FG='random', tauFSG={}):
        """:107-156."""
        self.tauF = np.array(tauFSG['tauF'], dtype=float) if 'tauF' in tauFSG else np.ones((self.I, self.K))
        self.tauS = np.array(tauFSG['tauS'], dtype=float) if 'tauS' in tauFSG else np.ones((self.K, self.L))
        self.tauG = np.array(tauFSG['tauG'], dtype=float) if 'tauG' in tauFSG else np.ones((self.J, self.L))
        assert init_S in ['exp', 'random'], "Unrecognised init option for S: %s." % init_S
        self.muS = 1. / self.lambdaS
        if init_S == 'random':
            self.muS = self._rng().exponential(scale=1.0 / self.lambdaS)
        assert init_FG in ['exp', 'random', 'kmeans'], "Unrecognised init option for F,G: %s." % init_FG
        self.muF, self.muG = 1. / self.lambdaF, 1. / self.lambdaG
        if init_FG == 'random':
            self.muF = self._rng().exponential(scale=1.0 / self.lambdaF)
            self.muG = self._rng().exponential(scale=1.0 / self.lambdaG)
        elif init_FG == 'kmeans':
            if self.verbose: print("Initialising F using KMeans.")
            kmeans_F = KMeans(self.R, self.M, self.K, device=self._device, layout=getattr(self, '_layout', 'dense'))
            kmeans_F.initialise()
            kmeans_F.cluster()
            self.muF = kmeans_F.clustering_results
            if self.verbose: print("Initialising G using KMeans.")
            kmeans_G = KMeans(self.R.T, self.M.T, self.L, device=self._device, layout=getattr(self, '_layout', 'dense'))
            kmeans_G.initialise()
            kmeans_G.cluster()
            self.muG = kmeans_G.clustering_results
        self._initial_moments()            # (update_exp_F(k), update_exp_S(k, l), update_exp_G(l) of every column and entry, :147-153)
        self.update_tau()
        self.update_exp_tau()

    def _draw_orders(self, iterations):
        """The three shuffles of every iteration, as the reference's run() makes them (:171-186)."""
        K, L = self.K, self.L
        out = np.zeros((iterations, K * L + K + L), dtype=np.int32)
        for it in range(iterations):
            indices_kl = list(itertools.product(range(K), range(L)))
            random.shuffle(indices_kl)
            indices_k = list(range(K))
            random.shuffle(indices_k)
            indices_l = list(range(L))
            random.shuffle(indices_l)
            out[it, :K * L] = [k * L + l for k, l in indices_kl]
            out[it, K * L:K * L + K] = indices_k
            out[it, K * L + K:] = indices_l
        return out

    def run(self, iterations, orders=None, *, M_test=None):
        """:160-205.  orders (optional): int array [iterations][K L + K + L] of update orders instead of fresh shuffles.  M_test:
        the held-out metrics of E[F] E[S] E[G]^T behind every iteration, in all_performances_test (see bnmf_gibbs_optimised.run)."""
        Mt = self._check_heldout(M_test)
        it = int(iterations)
        orders = self._draw_orders(it) if orders is None else np.ascontiguousarray(orders, dtype=np.int32)
        assert orders.shape == (it, self.K * self.L + self.K + self.L)
        # (all_elbo_terms: of the ELBO the reference prints per iteration only the last one can be finished -- the K.L terms of S
        # need the q(S) of that iteration; earlier iterations carry the F / G / tau part)
        self._run(it, Mt, orders)

    def _run_device(self, it, orders, exptau, perf, terms, times):
        """The device call of run(), either layout's."""
        _lib.check(self._entry("run")(self._handle(), it, _lib.ptr(orders), _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times)))

    # -- ELBO -------------------------------------------------------------------
    def elbo(self):
        """:208-223: exp_square_diff on the device, the O(IK + KL + JL) sums on the host."""
        with np.errstate(all='ignore'):
            v = self.size_Omega / 2. * (self.explogtau - math.log(2 * math.pi)) - self.exptau / 2. * self.exp_square_diff() \
                + self.alpha * math.log(self.beta) - scipy.special.gammaln(self.alpha) \
                + (self.alpha - 1.) * self.explogtau - self.beta * self.exptau \
                - self.alpha_s * math.log(self.beta_s) + scipy.special.gammaln(self.alpha_s) \
                - (self.alpha_s - 1.) * self.explogtau + self.beta_s * self.exptau
            for lam, e, var, mu, tau, n in ((self.lambdaF, self.expF, self.varF, self.muF, self.tauF, self.I * self.K),
                                            (self.lambdaS, self.expS, self.varS, self.muS, self.tauS, self.K * self.L),
                                            (self.lambdaG, self.expG, self.varG, self.muG, self.tauG, self.J * self.L)):
                v += np.log(lam).sum() - (lam * e).sum()
                v += -.5 * np.log(tau).sum() + n / 2. * math.log(2 * math.pi) \
                    + np.log(0.5 * scipy.special.erfc(-mu * np.sqrt(tau) / math.sqrt(2))).sum() + (tau / 2. * (var + (e - mu) ** 2)).sum()
            return v

    def triple_dot(self, M1, M2, M3):
        """:226-227 (host utility on explicit arrays)."""
        return np.dot(M1, np.dot(M2, M3))

    # -- updates ----------------------------------------------------------------
    def update_F(self, k):
        """:241-250."""
        self._update(0, k, 0, 0)

    def update_S(self, k, l):
        """:252-262."""
        self._update(1, k, l, 0)

    def update_G(self, l):
        """:264-273."""
        self._update(2, 0, l, 0)

    def update_exp_F(self, k):
        """:276-278."""
        self._update_exp("F", np.s_[:, k])

    def update_exp_S(self, k, l):
        """:280-282."""
        self._update_exp("S", (k, l))

    def update_exp_G(self, l):
        """:284-285."""
        self._update_exp("G", np.s_[:, l])


bnmtf_vb = bnmtf_vb_optimised
