"""Drop-in for code/models/bnmf_gibbs_optimised.py (class bnmf_gibbs_optimised):
Gibbs sampler for Bayesian non-negative matrix factorisation R ~ U.V^T, with the
per-iteration work done by libbnmtf_hip.so on an MI355X.

    BNMF = bnmf_gibbs_optimised(R, M, K, priors)
    BNMF.initialise(init)          # 'random' | 'exp'
    BNMF.run(iterations)           # -> (all_U, all_V, all_tau)
    BNMF.approx_expectation(burn_in, thinning); BNMF.predict(M_pred, burn_in, thinning)
    BNMF.quality(metric, burn_in, thinning)

Same constructor arguments, attributes (R, M, I, J, K, size_Omega, alpha, beta,
lambdaU, lambdaV, U, V, tau, all_U, all_V, all_tau, all_times, all_performances),
methods and assertion messages as the reference.  Build-only extras are
keyword-only: seed (Philox key; default drawn from numpy.random so that
numpy.random.seed() makes runs reproducible, as in the reference), device,
verbose, rank/world/comm_id (row/column sharding over several GPUs), layout.

layout='observed' keeps the per-entry state on the OBSERVED entries instead of the missing
ones (_observed.py): cost and device memory follow the number of
observed entries, the layout for matrices that are mostly missing.  Same chain for the same
seed (same conditionals, same Philox keying), ranks up to 256 on one handle, one GPU; no
expectation=, run_many, set_sweep_path / set_small_path / set_profiling.  On this layout the
matrix may be given as lists, bnmf_gibbs_optimised(Entries, None, K, priors, layout='observed')
(entries.py: nothing of size I x J on the host), and run(M_test=Entries) keeps the held-out
curve in all_performances_test.
"""
import numpy as np

from . import _lib, _observed
from ._base import broadcast_lambda, check_rank
from ._blocked import BLOCK, MAX_BLOCKS, ColumnBlocks
from ._sampler import GibbsSampler

MAX_RANK_BLOCKED = BLOCK * MAX_BLOCKS      # 256: ranks above 64 run as column blocks (_blocked.py)


class bnmf_gibbs_optimised(GibbsSampler):
    _FACTORS = ("U", "V")
    _PRIORS = ("lambdaU", "lambdaV")
    _DENSE = dict(set_state="bnmf_set_state", get_state="bnmf_get_state", run="bnmf_gibbs_run", cond_params="bnmf_cond_params",
                  run_many="bnmf_gibbs_run_many")
    _OBSERVED = dict(set_state="bnmf_obs_set_state", get_state="bnmf_obs_get_state", run="bnmf_obs_run", cond_params="bnmf_obs_cond_params",
                     create=_observed.create_handle, metric_sums=_observed.metric_sums)
    _BLOCKS_KEEP_STATE = True           # (ColumnBlocks hold U, V, tau between calls: _sampler.py)

    def __init__(self, R, M, K, priors, *, seed=None, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense'):
        _observed.check_layout(layout)
        self._layout = layout
        self.K = K
        (self.I, self.J), self.size_Omega = _observed.take_R_M(self, R, M, layout)      # (dense arrays, or an Entries and None)
        if layout == 'observed':
            _observed.check_constructor(self, world)
        else:
            check_rank("bnmf_gibbs_optimised", MAX_RANK_BLOCKED, K=self.K)
        self.alpha, self.beta = float(priors['alpha']), float(priors['beta'])
        self.lambdaU = broadcast_lambda(priors['lambdaU'], (self.I, self.K), "lambdaU")
        self.lambdaV = broadcast_lambda(priors['lambdaV'], (self.J, self.K), "lambdaV")
        self.verbose = verbose
        self._init_device(seed, device, rank, world, comm_id)
        # ranks above 64 (the reference has no limit, :54-78): column blocks of at most 64, one device model each (_blocked.py)
        self._blocks = None
        if self.K > BLOCK and layout == 'dense':       # (the observed-entry layout ties no rank to a lane: one handle up to 256)
            assert world == 1, "ranks above %d run on one GPU (column blocks: DESIGN.md section 8)" % BLOCK
            self._blocks = ColumnBlocks(self, bnmf_gibbs_optimised)

    def _shapes(self):
        return ((self.I, self.K), (self.J, self.K))

    def _handle(self):
        if getattr(self, "_blocks", None) is not None:       # shape-only entry points (omega_counts, ...): the first block's handle
            return self._blocks.handles()[0]
        return super(bnmf_gibbs_optimised, self)._handle()

    def initialise(self, init='random'):
        """:100-117.  'random' consumes numpy.random.exponential in (i,k) row-major order,
        i.e. the same values as the reference's scalar loop for the same numpy seed."""
        assert init in ['random', 'exp'], "Unknown initialisation option: %s. Should be 'random' or 'exp'." % init
        if init == 'random':
            self.U = self._rng().exponential(scale=1.0 / self.lambdaU)
            self.V = self._rng().exponential(scale=1.0 / self.lambdaV)
        else:
            self.U = 1.0 / self.lambdaU
            self.V = 1.0 / self.lambdaV
        self.tau = self.alpha_s() / self.beta_s()

    def describe(self):
        if self._blocks is not None:
            self._blocks._prepare()
            return "column blocks %s: " % (self._blocks.ranges,) + " | ".join(ch.describe() for ch in self._blocks.children)
        return super(bnmf_gibbs_optimised, self).describe()

    # Parameters of the conditional posteriors (:161-177), evaluated on the device (alpha_s, beta_s: _sampler.py)
    def _cond(self, which, k):
        self._push()
        if self._blocks is not None:
            return self._blocks.cond(which, k)
        n = self.I if which == 0 else self.J
        numer = np.zeros(n); tauk = np.zeros(n)
        _lib.check(self._entry("cond_params")(self._handle(), which, int(k), _lib.ptr(numer), _lib.ptr(tauk)))
        return numer, tauk

    def tauU(self, k):
        return self._cond(0, k)[1]

    def muU(self, tauUk, k):
        return 1. / np.asarray(tauUk, dtype=float) * self._cond(0, k)[0]

    def tauV(self, k):
        return self._cond(1, k)[1]

    def muV(self, tauVk, k):
        return 1. / np.asarray(tauVk, dtype=float) * self._cond(1, k)[0]

    def log_likelihood(self, expU, expV, exptau):
        """:247-251."""
        return self._log_likelihood((expU, expV), exptau)


bnmf_gibbs = bnmf_gibbs_optimised
