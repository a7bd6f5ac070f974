"""Drop-in for code/models/bnmtf_gibbs_optimised.py (class bnmtf_gibbs_optimised): Gibbs sampler
for Bayesian non-negative matrix tri-factorisation R ~ F.S.G^T on an MI355X.

    BNMTF = bnmtf_gibbs_optimised(R, M, K, L, priors)
    BNMTF.initialise(init_S, init_FG)      # init_S: 'random'|'exp'; init_FG: 'random'|'exp'|'kmeans'
    BNMTF.run(iterations)                  # -> (all_F, all_S, all_G, all_tau)

layout='observed' (keyword only, default 'dense') keeps the per-entry state on the OBSERVED entries (DESIGN.md section 2.7;
_observed.py): cost and device memory follow the number of observed entries, the layout for matrices that are mostly missing.
Same update order and Philox keying, so the same seed gives the dense layout's chain up to fp32 rounding.  K, L <= 32, one GPU.
"""
import numpy as np

from . import _lib, _observed
from ._base import broadcast_lambda, check_rank, check_R_M
from .kmeans import KMeans
from ._blocked import BLOCK, MAX_BLOCKS, TriBlocks
from ._sampler import GibbsSampler

MAX_RANK_BLOCKED = BLOCK * MAX_BLOCKS      # 256: K or L above 64 run as blocks of S (_blocked.py: TriBlocks)


class bnmtf_gibbs_optimised(GibbsSampler):
    _FACTORS = ("F", "S", "G")
    _PRIORS = ("lambdaF", "lambdaS", "lambdaG")
    _DENSE = dict(set_state="bnmtf_set_state", get_state="bnmtf_get_state", run="bnmtf_gibbs_run", cond_params="bnmtf_cond_params",
                  run_many="bnmtf_gibbs_run_many")
    _OBSERVED = dict(set_state="bnmtf_otri_set_state", get_state="bnmtf_otri_get_state", run="bnmtf_otri_run",
                     cond_params="bnmtf_otri_cond_params", create=_observed.create_tri_handle, metric_sums=_observed.tri_metric_sums)
    _BLOCKS_KEEP_STATE = False          # (a blocked model's state lives on the host between the phases of its iterations: _sampler.py)

    def __init__(self, R, M, K, L, priors, *, seed=None, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense'):
        _observed.check_layout(layout)
        _observed.refuse_entries(self, R, M)
        self._layout = layout
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K = K
        self.L = L
        check_R_M(self.R, self.M)
        if layout == 'observed':
            _observed.check_constructor_tri(self, world)
        else:
            check_rank("bnmtf_gibbs_optimised", MAX_RANK_BLOCKED, K=self.K, L=self.L)
        (self.I, self.J) = self.R.shape
        self.size_Omega = self.M.sum()
        self.alpha, self.beta = float(priors['alpha']), float(priors['beta'])
        self.lambdaF = broadcast_lambda(priors['lambdaF'], (self.I, self.K), "lambdaF")
        self.lambdaS = broadcast_lambda(priors['lambdaS'], (self.K, self.L), "lambdaS")
        self.lambdaG = broadcast_lambda(priors['lambdaG'], (self.J, self.L), "lambdaG")
        self.verbose = verbose
        self._init_device(seed, device, rank, world, comm_id)
        # K or L above 64 (the reference has no limit, :56-84): F's and G's column blocks and the blocks of S, one device model each
        self._blocks = None
        if self.K > BLOCK or self.L > BLOCK:
            assert world == 1, "ranks above %d run on one GPU (blocks: DESIGN.md section 8)" % BLOCK
            from .bnmf_gibbs import bnmf_gibbs_optimised
            self._blocks = TriBlocks(self, bnmf_gibbs_optimised, bnmtf_gibbs_optimised)

    def _shapes(self):
        return ((self.I, self.K), (self.K, self.L), (self.J, self.L))

    def _handle(self):
        if getattr(self, "_blocks", None) is not None:       # shape-only entry points (omega_counts, ...): the first F block's handle
            self._blocks._prepare()
            return self._blocks.Fch[0]._handle()
        return super(bnmtf_gibbs_optimised, self)._handle()

    def describe(self):
        if self._blocks is not None:
            self._blocks._prepare()
            return "blocks of F %s, of G %s, of S their product: " % (self._blocks.kr, self._blocks.lr) + " | ".join(ch.describe() for ch in self._blocks.children())
        return super(bnmtf_gibbs_optimised, self).describe()

    def initialise(self, init_S='random', init_FG='random'):
        """:106-134."""
        assert init_S in ['random', 'exp'], "Unknown initialisation option for S: %s. Should be 'random' or 'exp'." % init_S
        assert init_FG in ['random', 'exp', 'kmeans'], "Unknown initialisation option for S: %s. Should be 'random', 'exp', or 'kmeans." % init_FG
        self.S = 1. / self.lambdaS
        if init_S == 'random':
            self.S = self._rng().exponential(scale=1.0 / self.lambdaS)
        self.F, self.G = 1. / self.lambdaF, 1. / self.lambdaG
        if init_FG == 'random':
            self.F = self._rng().exponential(scale=1.0 / self.lambdaF)
            self.G = self._rng().exponential(scale=1.0 / self.lambdaG)
        elif init_FG == 'kmeans':
            if self.verbose: print("Initialising F using KMeans.")
            kmeans_F = KMeans(self.R, self.M, self.K, device=self._device, layout=getattr(self, '_layout', 'dense'))
            kmeans_F.initialise()
            kmeans_F.cluster()
            self.F = kmeans_F.clustering_results + 0.2
            if self.verbose: print("Initialising G using KMeans.")
            kmeans_G = KMeans(self.R.T, self.M.T, self.L, device=self._device, layout=getattr(self, '_layout', 'dense'))
            kmeans_G.initialise()
            kmeans_G.cluster()
            self.G = kmeans_G.clustering_results + 0.2
        self.tau = self.alpha_s() / self.beta_s()

    def triple_dot(self, M1, M2, M3):
        """:184-185 (host utility on explicit arrays)."""
        return np.dot(M1, np.dot(M2, M3))

    # Parameters of the conditional posteriors of F, S, G, evaluated on the device (alpha_s, beta_s: _sampler.py)
    def _cond(self, which, k, l, n):
        if self._blocks is not None:
            return self._blocks.cond(which, k, l, self.F, self.S, self.G, float(getattr(self, "tau", 1.0)))
        self._push()
        numer = np.zeros(n); tauk = np.zeros(n)
        _lib.check(self._entry("cond_params")(self._handle(), which, int(k), int(l), _lib.ptr(numer), _lib.ptr(tauk)))
        return numer, tauk

    def tauF(self, k):
        return self._cond(0, k, 0, self.I)[1]

    def muF(self, tauFk, k):
        return 1. / np.asarray(tauFk, dtype=float) * self._cond(0, k, 0, self.I)[0]

    def tauS(self, k, l):
        return float(self._cond(1, k, l, 1)[1][0])

    def muS(self, tauSkl, k, l):
        return 1. / tauSkl * float(self._cond(1, k, l, 1)[0][0])

    def tauG(self, l):
        return self._cond(2, 0, l, self.J)[1]

    def muG(self, tauGl, l):
        return 1. / np.asarray(tauGl, dtype=float) * self._cond(2, 0, l, self.J)[0]

    def log_likelihood(self, expF, expS, expG, exptau):
        """:282-285."""
        return self._log_likelihood((expF, expS, expG), exptau)


bnmtf_gibbs = bnmtf_gibbs_optimised
