"""Drop-in for code/models/nmtf_np.py (class NMTF): non-probabilistic non-negative matrix tri-factorisation with the
multiplicative updates of Yoo and Choi (2009), R ~ F S G^T under the I-divergence.  Per iteration the K L entries of S row by
row, then the K columns of F, then the L columns of G, each update seeing all the ones before it (:127-141).

The F step is the half sweep of nmf_np with V := G S^T and the G step the one with U := F S (csrc/kernel_np.hip).  The S step is
K L dependent passes over the observed entries -- the multiplicative rule is not linear in P, so each entry needs the P its
predecessor left -- one launch per entry, each applying the previous entry's change to P while it sums the next numerator.

    NMTF = NMTF(R, M, K, L)
    NMTF.initialise(init_S, init_FG, expo_prior)    # init_S: 'ones'|'random'|'exponential'; init_FG: ... |'kmeans'
    NMTF.run(iterations)                            # M_test=Mt: all_performances_test, the held-out metrics per iteration
    NMTF.predict(M_pred); NMTF.compute_I_div()

One GPU; ranks 1 <= K, L <= 256.

layout='observed' (keyword, default 'dense'): the same updates on the observed-entry layout (csrc/kernel_obs_np.hip; DESIGN.md
section 2.7; _observed.ObservedNP): P lives on the observed entries only, so the K L passes of the S step read what is observed
instead of an I x J matrix, and rows and columns have no length limit.  run(M_test=) and run_many are refused there."""
import numpy as np

from . import _lib, _observed
from ._base import check_R_M, check_rank
from .kmeans import KMeans
from .nmf_np import MAX_RANK_NP, NPDevice


class NMTF(_observed.ObservedNP, NPDevice):
    def __init__(self, R, M, K, L, *, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense'):
        _observed.refuse_entries(self, R, M)
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K = K
        self.L = L
        self._init_layout(layout, world)
        self.metrics = ['MSE', 'R^2', 'Rp']
        check_R_M(self.R, self.M)
        (self.I, self.J) = self.R.shape
        check_rank("NMTF", MAX_RANK_NP, K=self.K, L=self.L)
        self.verbose = verbose
        self._init_np("NMTF", device, rank, world)
        # For computing the I-div it is better if unknown values are 1's, not 0's (:57-60)
        self.R_excl_unknown = np.where(self.M != 0, self.R, 1.)

    def check_empty_rows_columns(self):
        """:64-72."""
        check_R_M(self.R, self.M)

    def initialise(self, init_S='random', init_FG='random', expo_prior=1.):
        """:76-113: S first, then F and G; 'exponential' consumes numpy.random.exponential in the reference's element order."""
        assert init_S in ['ones', 'random', 'exponential'], "Unrecognised init option for S: %s." % init_S
        assert init_FG in ['ones', 'random', 'exponential', 'kmeans'], "Unrecognised init option for F,G: %s." % init_FG
        if init_S == 'ones':
            self.S = np.ones((self.K, self.L))
        elif init_S == 'random':
            self.S = np.random.rand(self.K, self.L)
        elif init_S == 'exponential':
            self.S = np.random.exponential(scale=1.0 / expo_prior, size=(self.K, self.L))

        if init_FG == 'ones':
            self.F = np.ones((self.I, self.K))
            self.G = np.ones((self.J, self.L))
        elif init_FG == 'random':
            self.F = np.random.rand(self.I, self.K)
            self.G = np.random.rand(self.J, self.L)
        elif init_FG == 'exponential':
            self.F = np.random.exponential(scale=1.0 / expo_prior, size=(self.I, self.K))
            self.G = np.random.exponential(scale=1.0 / expo_prior, size=(self.J, self.L))
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

    def run(self, iterations, *, M_test=None):
        """:116-144.  One device call runs all iterations.  M_test: the held-out metrics of F S G^T behind every iteration, in
        all_performances_test (see bnmf_gibbs_optimised.run)."""
        self._check_initialised()
        self._run_device(self._entry("bnmtf_np_run"), iterations, M_test)

    def _check_initialised(self):
        assert hasattr(self, 'F') and hasattr(self, 'S') and hasattr(self, 'G'), \
            "F, S and G have not been initialised - please run NMTF.initialise() first."

    def train(self, iterations, init_S='random', init_FG='random', expo_prior=1.):
        """:148-150."""
        self.initialise(init_S=init_S, init_FG=init_FG, expo_prior=expo_prior)
        self.run(iterations=iterations)

    def triple_dot(self, M1, M2, M3):
        """:155-156 (host NumPy, as in the reference: a helper on explicit matrices)."""
        return np.dot(M1, np.dot(M2, M3))

    def update_F(self, k):
        """:158-163 on the device."""
        assert 0 <= int(k) < self.K, "column %s out of range (K = %s)" % (k, self.K)
        self._update(0, k, 0)

    def update_G(self, l):
        """:165-170 on the device."""
        assert 0 <= int(l) < self.L, "column %s out of range (L = %s)" % (l, self.L)
        self._update(2, 0, l)

    def update_S(self, k, l):
        """:172-177 on the device."""
        assert 0 <= int(k) < self.K and 0 <= int(l) < self.L, "entry (%s, %s) out of range (K = %s, L = %s)" % (k, l, self.K, self.L)
        self._update(1, k, l)

    def _update(self, which, k, l):
        self._push()
        _lib.check(self._entry("bnmtf_np_update")(self._handle(), int(which), int(k), int(l)))
        self._pull()

    def _factors(self):
        return [self.F, self.S, self.G]

    def _set_state(self, F, S, G):
        assert F.shape == (self.I, self.K) and S.shape == (self.K, self.L) and G.shape == (self.J, self.L), \
            "F, S, G have the wrong shapes: %s, %s, %s" % (F.shape, S.shape, G.shape)
        _lib.check(self._entry("bnmtf_np_set_state")(self._handle(), _lib.ptr(F), _lib.ptr(S), _lib.ptr(G)))

    def _pull(self):
        F = np.zeros((self.I, self.K)); S = np.zeros((self.K, self.L)); G = np.zeros((self.J, self.L))
        _lib.check(self._entry("bnmtf_np_get_state")(self._handle(), _lib.ptr(F), _lib.ptr(S), _lib.ptr(G)))
        self.F, self.S, self.G = F, S, G
        self._note_pulled()
