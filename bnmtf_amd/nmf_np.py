"""Drop-in for code/models/nmf_np.py (class NMF): non-probabilistic non-negative matrix factorisation with the multiplicative
updates of Lee and Seung (2001), R ~ U V^T under the I-divergence,

    U_ik <- U_ik * (sum_{j in Omega_i} V_jk R_ij / (U V^T)_ij) / (sum_{j in Omega_i} V_jk)     (and V alike),

column by column, each column seeing the columns before it.  The updates run on the device (csrc/kernel_np.hip: a block
owns a few rows, their data and their P = U V^T in registers); run() is one device call for all iterations.

    NMF = NMF(R, M, K)
    NMF.initialise(init_UV, expo_prior)     # 'ones' | 'random' | 'exponential'
    NMF.run(iterations)                     # fills all_times, all_performances; prints the I-divergence per iteration
    NMF.run(iterations, M_test=Mt)          # ... and all_performances_test: MSE / R^2 / Rp on Mt behind every iteration
    NMF.predict(M_pred); NMF.compute_I_div()

Same constructor arguments, attributes and assertion messages as the reference; build-only extras are keyword-only
(device, verbose, layout).  One GPU; ranks 1 <= K <= 256.

layout='observed' (default 'dense'): the same updates with P kept on the observed entries only (csrc/kernel_obs_np.hip;
DESIGN.md section 2.7; _observed.ObservedNP) -- device memory and time follow the number of observed entries, and a row or
column may be as long as it likes (the dense layout: at most 16 384 entries).  The whole API keeps its meaning; run(M_test=) and
run_many are the dense layout's and are refused."""
import ctypes as C
import math

import numpy as np

from . import _lib, _observed
from ._base import HeldoutMixin, check_binary, check_R_M, check_rank, compute_MSE, compute_R2, compute_Rp, performances

MAX_RANK_NP = 256


def metrics_from_np_sums(s):
    """MSE / R^2 / Rp from the eight sums of bnmtf_np_metrics (n, sum R, sum R^2, sum P, sum P^2, sum R P, I-div, SSE): the
    quantities of nmf_np.py:129-144, with the squared error summed directly."""
    n, sr, srr, sp, spp, srp, _, sse = [float(v) for v in s]
    ss_tot = srr - sr * sr / n
    cov = srp - sr * sp / n
    vp = spp - sp * sp / n
    with np.errstate(all="ignore"):
        rp = np.float64(cov) / np.float64(math.sqrt(max(ss_tot, 0.0)) * math.sqrt(max(vp, 0.0)))
    return {"MSE": sse / n, "R^2": (1.0 - sse / ss_tot) if ss_tot != 0.0 else np.inf, "Rp": float(rp)}


class NPDevice(HeldoutMixin):
    """The bnmtf_np_create handle of one model (created at the first device call) and the calls both models share.  run(M_test=):
    the helpers of _base.HeldoutMixin; the record holds six sums, finished with metrics_from_sums."""

    def _init_np(self, name, device, rank, world):
        if int(world) != 1 or int(rank) != 0:
            raise _lib.BnmtfError("%s runs on one GPU (world = %s): the non-probabilistic models are not sharded" % (name, world))
        self._h = None
        self._device = int(device)
        self._pushed = None

    def _handle(self):
        if self._h is None:
            R32 = np.ascontiguousarray(self.R, dtype=np.float32)
            Mb = np.ascontiguousarray(check_binary(self.M, "M"))
            M8 = Mb.view(np.uint8)
            h = C.c_void_p()
            _lib.check(_lib.lib().bnmtf_np_create(_lib.ptr(R32), _lib.ptr(M8), self.I, self.J, self.K, getattr(self, "L", 0),
                                                  self._device, C.byref(h)))
            self._h = h
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            _lib.lib().bnmtf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _factors(self):
        raise NotImplementedError

    def _entry(self, name):
        """The library's entry point `name` (_observed.ObservedNP: the other layout's call in its place)."""
        return getattr(_lib.lib(), name)

    def _push(self):
        """Hand the current factors to the device unless it holds them already (nothing touched them since the last pull)."""
        cur = [np.asarray(f, dtype=float) for f in self._factors()]
        if self._pushed is not None and self._pushed[0] is self._h and all(np.array_equal(a, b) for a, b in zip(cur, self._pushed[1])):
            return
        self._set_state(*[_lib.f64(f) for f in cur])
        self._pushed = (self._h, [f.copy() for f in cur])

    def _note_pulled(self):
        self._pushed = (self._h, [np.array(f, dtype=float) for f in self._factors()])

    def _sums(self, M_pred=None):
        self._push()
        Mp = None
        if M_pred is not None:
            Mp_ = np.asarray(M_pred)
            assert Mp_.shape == (self.I, self.J), "M_pred has the wrong shape: %s instead of %s." % (Mp_.shape, (self.I, self.J))
            Mp = np.ascontiguousarray(check_binary(Mp_, "M_pred"), dtype=np.uint8)
        out = np.zeros(8)
        _lib.check(_lib.lib().bnmtf_np_metrics(self._handle(), _lib.ptr(Mp), _lib.ptr(out)))
        return out

    def _run_device(self, fn, iterations, M_test=None):
        """run(): M_test as the six other classes take it -- the held-out metrics of the factors every iteration ends with, in
        all_performances_test; the attribute exists only after a call that was given a mask, and the trajectory is the same
        bits with and without one."""
        Mt = self._check_heldout(M_test)
        it = int(iterations)
        perf, idiv, times = self._run_prepare(it)
        self._set_heldout(Mt)
        _lib.check(fn(self._handle(), it, _lib.ptr(perf), _lib.ptr(idiv), _lib.ptr(times)))
        self._finish_heldout(it)
        return self._run_finish(it, perf, idiv, times)

    def _run_prepare(self, it):
        """What run() does before the device call (batch.run_many: before the call that runs this model among others): the
        factors to the device, the output arrays."""
        self._push()
        return np.zeros((it, 3)), np.zeros(it), np.zeros(it)

    def _run_finish(self, it, perf, idiv, times):
        """What run() does behind the device call."""
        self._pull()
        self.all_times = list(times)
        self.all_performances = performances(perf)
        if self.verbose:
            for i in range(it):
                print("Iteration %s. I-divergence: %s. MSE: %s. R^2: %s. Rp: %s." % (i + 1, idiv[i], perf[i, 0], perf[i, 1], perf[i, 2]))
        return idiv

    # Functions for computing MSE, R^2 (coefficient of determination), Rp (Pearson correlation)
    def predict(self, M_pred):
        """Metrics of the current point on M_pred (nmf_np.py:124-129)."""
        return metrics_from_np_sums(self._sums(M_pred))

    def compute_MSE(self, M, R, R_pred):
        return compute_MSE(np.asarray(M), np.asarray(R), np.asarray(R_pred))

    def compute_R2(self, M, R, R_pred):
        return compute_R2(np.asarray(M), np.asarray(R), np.asarray(R_pred))

    def compute_Rp(self, M, R, R_pred):
        return compute_Rp(np.asarray(M), np.asarray(R), np.asarray(R_pred))

    def compute_I_div(self):
        """:146-148: sum over the training entries of R log(R / P) - R + P."""
        return float(self._sums(None)[6])


class NMF(_observed.ObservedNP, NPDevice):
    def __init__(self, R, M, K, *, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense'):
        _observed.refuse_entries(self, R, M)
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K = K
        self._init_layout(layout, world)
        self.metrics = ['MSE', 'R^2', 'Rp']
        check_R_M(self.R, self.M)
        (self.I, self.J) = self.R.shape
        check_rank("NMF", MAX_RANK_NP, K=self.K)
        self.verbose = verbose
        self._init_np("NMF", device, rank, world)
        # For computing the I-div it is better if unknown values are 1's, not 0's (:52-55)
        self.R_excl_unknown = np.where(self.M != 0, self.R, 1.)

    def check_empty_rows_columns(self):
        """:59-67."""
        check_R_M(self.R, self.M)

    def initialise(self, init_UV='random', expo_prior=1.):
        """:71-84.  'exponential' consumes numpy.random.exponential in (i,k) then (j,k) order, the reference's scalar loop."""
        assert init_UV in ['ones', 'random', 'exponential'], "Unrecognised init option for U,V: %s." % init_UV
        if init_UV == 'ones':
            self.U = np.ones((self.I, self.K))
            self.V = np.ones((self.J, self.K))
        elif init_UV == 'random':
            self.U = np.random.rand(self.I, self.K)
            self.V = np.random.rand(self.J, self.K)
        elif init_UV == 'exponential':
            self.U = np.random.exponential(scale=1.0 / expo_prior, size=(self.I, self.K))
            self.V = np.random.exponential(scale=1.0 / expo_prior, size=(self.J, self.K))

    def run(self, iterations, *, M_test=None):
        """:87-107.  One device call runs all iterations.  M_test: the held-out metrics of U V^T behind every iteration, in
        all_performances_test (see bnmf_gibbs_optimised.run)."""
        self._check_initialised()
        self._run_device(self._entry("bnmf_np_run"), iterations, M_test)

    def _check_initialised(self):
        assert hasattr(self, 'U') and hasattr(self, 'V'), "U and V have not been initialised - please run NMF.initialise() first."

    def train(self, iterations, init_UV='random', expo_prior=1.):
        """:111-113."""
        self.initialise(init_UV=init_UV, expo_prior=expo_prior)
        self.run(iterations=iterations)

    def update_U(self, k):
        """:117-118 on the device."""
        self._update(0, k)

    def update_V(self, k):
        """:120-121 on the device."""
        self._update(1, k)

    def _update(self, which, k):
        assert 0 <= int(k) < self.K, "column %s out of range (K = %s)" % (k, self.K)
        self._push()
        _lib.check(self._entry("bnmf_np_update")(self._handle(), int(which), int(k)))
        self._pull()

    def _factors(self):
        return [self.U, self.V]

    def _set_state(self, U, V):
        assert U.shape == (self.I, self.K) and V.shape == (self.J, self.K), "U, V have the wrong shapes: %s, %s" % (U.shape, V.shape)
        _lib.check(self._entry("bnmf_np_set_state")(self._handle(), _lib.ptr(U), _lib.ptr(V)))

    def _pull(self):
        U = np.zeros((self.I, self.K)); V = np.zeros((self.J, self.K))
        _lib.check(self._entry("bnmf_np_get_state")(self._handle(), _lib.ptr(U), _lib.ptr(V)))
        self.U, self.V = U, V
        self._note_pulled()
