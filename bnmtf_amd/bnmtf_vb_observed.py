"""bnmtf_vb_observed: the variational tri-factorisation (bnmtf_vb_optimised) on the observed-entry layout.

    BNMTF = bnmtf_vb_observed(R, M, K, L, priors)
    BNMTF.initialise(init_S, init_FG, tauFSG={})
    BNMTF.run(iterations)

The API, the attributes and the assertion messages of bnmtf_vb_optimised; run() draws the three shuffles of every iteration with
random.shuffle exactly as that class does and hands them to the device once per call.  The device keeps the residual
R_ij - E[F_i] E[S] E[G_j] on the OBSERVED entries (csrc/kernel_obs_vb.hip, kernel_obs_tri.hip, kernel_obs_trivb.hip), so cost and
device memory follow the number of observed entries: the class for matrices that are mostly missing.  R and M stay dense NumPy
arrays at the Python boundary.  K, L <= 32, one GPU; no run(M_test=), run_many, masked_sums / column_maxima, set_sweep_path /
set_small_path / set_profiling.  A class of its own, not a keyword of bnmtf_vb_optimised: that class keeps refusing layout=."""
import ctypes as C

import numpy as np

from . import _lib, _observed
from ._base import broadcast_lambda, check_R_M
from .bnmtf_vb import bnmtf_vb_optimised


class bnmtf_vb_observed(_observed.ObservedVB, bnmtf_vb_optimised):
    _SET_STATE, _GET_STATE = "bnmtf_otvb_set_state", "bnmtf_otvb_get_state"

    def __init__(self, R, M, K, L, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None):
        self._layout = 'observed'
        _observed.refuse_entries(self, R, M)
        self.R = np.array(R, dtype=float)
        self.M = np.array(M, dtype=float)
        self.K, self.L = K, L
        check_R_M(self.R, self.M)
        _observed.check_constructor_tri(self, world)
        (self.I, self.J) = self.R.shape
        self.size_Omega = self.M.sum()
        self.alpha, self.beta = float(priors['alpha']), float(priors['beta'])
        self.lambdaF = broadcast_lambda(priors['lambdaF'], (self.I, self.K), "lambdaF")
        self.lambdaS = broadcast_lambda(priors['lambdaS'], (self.K, self.L), "lambdaS")
        self.lambdaG = broadcast_lambda(priors['lambdaG'], (self.J, self.L), "lambdaG")
        self.verbose = verbose
        self._init_device(0, device, rank, world, comm_id)      # VB draws nothing: the key is unused
        self._blocks = None

    def _handle(self):
        if self._h is None:
            self._h = _observed.create_tri_handle(self)
        return self._h

    def _push(self):
        for n, s in zip(self._NAMES, self._shapes()):      # the reference's tests set only some of the attributes
            if not hasattr(self, n):
                setattr(self, n, np.ones(s))
        super(bnmtf_vb_observed, self)._push()

    def _run_device(self, it, orders, exptau, perf, terms, times):
        _lib.check(_lib.lib().bnmtf_otvb_run(self._handle(), it, _lib.ptr(orders), _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times)))

    def _run_finish(self, it, exptau, perf, terms, times):
        super(bnmtf_vb_observed, self)._run_finish(it, exptau, perf, terms, times)
        if it > 0:          # (the exptau the device holds now is the fp64 one this was formed from: the next run() uploads nothing)
            self._device_state = (self._device_state[0], float(self.exptau), self._device_state[2])

    def _update(self, which, k, l, moments):
        self._push()
        _lib.check(_lib.lib().bnmtf_otvb_update(self._handle(), which, int(k), int(l), int(moments)))
        self._pull()

    def exp_square_diff(self):
        """:235-239 (fp64 on the device, all four terms per observed entry)."""
        self._push()
        out = C.c_double()
        _lib.check(_lib.lib().bnmtf_otvb_exp_square_diff(self._handle(), C.byref(out)))
        return out.value

    def _metric_sums(self, M_pred, A, S, B):
        return _observed.tri_metric_sums(self, M_pred, self.expF if A is None else A, self.expS if S is None else S, self.expG if B is None else B)
