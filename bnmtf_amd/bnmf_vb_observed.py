"""bnmf_vb_observed: the variational two-factor model (bnmf_vb_optimised) on the observed-entry layout.

    BNMF = bnmf_vb_observed(R, M, K, priors)
    BNMF.initialise(init='exp', tauUV={})
    BNMF.run(iterations)

The API, the attributes and the assertion messages of bnmf_vb_optimised.  The device keeps the residual R_ij - E[U_i].E[V_j] on
the OBSERVED entries (csrc/kernel_obs_vb.hip), so cost and device memory follow the number of observed entries: the class for
matrices that are mostly missing.  The matrix is given as dense arrays R, M or as lists, bnmf_vb_observed(Entries, None, K, priors)
(entries.py: nothing of size I x J on the host); run(M_test=Entries) keeps the held-out curve of E[U] E[V]^T in
all_performances_test.  Ranks up to 256 on one handle (no column blocks), one GPU; no masked_sums, run_many, set_sweep_path /
set_small_path / set_profiling.  A class of its own, not a keyword of bnmf_vb_optimised: that class keeps refusing layout=."""
import ctypes as C

import numpy as np

from . import _lib, _observed
from ._base import broadcast_lambda
from .bnmf_vb import bnmf_vb_optimised


class bnmf_vb_observed(_observed.ObservedVB, bnmf_vb_optimised):
    _SET_STATE, _GET_STATE = "bnmf_vbo_set_state", "bnmf_vbo_get_state"

    def __init__(self, R, M, K, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None):
        self._layout = 'observed'
        self.K = K
        (self.I, self.J), self.size_Omega = _observed.take_R_M(self, R, M)      # (dense arrays, or an Entries and None)
        _observed.check_constructor(self, world)
        self.alpha, self.beta = float(priors['alpha']), float(priors['beta'])
        self.lambdaU = broadcast_lambda(priors['lambdaU'], (self.I, self.K), "lambdaU")
        self.lambdaV = broadcast_lambda(priors['lambdaV'], (self.J, self.K), "lambdaV")
        self.verbose = verbose
        self._init_device(0, device, rank, world, comm_id)      # VB draws nothing: the key is unused
        self._blocks = None                                     # (the layout ties no rank to a lane: one handle up to 256)

    def _handle(self):
        if self._h is None:
            self._h = _observed.create_handle(self)
        return self._h

    def _shapes(self):
        return [(self.I, self.K)] * 4 + [(self.J, self.K)] * 4

    def _run_device(self, it, exptau, perf, terms, times):
        _lib.check(_lib.lib().bnmf_vbo_run(self._handle(), it, _lib.ptr(exptau), _lib.ptr(perf), _lib.ptr(terms), _lib.ptr(times)))

    def _update(self, which, k, moments):
        self._push()
        _lib.check(_lib.lib().bnmf_vbo_update(self._handle(), which, int(k), int(moments)))
        self._pull()

    def exp_square_diff(self):
        """:185-187 (fp64 on the device, over the observed entries)."""
        for n in ("muU", "tauU", "muV", "tauV"):          # the test-suite sets exp/var only
            if not hasattr(self, n):
                setattr(self, n, np.ones((self.I if n.endswith("U") else self.J, self.K)))
        self._push()
        out = C.c_double()
        _lib.check(_lib.lib().bnmf_vbo_exp_square_diff(self._handle(), C.byref(out)))
        return out.value

    def _metric_sums(self, M_pred, A, S, B):
        return _observed.metric_sums(self, M_pred, self.expU if A is None else A, self.expV if B is None else B)
