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
import numpy as np

from . import _observed
from ._base import check_R_M
from .bnmtf_vb import bnmtf_vb_optimised


class bnmtf_vb_observed(_observed.ObservedVB, bnmtf_vb_optimised):
    _OBSERVED = {"set_state": "bnmtf_otvb_set_state", "get_state": "bnmtf_otvb_get_state", "run": "bnmtf_otvb_run",
                 "update": "bnmtf_otvb_update", "exp_square_diff": "bnmtf_otvb_exp_square_diff",
                 "create": _observed.create_tri_handle, "metric_sums": _observed.tri_metric_sums}
    _KEEPS_DEVICE_STATE = True          # (the observed-entry handle: run(a); run(b) is the trajectory of run(a + b))

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
        self._init_priors(priors, device, verbose, rank, world, comm_id)
        self._blocks = None
