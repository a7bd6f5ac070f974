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
from . import _observed
from .bnmf_vb import bnmf_vb_optimised


class bnmf_vb_observed(_observed.ObservedVB, bnmf_vb_optimised):
    _OBSERVED = {"set_state": "bnmf_vbo_set_state", "get_state": "bnmf_vbo_get_state", "run": "bnmf_vbo_run", "update": "bnmf_vbo_update",
                 "exp_square_diff": "bnmf_vbo_exp_square_diff", "create": _observed.create_handle, "metric_sums": _observed.metric_sums}

    def __init__(self, R, M, K, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None):
        self._layout = 'observed'
        self.K = K
        (self.I, self.J), self.size_Omega = _observed.take_R_M(self, R, M)      # (dense arrays, or an Entries and None)
        _observed.check_constructor(self, world)
        self._init_priors(priors, device, verbose, rank, world, comm_id)
        self._blocks = None                                     # (the layout ties no rank to a lane: one handle up to 256)
