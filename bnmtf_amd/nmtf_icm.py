"""Drop-in for code/models/nmtf_icm.py (class nmtf_icm): Iterated Conditional Modes for MAP
non-negative matrix tri-factorisation R ~ F.S.G^T.  Sweep order F columns, S row-major, G
columns, tau (nmtf_icm.py:141-162); every update is max(0, mu) clamped from below by
minimum_TN, tau is the Gamma mode.  Deterministic: compared with the reference end to end.
"""
from ._sampler import ICMRules
from .bnmtf_gibbs import bnmtf_gibbs_optimised
from .nmf_icm import gamma_mode


class nmtf_icm(ICMRules, bnmtf_gibbs_optimised):
    def initialise(self, init_S='random', init_FG='random'):
        """:100-128: the Gibbs class's initial F, S, G; tau = gamma_mode."""
        super().initialise(init_S=init_S, init_FG=init_FG)
        self.tau = gamma_mode(self.alpha_s(), self.beta_s())
