"""Drop-in for code/models/nmf_icm.py (class nmf_icm): Iterated Conditional Modes for MAP
non-negative matrix factorisation.  Same conditional parameters as the Gibbs sampler
(tauU/muU/tauV/muV, nmf_icm.py:159-169), but every update takes the mode of the truncated
normal, max(0, mu), clamped from below by minimum_TN (:128-135), and tau takes the Gamma
mode (alpha_s - 1) / beta_s (:137, distributions/gamma.py:27-29).  The whole trajectory is
deterministic, so it is compared with the reference end to end.

    NMF = nmf_icm(R, M, K, priors)
    NMF.initialise(init)                    # 'random' | 'exp'
    NMF.run(iterations, minimum_TN=0.)      # fills all_tau, all_times, all_performances
    NMF.predict(M_pred); NMF.quality(metric)
"""
from ._sampler import ICMRules
from .bnmf_gibbs import bnmf_gibbs_optimised


def gamma_mode(alpha, beta):
    """distributions/gamma.py:27-29."""
    return (float(alpha) - 1) / float(beta)


class nmf_icm(ICMRules, bnmf_gibbs_optimised):
    def initialise(self, init='random'):
        """:93-111 ('random' consumes numpy.random.exponential in the reference's (i,k) order)."""
        assert init in ['random', 'exp'], "Unknown initialisation option: %s. Should be 'random' or 'exp'." % init
        if init == 'random':
            self.U = self._rng().exponential(scale=1.0 / self.lambdaU)
            self.V = self._rng().exponential(scale=1.0 / self.lambdaV)
        else:
            self.U = 1.0 / self.lambdaU
            self.V = 1.0 / self.lambdaV
        self.tau = gamma_mode(self.alpha_s(), self.beta_s())
