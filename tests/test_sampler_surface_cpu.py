"""The public surface of the four sampler classes, frozen: bnmf_gibbs_optimised, bnmtf_gibbs_optimised, nmf_icm and nmtf_icm are
drop-ins for the reference's classes, and most of their methods live in one shared base (bnmtf_amd/_sampler.py).  Whatever moves
between the base and the classes, these stay: the public method names and their signatures, the attributes of an instance after
construction and after initialise, the two signatures of _cond, and what run_many takes.  The expected values are literals, read
off the classes as they were before the shared base existed.  No device: construction makes no handle, and beta_s -- the one
device call of initialise -- is replaced."""
import inspect

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import batch

INIT2 = "(self, R, M, K, priors, *, seed=None, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense')"
INIT3 = "(self, R, M, K, L, priors, *, seed=None, device=0, verbose=True, rank=0, world=1, comm_id=None, layout='dense')"

# what every one of the four has (DeviceModel's and ObservedLayout's public methods among them)
COMMON = {
    'alpha_s': '(self)',
    'approx_expectation': '(self, burn_in, thinning)',
    'beta_s': '(self)',
    'close': '(self)',
    'compute_MSE': '(self, M, R, R_pred)',
    'compute_R2': '(self, M, R, R_pred)',
    'compute_Rp': '(self, M, R, R_pred)',
    'describe': '(self)',
    'is_small': '(self)',
    'kernel_stats': '(self, kernel)',
    'omega_counts': '(self)',
    'predict_while_running': '(self)',
    'set_profiling': '(self, enable=True, kernel=None, every=1)',
    'set_small_path': "(self, on='auto')",
    'set_sweep_path': '(self, fast=True)',
    'train': '(self, init, iterations)',
}
TWO = {
    'initialise': "(self, init='random')",
    'muU': '(self, tauUk, k)',
    'muV': '(self, tauVk, k)',
    'tauU': '(self, k)',
    'tauV': '(self, k)',
}
TRI = {
    'initialise': "(self, init_S='random', init_FG='random')",
    'muF': '(self, tauFk, k)',
    'muG': '(self, tauGl, l)',
    'muS': '(self, tauSkl, k, l)',
    'tauF': '(self, k)',
    'tauG': '(self, l)',
    'tauS': '(self, k, l)',
    'triple_dot': '(self, M1, M2, M3)',
}
GIBBS = {
    'predict': '(self, M_pred, burn_in, thinning)',
    'quality': '(self, metric, burn_in, thinning)',
    'run': "(self, iterations, update='draw', store_samples=True, expectation=None, *, M_test=None)",
}
ICM = {
    'log_likelihood': '(self)',
    'predict': '(self, M_pred)',
    'quality': '(self, metric)',
    'run': '(self, iterations, minimum_TN=0.0, *, M_test=None)',
}

ATTRS = ['I', 'J', 'K', 'M', 'R', '_blocks', '_comm_id', '_device', '_h', '_init_rs', '_layout', '_rank', '_seed', '_world', 'alpha',
         'beta', 'size_Omega', 'verbose']
ATTRS2 = sorted(ATTRS + ['lambdaU', 'lambdaV'])
ATTRS3 = sorted(ATTRS + ['L', 'lambdaF', 'lambdaG', 'lambdaS'])

PRI2 = dict(alpha=1.0, beta=1.0, lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)

# class name -> (constructor, public methods, _cond, attributes after construction, those initialise adds, the ranks and priors
#                of a 6 x 5 model, tau after initialise('exp') with beta_s = 2, does run_many take it)
SURFACE = {
    'bnmf_gibbs_optimised': (INIT2, dict(COMMON, **TWO, **GIBBS, log_likelihood='(self, expU, expV, exptau)'), '(self, which, k)',
                             ATTRS2, ['U', 'V', 'tau'], (2, PRI2), 8.0, True),
    'bnmtf_gibbs_optimised': (INIT3, dict(COMMON, **TRI, **GIBBS, log_likelihood='(self, expF, expS, expG, exptau)'), '(self, which, k, l, n)',
                              ATTRS3, ['F', 'G', 'S', 'tau'], (2, 2, PRI3), 8.0, True),
    'nmf_icm': (INIT2, dict(COMMON, **TWO, **ICM), '(self, which, k)', ATTRS2, ['U', 'V', 'tau'], (2, PRI2), 7.5, False),
    'nmtf_icm': (INIT3, dict(COMMON, **TRI, **ICM), '(self, which, k, l, n)', ATTRS3, ['F', 'G', 'S', 'tau'], (2, 2, PRI3), 7.5, False),
}


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_public_methods_and_signatures(name):
    init, methods, cond, _, _, _, _, _ = SURFACE[name]
    cls = getattr(bnmtf_amd, name)
    assert str(inspect.signature(cls.__init__)) == init
    found = {n: str(inspect.signature(f)) for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}
    assert sorted(found) == sorted(methods)
    assert found == methods
    assert str(inspect.signature(cls._cond)) == cond


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_attributes_after_construction_and_initialise(name, monkeypatch):
    _, _, _, attrs, added, args, tau, _ = SURFACE[name]
    cls = getattr(bnmtf_amd, name)
    monkeypatch.setattr(cls, "beta_s", lambda self: 2.0)
    R = np.arange(30, dtype=float).reshape(6, 5) + 1.0
    m = cls(R, np.ones((6, 5)), *args, verbose=False)
    assert sorted(vars(m)) == attrs
    assert m._h is None and m._blocks is None
    m.initialise('exp')
    assert sorted(vars(m)) == sorted(attrs + added)
    assert m._h is None                               # (with beta_s replaced, initialise reaches no device either)
    assert m.tau == tau                               # alpha_s = 1 + 30 / 2: its ratio to beta_s, and the Gamma mode for ICM


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_run_many_takes_the_gibbs_classes_and_not_the_icm_ones(name):
    args, taken = SURFACE[name][5], SURFACE[name][7]
    m = getattr(bnmtf_amd, name)(np.ones((6, 5)), np.ones((6, 5)), *args, verbose=False)
    assert batch.takes(m) is taken
    kinds = {'bnmf_gibbs_optimised': "bnmf", 'bnmtf_gibbs_optimised': "bnmtf", 'nmf_icm': None, 'nmtf_icm': None}
    assert batch._kind(m) == kinds[name]              # (the two Gibbs classes share one run(): still told apart)
