"""The public surface of the four variational classes, frozen: bnmf_vb_optimised and bnmtf_vb_optimised are drop-ins for the
reference's classes, bnmf_vb_observed and bnmtf_vb_observed the same on the observed-entry layout, and most of their methods live
in one shared base (bnmtf_amd/_variational.py).  Whatever moves between the base and the classes, these stay: the public method
names and their signatures, the constructors, _NAMES, the attributes of an instance after construction and after initialise, and
that the two dense classes refuse layout=.  The expected values are literals, read off the classes as they were before the shared
base existed.  No device: construction makes no handle, and the device calls of initialise -- the truncated-normal moments and
exp_square_diff -- are replaced."""
import inspect

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import _lib, _variational, batch

INIT2 = "(self, R, M, K, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None)"
INIT3 = "(self, R, M, K, L, priors, *, device=0, verbose=True, rank=0, world=1, comm_id=None)"

# what every one of the four has (DeviceModel's public methods among them)
COMMON = {
    'close': '(self)',
    'compute_MSE': '(self, M, R, R_pred)',
    'compute_R2': '(self, M, R, R_pred)',
    'compute_Rp': '(self, M, R, R_pred)',
    'describe': '(self)',
    'elbo': '(self)',
    'exp_square_diff': '(self)',
    'is_small': '(self)',
    'kernel_stats': '(self, kernel)',
    'log_likelihood': '(self)',
    'omega_counts': '(self)',
    'predict': '(self, M_pred)',
    'quality': '(self, metric)',
    'set_profiling': '(self, enable=True, kernel=None, every=1)',
    'set_small_path': "(self, on='auto')",
    'set_sweep_path': '(self, fast=True)',
    'update_exp_tau': '(self)',
    'update_tau': '(self)',
}
TWO = {
    'column_maxima': '(self, which)',
    'initialise': "(self, init='exp', tauUV={})",
    'masked_sums': '(self, which)',
    'run': '(self, iterations, *, M_test=None)',
    'train': "(self, iterations, init_UV='random')",
    'update_U': '(self, k)',
    'update_V': '(self, k)',
    'update_exp_U': '(self, k)',
    'update_exp_V': '(self, k)',
}
TRI = {
    'initialise': "(self, init_S='random', init_FG='random', tauFSG={})",
    'run': '(self, iterations, orders=None, *, M_test=None)',
    'train': '(self, init_S, init_FG, iterations)',
    'triple_dot': '(self, M1, M2, M3)',
    'update_F': '(self, k)',
    'update_G': '(self, l)',
    'update_S': '(self, k, l)',
    'update_exp_F': '(self, k)',
    'update_exp_G': '(self, l)',
    'update_exp_S': '(self, k, l)',
}
HOOKS = {'column_maxima': '(self, which)', 'masked_sums': '(self, which)'}       # (the observed tri class refuses them by name)

NAMES2 = ('muU', 'tauU', 'expU', 'varU', 'muV', 'tauV', 'expV', 'varV')
NAMES3 = ('muF', 'tauF', 'expF', 'varF', 'muS', 'tauS', 'expS', 'varS', 'muG', 'tauG', 'expG', 'varG')

ATTRS = ['I', 'J', 'K', 'M', 'R', '_comm_id', '_device', '_h', '_init_rs', '_rank', '_seed', '_world', 'alpha', 'beta', 'size_Omega', 'verbose']
ATTRS2 = ATTRS + ['_blocks', 'lambdaU', 'lambdaV']
ATTRS3 = ATTRS + ['L', 'lambdaF', 'lambdaG', 'lambdaS']
TAU = ['alpha_s', 'beta_s', 'explogtau', 'exptau']

PRI2 = dict(alpha=1.0, beta=1.0, lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1.0, beta=1.0, lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)

# class name -> (constructor, public methods, properties, _NAMES, attributes after construction, ranks and priors of a 6 x 5 model,
#                the arguments of initialise with the expectations at the prior means, ... drawn, the kind run_many knows it by)
SURFACE = {
    'bnmf_vb_optimised': (INIT2, dict(COMMON, **TWO), ['all_elbo'], NAMES2, ATTRS2, (2, PRI2), ('exp',), ('random',), "vb"),
    'bnmtf_vb_optimised': (INIT3, dict(COMMON, **TRI), [], NAMES3, ATTRS3, (2, 3, PRI3), ('exp', 'exp'), ('random', 'random'), "trivb"),
    'bnmf_vb_observed': (INIT2, dict(COMMON, **TWO), ['all_elbo'], NAMES2, ATTRS2 + ['_layout'], (2, PRI2), ('exp',), ('random',), "vb"),
    'bnmtf_vb_observed': (INIT3, dict(COMMON, **TRI, **HOOKS), [], NAMES3, ATTRS3 + ['_blocks', '_layout'], (2, 3, PRI3), ('exp', 'exp'),
                          ('random', 'random'), "trivb"),
}


class _NoDevice(object):
    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_public_methods_signatures_and_names(name):
    init, methods, props, names = SURFACE[name][:4]
    cls = getattr(bnmtf_amd, name)
    assert str(inspect.signature(cls.__init__)) == init
    found = {n: str(inspect.signature(f)) for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}
    assert sorted(found) == sorted(methods)
    assert found == methods
    assert [n for n, _ in inspect.getmembers(cls, lambda x: isinstance(x, property))] == props
    assert cls._NAMES == names and isinstance(cls._NAMES, tuple)
    assert issubclass(cls, _variational.Variational)


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_attributes_after_construction_and_initialise(name, monkeypatch):
    _, _, _, names, attrs, args, at_mean, drawn, _ = SURFACE[name]
    cls = getattr(bnmtf_amd, name)
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())
    monkeypatch.setattr(cls, "exp_square_diff", lambda self: 4.0)
    moments = lambda mus, taus, device=0: (np.asarray(mus, dtype=float) + 1.0, np.asarray(taus, dtype=float) + 2.0)
    for module in (_variational, bnmtf_amd.distributions):
        monkeypatch.setattr(module, "_moments", moments)
    R = np.arange(30, dtype=float).reshape(6, 5) + 1.0
    m = cls(R, np.ones((6, 5)), *args, verbose=False)
    assert sorted(vars(m)) == sorted(attrs)
    assert m._h is None and getattr(m, "_blocks", None) is None
    assert getattr(m, "_layout", "dense") == ('observed' if name.endswith("observed") else 'dense')
    for how in (at_mean, drawn):
        m.initialise(*how)
        assert sorted(vars(m)) == sorted(attrs + list(names) + TAU)
        assert m._h is None
        # alpha_s = 1 + 30 / 2, beta_s = 1 + 4 / 2
        assert (m.alpha_s, m.beta_s, m.exptau) == (16.0, 3.0, 16.0 / 3.0)
        for n, shape in zip(names, [s for s in ((6, 2), (2, 3), (5, 3)) for _ in range(4)] if len(names) == 12 else [(6, 2)] * 4 + [(5, 2)] * 4):
            assert getattr(m, n).shape == shape and getattr(m, n).dtype == np.float64, n
    m.initialise(*at_mean)
    for f in names[0][len("mu"):], names[-1][len("var"):]:
        assert (getattr(m, "mu" + f) == 10.0).all() and (getattr(m, "tau" + f) == 1.0).all()
        assert (getattr(m, "exp" + f) == 11.0).all() and (getattr(m, "var" + f) == 3.0).all()


@pytest.mark.parametrize("name", ["bnmf_vb_optimised", "bnmtf_vb_optimised"])
def test_the_dense_classes_keep_refusing_layout(name):
    args = SURFACE[name][5]
    cls = getattr(bnmtf_amd, name)
    assert "layout" not in inspect.signature(cls.__init__).parameters
    with pytest.raises(TypeError):
        cls(np.ones((6, 5)), np.ones((6, 5)), *args, verbose=False, layout='observed')
    with pytest.raises(TypeError):
        cls(np.ones((6, 5)), np.ones((6, 5)), *args, verbose=False, layout='dense')


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_run_many_knows_the_four_by_their_dense_class(name):
    args, kind = SURFACE[name][5], SURFACE[name][8]
    m = getattr(bnmtf_amd, name)(np.ones((6, 5)), np.ones((6, 5)), *args, verbose=False)
    assert batch.takes(m) is True and batch._kind(m) == kind
