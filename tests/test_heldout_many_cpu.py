"""run_many(..., M_tests=): what needs no device -- the signature, and that the list of masks is validated for every model before
anything reaches the device (NMF / NMTF create their handle at the first device call: a model that was refused has none)."""
import inspect

import numpy as np
import pytest

from bnmtf_amd import NMF, NMTF, run_many


def _models():
    rs = np.random.RandomState(1)
    out = []
    for I, J, K, L in [(20, 15, 3, 0), (12, 18, 2, 4)]:
        R = rs.exponential(1.0, (I, J)) + 0.01
        M = np.ones((I, J)); M[0, 1] = 0
        np.random.seed(2)
        if L:
            m = NMTF(R, M, K, L, verbose=False); m.initialise('random', 'random')
        else:
            m = NMF(R, M, K, verbose=False); m.initialise('random')
        out.append(m)
    return out


def test_M_tests_is_the_last_argument_and_defaults_to_None():
    params = list(inspect.signature(run_many).parameters.values())
    assert params[-1].name == "M_tests" and params[-1].default is None
    assert [p.name for p in params[:6]] == ["models", "iterations", "update", "store_samples", "expectation", "orders"]
    for cls in (NMF, NMTF):
        p = inspect.signature(cls.run).parameters["M_test"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("M_tests, error", [
    (lambda ms: [np.ones(ms[0].R.shape)], ValueError),                                        # one mask for two models
    (lambda ms: [None, None, None], ValueError),
    (lambda ms: [np.ones(ms[0].R.shape), np.ones((3, 3))], AssertionError),                   # the second model's has the wrong shape
    (lambda ms: [np.ones(ms[0].R.shape), np.zeros(ms[1].R.shape)], AssertionError),           # ... no entries
    (lambda ms: [np.ones(ms[0].R.shape), np.full(ms[1].R.shape, 2.0)], AssertionError),       # ... is not 0/1
], ids=["short", "long", "shape", "empty", "not 0/1"])
def test_the_masks_of_all_models_are_checked_before_any_device_call(M_tests, error):
    ms = _models()
    U0 = ms[0].U.copy()
    with pytest.raises(error):
        run_many(ms, 3, M_tests=M_tests(ms))
    assert all(m._h is None for m in ms)                # no handle: nothing reached the device
    assert np.array_equal(ms[0].U, U0) and not hasattr(ms[0], "all_performances_test")
