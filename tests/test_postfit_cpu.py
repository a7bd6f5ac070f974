"""bnmtf_amd._postfit, what posterior_predictive, top_entries and fold_in share: the class dispatch over the ten exported classes,
the texts of the two users of the entry-list check, and the finish of the shifted moments.  No GPU needed."""
import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (NMF, NMTF, _lib, _postfit, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised,
                       bnmtf_vb_observed, bnmtf_vb_optimised, nmf_icm, nmtf_icm)
from bnmtf_amd._sampler import GibbsSampler, ICMRules
from bnmtf_amd._variational import Variational
from bnmtf_amd.nmf_np import NPDevice

PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5


class _NoDevice(object):
    """Any attempt to reach the library fails the test."""

    def __getattr__(self, name):
        raise AssertionError("device call %s" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def test_kind_of_is_the_dispatch_of_the_three_calls(no_device):
    rs = np.random.RandomState(0)
    M = (rs.rand(I, J) < 0.5).astype(float)
    M[np.arange(I), np.arange(I) % J] = 1; M[np.arange(J) % I, np.arange(J)] = 1
    R = rs.rand(I, J) * 3 + 0.1
    want = {bnmf_gibbs_optimised: 'gibbs', bnmtf_gibbs_optimised: 'gibbs', nmf_icm: 'icm', nmtf_icm: 'icm',
            bnmf_vb_optimised: 'variational', bnmtf_vb_optimised: 'variational', bnmf_vb_observed: 'variational',
            bnmtf_vb_observed: 'variational', NMF: 'np', NMTF: 'np'}
    assert len(want) == 10 and all(getattr(bnmtf_amd, c.__name__) is c and c.__name__ in bnmtf_amd.__all__ for c in want)
    for cls, kind in want.items():
        tri = cls in (bnmtf_gibbs_optimised, nmtf_icm, bnmtf_vb_optimised, bnmtf_vb_observed, NMTF)
        ranks = (2, 2) if tri else (2,)
        prior = () if kind == 'np' else (PRI3 if tri else PRI,)
        layouts = ({}, {"layout": 'observed'}) if cls in (bnmf_gibbs_optimised, bnmtf_gibbs_optimised, nmf_icm, NMF, NMTF) else ({},)
        for kw in layouts:
            m = cls(R, M, *ranks, *prior, verbose=False, **kw)
            assert _postfit.kind_of(m) == kind, (cls.__name__, kw)
            # the expressions the three calls branched on before they shared this one
            gibbs = isinstance(m, GibbsSampler) and not isinstance(m, ICMRules)
            assert gibbs == (kind == 'gibbs')
            assert isinstance(m, Variational) == (kind == 'variational') and isinstance(m, NPDevice) == (kind == 'np')
            assert isinstance(m, (ICMRules, NPDevice)) == (kind in ('icm', 'np'))
            assert (isinstance(m, ICMRules) and isinstance(m, GibbsSampler)) == (kind == 'icm')
            assert isinstance(m, (GibbsSampler, Variational, NPDevice))
            assert _postfit.device_of(m, None) == 0 and _postfit.device_of(m, 3) == 3
    for other in (object(), 3, None, np.ones((2, 2))):
        assert _postfit.kind_of(other) is None


def _text(*args, **kw):
    with pytest.raises(bnmtf_amd.BnmtfError) as e:
        _postfit.entry_lists("who", (I, J), *args, **kw)
    return str(e.value)


def test_entry_lists_keeps_the_texts_of_both_users():
    plain, excluded = {}, dict(noun="excluded ", bits=32, empty=True)
    for kw, rows, cols, entry in ((plain, "rows", "cols", "entry"), (excluded, "the excluded rows", "the excluded cols", "excluded entry")):
        assert _text([[0, 1]], [0, 1], **kw) == "who: %s is one-dimensional, not 2-dimensional" % rows
        assert _text([0, 1], 3, **kw) == "who: %s is one-dimensional, not 0-dimensional" % cols
        assert _text([0.5, 1], [0, 1], **kw) == "who: %s holds integers, not float64" % rows
        assert _text([0, 1], np.array([0, 1], dtype=np.float32), **kw) == "who: %s holds integers, not float32" % cols
        assert _text([[0.5]], [0.5], **kw) == "who: %s is one-dimensional, not 2-dimensional" % rows          # (rows first, shape before type)
        assert _text([0, 1], [0], **kw) == "who: %s and cols have different lengths: 2 and 1" % rows
        assert _text([0, I], [0, 1], **kw) == "who: %s 1 (6, 1) lies outside the 6 x 5 matrix" % entry
        assert _text([0, 1], [-1, J], **kw) == "who: %s 0 (0, -1) lies outside the 6 x 5 matrix" % entry
        assert _text([0, 1, 2], [0], **kw).endswith("different lengths: 3 and 1")                            # (lengths before the range)
    assert _text([], []) == "who: the list of entries is empty"
    assert _text(np.zeros(0), np.zeros(0)) == "who: the list of entries is empty"                            # (an empty list has no type)
    for empty in ([], np.zeros(0)):
        er, ec = _postfit.entry_lists("who", (I, J), empty, empty, **excluded)
        assert er.dtype == ec.dtype == np.int32 and er.shape == ec.shape == (0,)

    # the length limits, on views that take no memory: 2^31 - 1 entries against 2^32 - 1
    def long_list(n):
        return np.broadcast_to(np.zeros(1, dtype=np.int8), (n,))

    assert _text(long_list(2 ** 31), long_list(2 ** 31)) == "who: at most 2^31 - 1 entries (%d given)" % 2 ** 31
    assert _text(long_list(2 ** 32), long_list(2 ** 32), **excluded) == "who: at most 2^32 - 1 excluded entries (%d given)" % 2 ** 32

    rows, cols = _postfit.entry_lists("who", (I, J), np.array([5, 0, 5], dtype=np.int64), [4, 0, 4])
    assert rows.dtype == cols.dtype == np.int32 and rows.flags["C_CONTIGUOUS"] and rows.tolist() == [5, 0, 5] and cols.tolist() == [4, 0, 4]
    strided = np.arange(12, dtype=np.int64)[::3]
    rows, cols = _postfit.entry_lists("who", (I, J), strided % I, strided % J)
    assert rows.flags["C_CONTIGUOUS"] and cols.flags["C_CONTIGUOUS"] and rows.tolist() == [0, 3, 0, 3] and cols.tolist() == [0, 3, 1, 4]


def test_shifted_moments_are_the_two_formulas_and_clamp_at_zero():
    # three values that differ from the first by d: the mean of d squared rounds below the square of the mean of d
    first = np.array([2.0, 1e9, 5.0])
    d = np.array([0.1, 0.3, 0.0])
    count = 3
    sum_d, sum_d2 = d * count, np.array([(0.1 * 0.1) * count, (0.3 * 0.3) * count * (1 - 2.0 ** -52), 0.0])
    md = sum_d / count
    raw = sum_d2 / count - md * md
    assert (raw < 0).any() and (raw > -1e-15).all()                    # (slightly negative: what the clamp is for)
    mean, variance = _postfit.shifted_moments(first, sum_d, sum_d2, count)
    assert mean.tobytes() == (first + md).tobytes()
    assert variance.tobytes() == np.maximum(0.0, raw).tobytes()
    assert (variance >= 0).all() and variance[raw < 0].tolist() == [0.0] * int((raw < 0).sum())
    # a spread the formula keeps: the same on a matrix, as fold_in gives it
    S, S2 = np.array([[1.0, 4.0]]), np.array([[3.0, 10.0]])
    mean, variance = _postfit.shifted_moments(np.array([[1.0, -1.0]]), S, S2, 2)
    assert mean.tolist() == [[1.5, 1.0]] and variance.tolist() == [[1.25, 1.0]]
