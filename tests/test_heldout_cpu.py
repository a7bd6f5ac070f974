"""Host side of run(..., M_test=): the argument checks and refusals that happen before any device call, the keyword's place in
the six run() signatures, the two entry points in the header and the binding.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import bnmtf_amd
from bnmtf_amd import (_lib, bnmf_gibbs_optimised, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_optimised, nmf_icm,
                       nmtf_icm)
from bnmtf_amd._base import compute_MSE, compute_R2, compute_Rp, metrics_from_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRI2 = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
PRI3 = dict(alpha=1., beta=1., lambdaF=0.1, lambdaS=0.1, lambdaG=0.1)
I, J = 6, 5


def _models(K=2, **kw):
    R = np.arange(1.0, I * J + 1).reshape(I, J); M = np.ones((I, J))
    return [bnmf_gibbs_optimised(R, M, K, PRI2, verbose=False, **kw), nmf_icm(R, M, K, PRI2, verbose=False, **kw),
            bnmf_vb_optimised(R, M, K, PRI2, verbose=False, **kw), bnmtf_gibbs_optimised(R, M, K, 3, PRI3, verbose=False, **kw),
            nmtf_icm(R, M, K, 3, PRI3, verbose=False, **kw), bnmtf_vb_optimised(R, M, K, 3, PRI3, verbose=False, **kw)]


class _NoDevice(object):
    """Any attempt to reach the library fails the test: the checks below come before every device call."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the argument checks" % name)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoDevice())


def test_M_test_is_keyword_only_on_the_six_classes():
    for cls in (bnmf_gibbs_optimised, bnmtf_gibbs_optimised, nmf_icm, nmtf_icm, bnmf_vb_optimised, bnmtf_vb_optimised):
        p = inspect.signature(cls.run).parameters["M_test"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, cls.__name__
    # run_many takes none
    assert "M_test" not in inspect.signature(bnmtf_amd.run_many).parameters


def test_wrong_shape_is_an_assertion_before_any_device_call(no_device):
    for m in _models():
        with pytest.raises(AssertionError) as e:
            m.run(2, M_test=np.ones((I, J + 1)))
        assert str(e.value) == ("Input matrix R is not of the same size as the held-out indicator matrix M_test: "
                                "(6, 5) and (6, 6) respectively."), type(m).__name__


def test_empty_mask_and_values_other_than_0_1_are_assertions(no_device):
    for m in _models():
        with pytest.raises(AssertionError) as e:
            m.run(2, M_test=np.zeros((I, J)))
        assert str(e.value) == "The held-out indicator matrix M_test has no entries."
        with pytest.raises(AssertionError) as e:
            m.run(2, M_test=2.0 * np.ones((I, J)))
        assert str(e.value) == "The indicator matrix M_test must contain only 0 and 1."


def test_a_model_in_column_blocks_is_refused(no_device):
    R = np.ones((70, 66)); M = np.ones((70, 66)); Mt = np.zeros((70, 66)); Mt[3, 4] = 1
    for m in (bnmf_gibbs_optimised(R, M, 65, PRI2, verbose=False), nmf_icm(R, M, 65, PRI2, verbose=False),
              bnmf_vb_optimised(R, M, 65, PRI2, verbose=False), bnmtf_gibbs_optimised(R, M, 3, 65, PRI3, verbose=False)):
        assert m._blocks is not None
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Mt)
        assert "column blocks" in str(e.value) and "rank above 64" in str(e.value)
        assert not hasattr(m, "all_performances_test")


def test_a_sharded_model_is_refused(no_device):
    Mt = np.zeros((I, J)); Mt[1, 2] = 1
    for m in _models(rank=0, world=2, comm_id=bytes(128)):
        with pytest.raises(bnmtf_amd.BnmtfError) as e:
            m.run(2, M_test=Mt)
        assert "sharded" in str(e.value) and "world = 2" in str(e.value)


def test_the_mask_handed_to_the_library_is_contiguous_fp64_and_None_stays_None():
    m = _models()[0]
    assert m._check_heldout(None) is None
    Mt = (np.arange(I * J).reshape(J, I).T % 3 == 0)          # bool, not contiguous
    got = m._check_heldout(Mt)
    assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, Mt.astype(float))
    got = m._check_heldout(Mt.astype(int).tolist())            # nested lists, as predict() takes them
    assert np.array_equal(got, Mt.astype(float))


def test_six_sums_finish_to_the_reference_formulas():
    """all_performances_test is metrics_from_sums of the device's six sums: the same quantities as compute_MSE / R2 / Rp."""
    rs = np.random.RandomState(5)
    R = rs.rand(I, J) * 4; P = rs.rand(I, J) * 4; Mt = (rs.rand(I, J) < 0.5).astype(float)
    s = [Mt.sum(), (Mt * R).sum(), (Mt * R * R).sum(), (Mt * P).sum(), (Mt * P * P).sum(), (Mt * R * P).sum()]
    got = metrics_from_sums(s)
    np.testing.assert_allclose([got["MSE"], got["R^2"], got["Rp"]], [compute_MSE(Mt, R, P), compute_R2(Mt, R, P), compute_Rp(Mt, R, P)], rtol=1e-12)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "bnmtf_hip.h")).read()
    assert re.search(r"^BNMTF_API int bnmtf_set_heldout\(bnmtf_handle h, const double\* M_test\);", hdr, flags=re.M)
    assert re.search(r"^BNMTF_API int bnmtf_get_heldout\(bnmtf_handle h, int n_iter, double\* sums_out\);", hdr, flags=re.M)
    assert "bnmtf_set_heldout" in _lib.EXPORTS and "bnmtf_get_heldout" in _lib.EXPORTS
    lib = bnmtf_amd.lib()
    assert hasattr(lib, "bnmtf_set_heldout") and hasattr(lib, "bnmtf_get_heldout")
    # a null handle is an error code, not a crash (function-try-block guard and argument check)
    assert lib.bnmtf_set_heldout(None, None) == -1
    assert lib.bnmtf_get_heldout(None, 1, None) == -1
