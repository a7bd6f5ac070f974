"""The non-probabilistic models' host side (bnmtf_amd.nmf_np.NMF, bnmtf_amd.nmtf_np.NMTF) without a GPU: the constructor
contract with the reference's assertion texts (its tests/code/test_nmf_np.py:14-58, test_nmtf_np.py:14-64), the initial
factors drawn from numpy.random as the reference draws them (tests/golden/np.npz, tests/golden/make_golden_np.py), the rank
bound and the refusals."""
import os

import numpy as np
import pytest

from bnmtf_amd import BnmtfError
from bnmtf_amd.nmf_np import NMF
from bnmtf_amd.nmtf_np import NMTF

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "np.npz"))
TOY = np.load(os.path.join(HERE, "golden", "toy_data.npz"))


def test_import_path_and_package_exports():
    import bnmtf_amd
    assert bnmtf_amd.NMF is NMF and bnmtf_amd.NMTF is NMTF


@pytest.mark.parametrize("make", [lambda R, M: NMF(R, M, 3), lambda R, M: NMTF(R, M, 3, 2)])
def test_constructor_assertions(make):
    with pytest.raises(AssertionError) as e:
        make(np.ones(3), np.ones(3))
    assert str(e.value) == "Input matrix R is not a two-dimensional array, but instead 1-dimensional."
    with pytest.raises(AssertionError) as e:
        make(np.ones((4, 3)), np.ones((3, 4)))
    assert str(e.value) == "Input matrix R is not of the same size as the indicator matrix M: (4, 3) and (3, 4) respectively."
    M = np.ones((3, 4)); M[1, :] = 0
    with pytest.raises(AssertionError) as e:
        make(np.ones((3, 4)), M)
    assert str(e.value) == "Fully unobserved row in R, row 1."
    M = np.ones((3, 4)); M[:, 2] = 0
    with pytest.raises(AssertionError) as e:
        make(np.ones((3, 4)), M)
    assert str(e.value) == "Fully unobserved column in R, column 2."


def test_constructor_attributes():
    R = np.arange(12.).reshape(3, 4); M = np.ones((3, 4)); M[0, 1] = 0
    n = NMF(R, M, 2, verbose=False)
    assert (n.I, n.J, n.K) == (3, 4, 2) and n.metrics == ['MSE', 'R^2', 'Rp']
    expect = R.copy(); expect[0, 1] = 1.
    assert np.array_equal(n.R_excl_unknown, expect)
    t = NMTF(R, M, 2, 3, verbose=False)
    assert (t.I, t.J, t.K, t.L) == (3, 4, 2, 3) and np.array_equal(t.R_excl_unknown, expect)


def test_nmf_initialise_draws_as_the_reference():
    R, M = TOY["bnmf/R"], TOY["bnmf/M"]
    for tag, init in [("nmf_rand", "random"), ("nmf_exp", "exponential")]:
        np.random.seed(int(G[tag + "/seed"]))
        n = NMF(R, M, 10, verbose=False)
        n.initialise(init, expo_prior=1.)
        assert np.array_equal(n.U, G[tag + "/U0"]) and np.array_equal(n.V, G[tag + "/V0"])
    n.initialise('ones')
    assert (n.U == 1).all() and (n.V == 1).all() and n.U.shape == (100, 10) and n.V.shape == (80, 10)
    with pytest.raises(AssertionError) as e:
        n.initialise('exp')
    assert str(e.value) == "Unrecognised init option for U,V: exp."


def test_nmtf_initialise_draws_as_the_reference():
    R, M = TOY["bnmtf/R"], TOY["bnmtf/M"]
    np.random.seed(int(G["nmtf_rand/seed"]))
    t = NMTF(R, M, 5, 5, verbose=False)
    t.initialise('random', 'random')
    for n in "SFG":
        assert np.array_equal(getattr(t, n), G["nmtf_rand/%s0" % n])
    np.random.seed(int(G["nmtf_expkm/seed"]))
    t.initialise('exponential', 'ones')              # S is drawn first: the same S as before the reference's k-means
    assert np.array_equal(t.S, G["nmtf_expkm/S0"]) and (t.F == 1).all() and (t.G == 1).all()
    with pytest.raises(AssertionError) as e:
        t.initialise('kmeans', 'random')
    assert str(e.value) == "Unrecognised init option for S: kmeans."
    with pytest.raises(AssertionError) as e:
        t.initialise('random', 'exp')
    assert str(e.value) == "Unrecognised init option for F,G: exp."


def test_run_before_initialise():
    R, M = np.ones((3, 4)), np.ones((3, 4))
    with pytest.raises(AssertionError) as e:
        NMF(R, M, 2).run(1)
    assert str(e.value) == "U and V have not been initialised - please run NMF.initialise() first."
    with pytest.raises(AssertionError) as e:
        NMTF(R, M, 2, 2).run(1)
    assert str(e.value) == "F, S and G have not been initialised - please run NMTF.initialise() first."


def test_rank_bound_and_one_gpu():
    R, M = np.ones((3, 4)), np.ones((3, 4))
    NMF(R, M, 256); NMTF(R, M, 256, 256)
    for make in [lambda: NMF(R, M, 257), lambda: NMF(R, M, 0), lambda: NMTF(R, M, 2, 257), lambda: NMTF(R, M, 257, 2)]:
        with pytest.raises(BnmtfError) as e:
            make()
        assert "is outside what this build runs" in str(e.value)
    with pytest.raises(BnmtfError) as e:
        NMF(R, M, 2, world=2)
    assert "one GPU" in str(e.value)
    with pytest.raises(BnmtfError):
        NMTF(R, M, 2, 2, rank=1, world=2)


def test_run_many_still_refuses_the_np_models():
    from bnmtf_amd import run_many
    R, M = np.ones((3, 4)), np.ones((3, 4))
    with pytest.raises(TypeError):
        run_many([NMF(R, M, 2)], 1)


@pytest.mark.parametrize("I,J", [(16385, 3), (3, 16385)])
def test_rows_and_columns_longer_than_16384_are_refused(I, J):
    """bnmtf_np_create refuses before any device call, so the refusal reads the same with or without a GPU."""
    R = np.ones((I, J)); M = np.ones((I, J))
    for m in (NMF(R, M, 2, verbose=False), NMTF(R, M, 2, 3, verbose=False)):
        m.U, m.V = np.ones((I, 2)), np.ones((J, 2))
        m.F, m.S, m.G = np.ones((I, 2)), np.ones((2, 3)), np.ones((J, 3))
        with pytest.raises(BnmtfError) as e:
            m.run(1)
        assert "at most 16384" in str(e.value)
        m.close()


@pytest.mark.parametrize("I,J", [(16384, 3), (3, 16384)])
def test_rows_and_columns_of_16384_pass_the_limit(I, J):
    """The limit's own value is accepted: without a GPU the call fails at the device, not at the shape check."""
    R = np.ones((I, J)); M = np.ones((I, J))
    n = NMF(R, M, 2, verbose=False)
    n.U, n.V = np.ones((I, 2)), np.ones((J, 2))
    try:
        n.run(1)
    except BnmtfError as e:
        assert "at most" not in str(e)
    n.close()
