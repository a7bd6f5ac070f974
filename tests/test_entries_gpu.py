"""List input on the observed-entry layout (bnmtf_amd.Entries) on the device: a model built from an Entries is,
bit for bit, the model built from the dense pair; predict() takes either form; and a matrix whose dense form no host could hold is
constructed, run and predicted on."""
import numpy as np
import pytest

from bnmtf_amd import Entries, bnmf_gibbs_optimised, bnmf_vb_observed, nmf_icm
from bnmtf_amd.synthetic import generate_bnmf

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
SEED_DATA, SEED_MASK = 3, 0      # tests/test_obs_gpu.py: generate_bnmf(97, 83, 5) at 90 % missing, no row or column empty
KINDS = ("gibbs", "icm", "vb")


def _problem():
    R, M, _, _ = generate_bnmf(97, 83, 5, 0.9, seed_data=SEED_DATA, seed_mask=SEED_MASK)
    M = M.astype(float)
    assert M.sum(axis=0).min() > 0 and M.sum(axis=1).min() > 0
    Mp = ((np.random.RandomState(5).rand(97, 83) < 0.05) & (M == 0)).astype(float)
    return R.astype(np.float64), M, Mp


def _fit(kind, R, M, Mp):
    """One fitted model and everything the issue lists of it, as a dict of arrays and floats."""
    np.random.seed(11)
    out = {}
    if kind == "gibbs":
        m = bnmf_gibbs_optimised(R, M, 5, PRI, seed=123, verbose=False, layout='observed')
        m.initialise('random')
        m.run(6)
        out.update(all_U=m.all_U, all_V=m.all_V, U=m.U, V=m.V, tau=m.tau)
        out.update(predict=m.predict(Mp, 2, 1), MSE=m.quality('MSE', 2, 1), BIC=m.quality('BIC', 2, 1))
    elif kind == "icm":
        m = nmf_icm(R, M, 5, PRI, verbose=False, layout='observed')
        m.initialise('random')
        m.run(6)
        out.update(U=m.U, V=m.V, tau=m.tau, predict=m.predict(Mp), MSE=m.quality('MSE'), BIC=m.quality('BIC'))
    else:
        m = bnmf_vb_observed(R, M, 5, PRI, verbose=False)
        m.initialise('random')
        m.run(6)
        out.update({n: getattr(m, n) for n in m._NAMES})
        out.update(all_tau=m.all_exp_tau, predict=m.predict(Mp), MSE=m.quality('MSE'), BIC=m.quality('BIC'), ELBO=m.quality('ELBO'))
    if kind != "vb":
        out["all_tau"] = m.all_tau
    out["perf"] = m.all_performances
    out["omega"] = m.omega_counts()
    m.close()
    return out


def _same_bits(a, b, where):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            assert sorted(x) == sorted(y)
            for n in x:
                assert np.array_equal(np.asarray(x[n], dtype=np.float64).view(np.uint64), np.asarray(y[n], dtype=np.float64).view(np.uint64)), (where, k, n)
        elif isinstance(x, tuple):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), (where, k)
        else:
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (where, k)


@pytest.fixture(scope="module")
def dense_fits():
    """the models built from (R, M), predicting on a dense mask: code paths as they were before Entries existed"""
    R, M, Mp = _problem()
    return {kind: _fit(kind, R, M, Mp) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_a_model_built_from_entries_is_the_dense_input_model_bit_for_bit(dense_fits, kind):
    R, M, Mp = _problem()
    E, Ep = Entries.from_dense(R, M), Entries.from_dense(R, Mp)
    _same_bits(_fit(kind, E, None, Ep), dense_fits[kind], kind)
    # ... and so is the one built from the same entries in another order
    order = np.random.RandomState(7).permutation(len(E))
    S = Entries(E.shape, E.rows[order], E.cols[order], E.values[order])
    order = np.random.RandomState(8).permutation(len(Ep))
    Sp = Entries(Ep.shape, Ep.rows[order], Ep.cols[order], Ep.values[order])
    _same_bits(_fit(kind, S, None, Sp), dense_fits[kind], kind + ", shuffled")


@pytest.mark.parametrize("kind", KINDS)
def test_predict_takes_entries_on_a_dense_input_model(dense_fits, kind):
    R, M, Mp = _problem()
    got = _fit(kind, R, M, Entries.from_dense(R, Mp))
    _same_bits(got, dense_fits[kind], kind)


def test_a_matrix_no_host_could_hold_densely_runs_from_its_entries():
    """200 000 x 150 000 with 600 000 entries (dense R in fp64: 240 GB): a cyclic diagonal, so that every row and column has an
    entry, plus random fill; two ICM iterations and predict() on a list of 1 000 entries."""
    n_i, n_j, K = 200000, 150000, 4
    rs = np.random.RandomState(0)
    d = np.arange(n_i, dtype=np.int64)
    flat = np.unique(np.concatenate([d * n_j + d % n_j, rs.randint(0, n_i, 600000 - n_i).astype(np.int64) * n_j + rs.randint(0, n_j, 600000 - n_i)]))
    E = Entries((n_i, n_j), flat // n_j, flat % n_j, rs.exponential(1.0, len(flat)))
    m = nmf_icm(E, None, K, PRI, verbose=False, layout='observed')
    tot, per_row, per_col = m.omega_counts()
    assert tot == len(E) == m.size_Omega and per_row.min() >= 1 and per_col.min() >= 1
    np.random.seed(3)
    m.initialise('random')
    m.run(2)
    assert m.U.shape == (n_i, K) and m.V.shape == (n_j, K) and np.isfinite(m.U).all() and np.isfinite(m.V).all()
    assert len(m.all_performances['MSE']) == 2 and np.isfinite(m.all_performances['MSE']).all()
    pick = rs.choice(len(E), 1000, replace=False)
    Ep = Entries(E.shape, E.rows[pick], E.cols[pick], E.values[pick])
    got = m.predict(Ep)
    # fp64 NumPy on the pulled factors (which hold the device's fp32 values exactly) and the fp32 values the device is handed
    p = np.einsum('ek,ek->e', m.U[Ep.rows], m.V[Ep.cols])
    r = Ep.values32().astype(np.float64)
    np.testing.assert_allclose(got['MSE'], ((r - p) ** 2).mean(), rtol=1e-9)
    m.close()
