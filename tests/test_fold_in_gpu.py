"""bnmtf_amd.fold_in on the device (csrc/kernel_foldin.hip): new units folded into a fixed factor, the whole
chain of a unit in one wave of one launch.

Launch shapes (tests/_fold_in_cases.py): (a) m = 1200, W = 3, eleven units of 1 .. 1100 entries -- every slot class of the register
form, both sides of its boundary to the long form, a last block of three units --; (b) m = 83, nine units, W = 1 .. 256.

Tolerances (derived, not measured).  A value of the mode chain: dmu = 2e-5 scale / tau_p + 1e-6 around max(0, mu), the bound the
project holds a half sweep's mu to (test_bnmf_gibbs_gpu.py; scale: the absolute-value sum of _draw_explainer._factor_pass), because
the residual is rebuilt at every sweep; where |mu| <= dmu either branch of the maximum is allowed, which the one inequality
|x - max(0, mu)| <= dmu says.  A draw: explained by the oracle's candidate sequence under _draw_explainer's tolerance model, with
at most _draw_cases.AMBIGUITY_CAP of the draws ambiguous.  Statistics: mean rtol 1e-9, the project's tolerance for fp64 device
sums; variance rtol 1e-9 plus atol 4 (T' + 4) 2^-53 dmax^2 -- test_predictive_gpu's derivation without its W term, because both
sides difference the same fp32 numbers.  W = 1: 5 standard errors of the mean and of the variance of 4000 i.i.d. draws."""
import ctypes as C

import numpy as np
import pytest

from bnmtf_amd import (Entries, _lib, bnmf_gibbs_optimised, bnmf_vb_observed, bnmf_vb_optimised, bnmtf_gibbs_optimised, bnmtf_vb_observed,
                       bnmtf_vb_optimised, fold_in, nmf_icm, nmtf_icm, top_entries)
import _draw_cases
import _fold_in_cases as cases

pytestmark = pytest.mark.gpu

NAMES = [s[0] for s in cases.SHAPES]
U53 = 2.0 ** -53


def _run(c, T=3, update='draw', new=None, **kw):
    kw.setdefault("ids", c.ids); kw.setdefault("seed", cases.SEED); kw.setdefault("store_samples", True)
    return fold_in.from_factors(c.other, c.new if new is None else new, c.lam, cases.TAU, T, update=update, **kw)


def _raw(c, T, form, discard=0, keep_every=1):
    """the C call itself: (first, sum_d, sum_d2, samples) as the library returns them"""
    unit, idx, val = c.new.row_major()
    first, sd, sd2 = np.zeros((c.n, c.W)), np.zeros((c.n, c.W)), np.zeros((c.n, c.W))
    samples = np.zeros((T, c.n, c.W), dtype=np.float32)
    p = _lib.ptr
    _lib.check(_lib.lib().bnmtf_fold_in(0, c.n, c.m, c.W, p(c.other), C.c_uint64(len(unit)), p(unit), p(idx), p(val), p(c.lam), cases.TAU, p(c.x0),
                                        p(c.ids), C.c_uint64(cases.SEED), T, 0, discard, keep_every, 0, 0.0, form, p(first), p(sd), p(sd2), p(samples)))
    return first, sd, sd2, samples


# ---------------------------------------------------------------- 1. the mode chain
@pytest.mark.parametrize("name", NAMES)
def test_mode_chain_conditioned_on_the_devices_own_states(name):
    c = cases.case(name)
    F = _run(c, 3, 'mode')
    assert F.samples.shape == (3, c.n, c.W) and F.samples.dtype == np.float32
    prev, worst = c.x0, 0.0
    for t in range(3):
        mu, tp, dmu = cases.conditionals(c, prev, F.samples[t])
        assert (tp > 0).all()
        worst = max(worst, float((np.abs(F.samples[t] - np.maximum(0.0, mu)) / dmu).max()))
        prev = F.samples[t]
    print("%s: largest |x - max(0, mu)| / dmu = %.3f" % (name, worst))
    assert worst <= 1.0
    assert F.count == 1 and (F.variance == 0.0).all() and F.mean.tobytes() == F.samples[-1].astype(np.float64).tobytes()
    # minimum_TN clamps from below
    G = _run(c, 2, 'mode', minimum_TN=0.75)
    assert (G.samples >= np.float32(0.75)).all()
    assert G.samples[0, :, 0].tobytes() == np.maximum(F.samples[0, :, 0], np.float32(0.75)).tobytes()       # (the first conditional of the chain is the same)


# ---------------------------------------------------------------- 2. every draw explained
@pytest.mark.parametrize("name", NAMES)
def test_every_draw_is_explained(name):
    c = cases.case(name)
    F = _run(c, 3, 'draw')
    e = cases.explain(c, F.samples)
    print("%s: draws %d unexplained %d ambiguous %d" % (name, e.draws, e.unexplained, e.ambiguous))
    assert e.draws == 3 * c.n * c.W
    assert e.unexplained == 0, e.offenders(5)
    assert e.ambiguous <= _draw_cases.AMBIGUITY_CAP * e.draws


# ---------------------------------------------------------------- 3. bits
def test_a_units_bits_depend_on_that_unit_alone():
    c = cases.case("a")
    F = _run(c, 3)
    # the form
    r0, r1 = _raw(c, 3, 0), _raw(c, 3, 1)
    for x, y in zip(r0, r1):
        assert x.tobytes() == y.tobytes()
    assert r0[3].tobytes() == F.samples.tobytes()
    assert _run(c, 3, form=1).samples.tobytes() == F.samples.tobytes()
    r0, r1 = _raw(c, 7, 0, 1, 2), _raw(c, 7, 1, 1, 2)
    for x, y in zip(r0, r1):
        assert x.tobytes() == y.tobytes()
    assert (r0[1] != 0).any() and (r0[2] > 0).any()
    # a unit alone, with its id
    for q in range(c.n):
        new, ids = c.unit(q)
        one = fold_in.from_factors(c.other, new, c.lam[q], cases.TAU, 3, ids=ids, seed=cases.SEED, store_samples=True)
        assert one.samples[:, 0].tobytes() == np.ascontiguousarray(F.samples[:, q]).tobytes(), q
        assert one.mean[0].tobytes() == F.mean[q].tobytes() and one.variance[0].tobytes() == F.variance[q].tobytes()
    # the order of the input list (c.new is shuffled), and a second call
    again, ordered = _run(c, 3), _run(c, 3, new=c.sorted)
    for G in (again, ordered):
        assert G.samples.tobytes() == F.samples.tobytes() and G.mean.tobytes() == F.mean.tobytes() and G.variance.tobytes() == F.variance.tobytes()
    # another seed, another id
    assert (_run(c, 3, seed=cases.SEED + 1).samples != F.samples).all(axis=2).any()
    moved = c.ids.copy(); moved[4] += 1
    other_id = _run(c, 3, ids=moved).samples
    assert (other_id[:, 4] != F.samples[:, 4]).any()
    keep = np.arange(c.n) != 4
    assert other_id[:, keep].tobytes() == F.samples[:, keep].tobytes()
    # a chain continued
    six = _run(c, 6).samples
    assert six[:3].tobytes() == F.samples.tobytes()
    rest = _run(c, 3, init=F.samples[2], first_iteration=3).samples
    assert rest.tobytes() == six[3:].tobytes()


# ---------------------------------------------------------------- 4. statistics
@pytest.mark.parametrize("name", ["a", "b65", "b256"])
def test_statistics_of_the_kept_sweeps(name):
    c = cases.case(name)
    T, discard, every = 40, 5, 3
    F = _run(c, T, discard=discard, keep_every=every)
    kept = F.samples[discard::every].astype(np.float64)
    n_kept = len(kept)
    assert F.count == n_kept == len(range(discard, T, every)) == 12
    ref_mean = kept.mean(0)
    ref_var = ((kept - ref_mean) ** 2).mean(0)
    dmax = np.abs(kept - kept[0]).max(0)
    np.testing.assert_allclose(F.mean, ref_mean, rtol=1e-9, atol=0)
    bound = 1e-9 * ref_var + 4 * (n_kept + 4) * U53 * dmax ** 2
    diff = np.abs(F.variance - ref_var)
    print("%s: largest variance difference / bound %.3g" % (name, (diff[bound > 0] / bound[bound > 0]).max()))
    assert (diff <= bound).all()
    assert (F.variance >= 0).all() and (F.variance > 0).any()
    one = _run(c, T, discard=T - 1)
    assert one.count == 1 and (one.variance == 0.0).all() and one.mean.tobytes() == one.samples[-1].astype(np.float64).tobytes()
    assert one.samples.tobytes() == F.samples.tobytes()


# ---------------------------------------------------------------- 5. W = 1: independent draws of one distribution
def _tn_moments(mu, tau_p):
    """mean, variance and fourth central moment of TN(mu, tau_p) on [0, inf) by quadrature in fp64"""
    sigma = 1.0 / np.sqrt(tau_p)
    x = np.linspace(0.0, max(mu, 0.0) + 12.0 * sigma, 400001)
    w = np.exp(-0.5 * tau_p * (x - mu) ** 2 + 0.5 * tau_p * min(mu, 0.0) ** 2)
    dx = x[1] - x[0]

    def integral(f):
        return (f[1:] + f[:-1]).sum() * dx / 2.0

    z = integral(w)
    mean = integral(w * x) / z
    var = integral(w * (x - mean) ** 2) / z
    return mean, var, integral(w * (x - mean) ** 4) / z


def test_one_column_draws_are_independent_draws_of_the_conditional():
    c = cases.case("b1")
    T = 4000
    F = _run(c, T, store_samples=False)
    assert F.samples is None and F.count == T
    mu, tp, _ = cases.conditionals(c, c.x0, c.x0)                 # (W = 1: the state does not enter)
    for q in range(c.n):
        mean, var, mu4 = _tn_moments(mu[q, 0], tp[q, 0])
        se_mean, se_var = np.sqrt(var / T), np.sqrt((mu4 - var ** 2) / T)
        print("unit %d: mean %.5f (%.5f, %.2f se), variance %.3e (%.3e, %.2f se)" % (
            q, F.mean[q, 0], mean, (F.mean[q, 0] - mean) / se_mean, F.variance[q, 0], var, (F.variance[q, 0] - var) / se_var))
        assert abs(F.mean[q, 0] - mean) <= 5 * se_mean
        assert abs(F.variance[q, 0] - var) <= 5 * se_var


# ---------------------------------------------------------------- 6. through the classes
PRI2 = dict(alpha=1., beta=1., lambdaU=1., lambdaV=1.)
PRI3 = dict(alpha=1., beta=1., lambdaF=1., lambdaS=1., lambdaG=1.)
KINDS = ["bnmf gibbs", "bnmf gibbs entries", "bnmtf gibbs observed", "bnmf vb", "bnmf vb observed", "bnmtf vb", "bnmtf vb observed", "nmf icm",
         "nmtf icm"]
N_I, N_J = 12, 9


def _data(tri, seed=3):
    rs = np.random.RandomState(seed)
    if tri:
        R = rs.exponential(1.0, (N_I, 3)) @ rs.exponential(1.0, (3, 2)) @ rs.exponential(1.0, (N_J, 2)).T
    else:
        R = rs.exponential(1.0, (N_I, 3)) @ rs.exponential(1.0, (N_J, 3)).T
    M = (rs.rand(N_I, N_J) >= 0.3).astype(float)
    M[rs.randint(N_I, size=N_J), np.arange(N_J)] = 1; M[np.arange(N_I), rs.randint(N_J, size=N_I)] = 1
    return R, M


def _model(kind):
    """(the fitted model, the keyword arguments of its fold_in, the factors its predict() multiplies, tau, the seed to hand on)"""
    np.random.seed(4)
    tri = "tf" in kind
    R, M = _data(tri)
    if kind == "bnmf gibbs":
        m = bnmf_gibbs_optimised(R, M, 3, PRI2, seed=1, verbose=False)
    elif kind == "bnmf gibbs entries":
        m = bnmf_gibbs_optimised(Entries.from_dense(R, M), None, 3, PRI2, seed=1, verbose=False, layout='observed')
    elif kind == "bnmtf gibbs observed":
        m = bnmtf_gibbs_optimised(R, M, 3, 2, PRI3, seed=1, verbose=False, layout='observed')
    elif kind == "bnmf vb":
        m = bnmf_vb_optimised(R, M, 3, PRI2, verbose=False)
    elif kind == "bnmf vb observed":
        m = bnmf_vb_observed(R, M, 3, PRI2, verbose=False)
    elif kind == "bnmtf vb":
        m = bnmtf_vb_optimised(R, M, 3, 2, PRI3, verbose=False)
    elif kind == "bnmtf vb observed":
        m = bnmtf_vb_observed(R, M, 3, 2, PRI3, verbose=False)
    elif kind == "nmf icm":
        m = nmf_icm(R, M, 3, PRI2, seed=1, verbose=False)
    else:
        m = nmtf_icm(R, M, 3, 2, PRI3, seed=1, verbose=False)
    m.initialise()
    if "icm" in kind:
        m.run(6, minimum_TN=0.1)                        # (without the clamp the ICM fit of this small matrix ends with a factor at zero)
    else:
        m.run(6)
    if "gibbs" in kind:
        est = m.approx_expectation(2, 2)
        return m, dict(burn_in=2, thinning=2), list(est[:-1]), est[-1], 1, {}
    if "vb" in kind:
        factors = [m.expF, m.expS, m.expG] if tri else [m.expU, m.expV]
        return m, {}, factors, m.exptau, 7, dict(seed=7)             # (a variational class is given no seed: the call names one)
    return m, {}, ([m.F, m.S, m.G] if tri else [m.U, m.V]), m.tau, 1, {}


def _fixed(factors, axis):
    """the fixed side from the factors, summed over the inner index in order"""
    factors = [np.asarray(f, dtype=np.float64) for f in factors]
    if len(factors) == 2:
        return factors[1] if axis == 0 else factors[0]
    F, S, G = factors
    X, T = (G, S.T) if axis == 0 else (F, S)
    out = np.zeros((X.shape[0], T.shape[1]))
    for i in range(X.shape[0]):
        for w in range(T.shape[1]):
            acc = 0.0
            for q in range(X.shape[1]):
                acc += X[i, q] * T[q, w]
            out[i, w] = acc
    return out


def _snapshot(m):
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in vars(m).items()
            if isinstance(v, (np.ndarray, int, float, str, tuple, list, type(None)))}


@pytest.mark.parametrize("kind", KINDS)
def test_fold_in_of_a_fitted_model_is_from_factors_on_its_attributes(kind):
    m, kw, factors, tau, seed, seed_kw = _model(kind)
    before = _snapshot(m)
    rs = np.random.RandomState(8)
    for axis in (0, 1):
        extent = N_J if axis == 0 else N_I
        idx = np.concatenate([rs.choice(extent, size=3, replace=False) for _ in range(4)])
        unit = np.repeat(np.arange(4), 3)
        values = rs.exponential(2.0, 12)
        new = Entries((4, N_J), unit, idx, values) if axis == 0 else Entries((N_I, 4), idx, unit, values)
        F = fold_in(m, new, 3, axis=axis, store_samples=True, **kw, **seed_kw)
        other = _fixed(factors, axis)
        lam = np.asarray(getattr(m, "lambda" + m._FACTORS[0 if axis == 0 else -1]))[0]
        want = fold_in.from_factors(other, new, lam, tau, 3, axis=axis, seed=seed, store_samples=True)
        assert F.other.tobytes() == np.ascontiguousarray(other).tobytes() and F.tau == float(tau)
        assert F.samples.shape == (3, 4, other.shape[1]) and F.ids.tolist() == [0, 1, 2, 3]
        for a, b in ((F.samples, want.samples), (F.mean, want.mean), (F.variance, want.variance)):
            assert a.tobytes() == b.tobytes()
        print("%s axis %d: largest |fixed side| %.3g, largest sample %.3g" % (kind, axis, np.abs(other).max(), F.samples.max()))
        assert np.abs(other).max() > 0                  # (a fit whose fixed side is zero folds everything to zero and shows nothing)
        assert (F.samples >= 0).all() and (F.samples > 0).any() and np.isfinite(F.mean).all() and F.count == 3
        mode = fold_in(m, new, 4, axis=axis, update='mode', **kw)
        wmode = fold_in.from_factors(other, new, lam, tau, 4, axis=axis, update='mode', seed=seed)
        assert mode.mean.tobytes() == wmode.mean.tobytes() and mode.count == 1 and (mode.variance == 0).all()
        # what to recommend for the new units: the best predicted entries outside the ones given
        ex = (new.rows, new.cols) if axis == 0 else (new.cols, new.rows)
        T = top_entries.from_factors((F.mean, F.other), 2, exclude=ex)
        assert T.cols.shape == (4, 2) and (T.counts == 2).all()
        given = set(zip(ex[0].tolist(), ex[1].tolist()))
        assert not given & set(zip(*[a.tolist() for a in T.entries()]))
        P = F.mean @ F.other.T
        for q in range(4):
            free = [j for j in range(extent) if (q, j) not in given]
            assert T.cols[q, 0] == free[int(np.argmax(P[q, free]))]
    assert _snapshot(m) == before                       # the model's own attributes: byte for byte what they were
