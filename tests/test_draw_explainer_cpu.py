"""tests/_draw_explainer.py without a GPU: the oracle's chains explain themselves; an honest fp32 restatement of the device's
sampler (sweep_common.h: tn_fast_pre / tn_fast_post, tn_cand_pre / tn_cand_post, in np.float32) is explained completely; every
mutation of it that moves a draw to another candidate, counter word or regime leaves unexplained draws; and the steered inputs
of every case of tests/test_draws_explained_gpu.py meet that case's ambiguity cap and its form's coverage counts on the oracle's
own chain."""
import time

import numpy as np
import pytest

from oracle import bnmtf_oracle as O
from oracle import rng

import _draw_cases as C
import _draw_explainer as X

f32 = np.float32


# ---------------------------------------------------------------- 1. the oracle's chains explain themselves
def _bnmf_problem(I, J, K, seed):
    rs = np.random.RandomState(seed)
    R = rs.exponential(1.0, (I, 3)) @ rs.exponential(1.0, (J, 3)).T + rs.randn(I, J)
    M = (rs.rand(I, J) > 0.2).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    return R, M, rs.exponential(0.6, (I, K)), rs.exponential(0.6, (J, K))


@pytest.mark.parametrize("I,J,K", [(60, 45, 6), (30, 25, 70)])
def test_bnmf_oracle_chain_explains_itself(I, J, K):
    """dmu = 0, the floor terms only: 0 unexplained, 0 ambiguous, on every iteration; K = 70: column words 64 ... 69 too"""
    R, M, U0, V0 = _bnmf_problem(I, J, K, 3 + K)
    pri = dict(alpha=2.0, beta=1.5, lambdaU=0.7, lambdaV=0.4)
    o = O.BNMFGibbsOracle(R, M, K, pri, seed=91)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 0.9
    o.run(3)
    e = X.explain_bnmf_run(R, M, 0.7, 0.4, 2.0, 1.5, 91, (U0, V0, 0.9), o.all_U, o.all_V, o.all_tau, c_mu=0.0)
    print("draws %d unexplained %d ambiguous %d max err %.2e tau %.1e" % (e.draws, e.unexplained, e.ambiguous, e["err"].max(), max(e.tau_rel)))
    assert e.draws == 3 * (I + J) * K
    assert e.unexplained == 0 and e.ambiguous == 0
    assert e["err"].max() < 1e-6                     # (the same fp64 formulas: the value error is rounding)
    assert set(e["it"]) == {0, 1, 2} and e["col"].max() == K - 1
    assert max(e.tau_rel) < 1e-12


def test_bnmtf_oracle_chain_explains_itself():
    rs = np.random.RandomState(8)
    I, J, K, L = 40, 30, 4, 3
    R = rs.exponential(1.0, (I, K)) @ rs.exponential(1.0, (K, L)) @ rs.exponential(1.0, (J, L)).T + rs.randn(I, J)
    M = (rs.rand(I, J) > 0.2).astype(float)
    M[np.arange(I), rs.randint(0, J, I)] = 1; M[rs.randint(0, I, J), np.arange(J)] = 1
    pri = dict(alpha=1.0, beta=1.0, lambdaF=0.6, lambdaS=0.3, lambdaG=0.5)
    F0, S0, G0 = rs.exponential(0.7, (I, K)), rs.exponential(0.7, (K, L)), rs.exponential(0.7, (J, L))
    o = O.BNMTFGibbsOracle(R, M, K, L, pri, seed=17)
    o.F, o.S, o.G, o.tau = F0.copy(), S0.copy(), G0.copy(), 1.1
    o.run(3)
    e = X.explain_bnmtf_run(R, M, 0.6, 0.3, 0.5, 1.0, 1.0, 17, (F0, S0, G0, 1.1), o.all_F, o.all_S, o.all_G, o.all_tau, c_mu=0.0)
    print("draws %d unexplained %d ambiguous %d max err %.2e tau %.1e" % (e.draws, e.unexplained, e.ambiguous, e["err"].max(), max(e.tau_rel)))
    assert e.draws == 3 * (I * K + K * L + J * L)
    assert e.unexplained == 0 and e.ambiguous == 0 and e["err"].max() < 1e-6
    assert int((e["factor"] == "S").sum()) == 3 * K * L and e["col"][e["factor"] == "S"].max() == K * L - 1
    assert max(e.tau_rel) < 1e-12


def test_residual_form_of_the_tri_chain_is_the_as_written_oracles():
    """the chain the coverage counts below run (_draw_cases.oracle_bnmtf_chain) against oracle.BNMTFGibbsOracle"""
    case = [c for c in C.BNMTF_CASES if c["id"] == "rowwise-90x70k5l4"][0]
    R, M, init, lams = C.case_inputs(case)
    o = O.BNMTFGibbsOracle(R, M, 5, 4, dict(alpha=1.0, beta=1.0, lambdaF=lams[0], lambdaS=lams[1], lambdaG=lams[2]), seed=C.SEED)
    o.F, o.S, o.G, o.tau = init[0].copy(), init[1].copy(), init[2].copy(), init[3]
    o.run(C.ITERATIONS)
    aF, aS, aG, at = C.oracle_bnmtf_chain(R, M, lams, init, C.SEED, C.ITERATIONS)
    for got, want in ((aF, o.all_F), (aS, o.all_S), (aG, o.all_G), (at, o.all_tau)):
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-10)


# ---------------------------------------------------------------- 2. an fp32 "device" in NumPy and its mutations
def _rcp(v):
    return f32(1.0) / v


def fp32_device_run(R, M, lamU, lamV, init, seed, iterations, mut=None, alpha=1.0, beta=1.0, noise_seed=4):
    """The two-factor sampler with the device's arithmetic restated in np.float32: the conditional's numerator and precision
    from the chain's own state in fp64, then rounded to fp32 with fp32-sized noise (4e-6 of the cancelling terms: a fifth of the
    bound the conditional-parameter tests hold the device to), the parameters by tn_fast_pre / tn_fast_post, the candidates by
    tn_cand_pre / tn_cand_post -- the reciprocal-based forms and the |e - d| <= sqrt(-2 ln u2) acceptance test of
    sweep_common.h.  mut names one deliberate defect (see MUTATIONS)."""
    mut = mut or {}
    I, J = R.shape
    U = np.array(init[0], dtype=np.float64); V = np.array(init[1], dtype=np.float64); tau = float(init[2])
    K = U.shape[1]
    nrs = np.random.RandomState(noise_seed)
    MR = M * np.abs(R)
    alpha_s = alpha + M.sum() / 2.0
    all_U, all_V, all_tau = [], [], []
    streams = (rng.STREAM_ROWS, rng.STREAM_COLS)
    if mut.get("swap_streams"):
        streams = streams[::-1]
    for t in range(iterations):
        itw = 0 if (mut.get("it_stuck") and t == 1) else t
        E = M * (R - U @ V.T)
        for X_, Y_, lam, Mm, MRm, stream, tr in ((U, V, lamU, M, MR, streams[0], False), (V, U, lamV, M.T, MR.T, streams[1], True)):
            n = X_.shape[0]
            elem = np.arange(n)
            if "local_from" in mut:                       # a shard whose first unit is local_from numbers its units from 0
                elem = np.where(elem >= mut["local_from"], elem - mut["local_from"], elem)
            for k in range(K):
                y = Y_[:, k]
                g = Mm @ (y * y)
                scale = tau * (MRm @ np.abs(y) + np.abs(X_) @ np.abs(Y_.T @ y))
                numer = f32(-lam[:, k] + tau * ((E.T if tr else E) @ y + X_[:, k] * g) + 4e-6 * scale * nrs.uniform(-1, 1, n))
                tau_p = f32(tau * g * (1.0 + 2e-7 * nrs.uniform(-1, 1, n)))
                colw = k + mut.get("col_off", 0)
                if "block_at" in mut and k >= mut["block_at"]:        # a column block that forgets its col0
                    colw = k - mut["block_at"]
                x = _tn_fast_draw(numer, tau_p, elem, colw, itw, stream, seed, mut)
                d = np.outer(x - X_[:, k], y)
                E -= M * (d.T if tr else d)
                X_[:, k] = x
        tau = X.gamma_unit(alpha_s, t, seed) / (beta + 0.5 * (E * E).sum())
        all_U.append(U.astype(f32)); all_V.append(V.astype(f32)); all_tau.append(tau)
    return np.array(all_U), np.array(all_V), np.array(all_tau)


def _tn_fast_draw(numer, tau_p, elem, col, it, stream, seed, mut):
    a0 = f32(mut.get("a0", rng.TN_A0))
    with np.errstate(all="ignore"):
        live = tau_p > 0
        tp = np.where(live, tau_p, f32(1.0)).astype(f32)
        irt = _rcp(np.sqrt(tp)).astype(f32); rcp = _rcp(tp).astype(f32); tpirt = (tp * irt).astype(f32)
        mu = (numer * rcp).astype(f32)
        a = (-mu * tpirt).astype(f32)
        if not mut.get("no_guard"):
            live = live & np.isfinite(a)
        d = (f32(2.0) * _rcp((np.sqrt((a * a + f32(4.0)).astype(f32)) + a).astype(f32))).astype(f32)
        tail = a >= a0
    n = numer.size
    out = np.zeros(n, dtype=f32)
    need = np.full(n, 2 if mut.get("second_accept") else 1)
    todo = np.nonzero(live if not mut.get("no_guard") else np.ones(n, dtype=bool))[0]
    c = 0
    while todo.size and c < 4096:
        cw = c + 1 if ("shift_from" in mut and c >= mut["shift_from"]) else c
        r0, r1, _, _ = rng.philox4x32_10(elem[todo], col, it, int(stream) + 16 * cw, seed)
        u1 = rng.u23(r0).astype(f32); u2 = rng.u23(r1).astype(f32)
        with np.errstate(all="ignore"):
            nl = (f32(-0.69314718) * np.log2(u1).astype(f32)).astype(f32)
            z = (np.sqrt((f32(2.0) * nl).astype(f32)) * np.cos(rng.TWO_PI * u2.astype(np.float64)).astype(f32)).astype(f32)
            sw = np.sqrt((f32(-1.38629436) * np.log2(u2).astype(f32)).astype(f32)).astype(f32)
            e = (nl * d[todo]).astype(f32)
            tt = (e - d[todo]).astype(f32)
            acc = np.where(tail[todo], np.abs(tt) <= sw, z >= a[todo])
            xv = np.where(tail[todo], (e * irt[todo]).astype(f32), (z * irt[todo] + mu[todo]).astype(f32)).astype(f32)
        if not mut.get("no_guard"):
            xv = np.where(np.isfinite(xv) & (xv >= 0), xv, f32(0.0)).astype(f32)
        need[todo[acc]] -= 1
        got = acc & (need[todo] == 0)
        out[todo[got]] = xv[got]
        todo = todo[~got]
        c += 1
    return out.astype(np.float64)


# candidate index +1 from the 2nd / 5th / 9th candidate on; the second accepted candidate; a column word off by one; col0 ignored
# in a column block (columns 8 ... numbered from 0); rows' and columns' streams swapped; local instead of global element index
# behind a non-zero first unit; the regime switch at 0.5; no guard (the raw e * irt of a dead conditional -- tau_p = 0, the zeroed
# column of V -- and of a negative value goes out instead of the guarded 0); the iteration word stuck at 0 in iteration 1
MUTATIONS = {
    "cand+1 from 2nd": dict(shift_from=1), "cand+1 from 5th": dict(shift_from=4), "cand+1 from 9th": dict(shift_from=8),
    "second accepted": dict(second_accept=True), "column word +1": dict(col_off=1), "col0 ignored": dict(block_at=8),
    "streams swapped": dict(swap_streams=True), "local element index": dict(local_from=64), "tail threshold 0.5": dict(a0=0.5),
    "no guard": dict(no_guard=True), "iteration word stuck": dict(it_stuck=True),
}
FP32_CASE = (192, 130, 12, 0.0, 0.5, 5)           # the unit / pair-layout case of the GPU test, column 5 of V0 zero


@pytest.fixture(scope="module")
def fp32_inputs():
    return C.bnmf_inputs(*FP32_CASE)


def _explain_fp32(inp, mut, iterations):
    R, M, init, (lamU, lamV) = inp
    aU, aV, at = fp32_device_run(R, M, lamU, lamV, init, C.SEED, iterations, mut)
    return X.explain_bnmf_run(R, M, lamU, lamV, 1.0, 1.0, C.SEED, init, aU, aV, at)


def test_honest_fp32_restatement_is_explained(fp32_inputs):
    e = _explain_fp32(fp32_inputs, None, 3)
    share = e.ambiguous / float(e.draws)
    print("fp32 restatement: draws %d unexplained %d ambiguous %d (%.3f %%) unique %d; err max %.3f; past 4: %d, past 8: %d; tau %.1e"
          % (e.draws, e.unexplained, e.ambiguous, 100 * share, int(e.unique().sum()), e["err"][e["explained"]].max(), e.past(4), e.past(8), max(e.tau_rel)))
    assert e.unexplained == 0, e.offenders()
    assert share < 0.005
    assert max(e.tau_rel) < X.TAU_REL
    assert int((e["cand"] == -1).sum()) >= 3 * 192          # the dead column's guarded zeros were explained as such


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutation_leaves_unexplained_draws(fp32_inputs, name):
    e = _explain_fp32(fp32_inputs, MUTATIONS[name], 2)
    print("%s: %d of %d draws unexplained" % (name, e.unexplained, e.draws))
    assert e.unexplained > 0


# ---------------------------------------------------------------- 3. the GPU cases' inputs on the oracle's own chain
_ORACLE = {}


def oracle_explained(case):
    """the oracle's chain on a case's steered inputs through the driver (shared by the cases that share inputs; never changed)"""
    key = (case["shape"], tuple(sorted(case["kw"].items())))
    if key not in _ORACLE:
        R, M, init, lams = C.case_inputs(case)
        t0 = time.time()
        if len(init) == 3:
            o = O.BNMFGibbsFairCPU(R, M, init[0].shape[1], dict(alpha=1.0, beta=1.0, lambdaU=lams[0], lambdaV=lams[1]), seed=C.SEED)
            o.U, o.V, o.tau = init[0].copy(), init[1].copy(), init[2]
            o.run(C.ITERATIONS)
            t1 = time.time()
            e = X.explain_bnmf_run(R, M, lams[0], lams[1], 1.0, 1.0, C.SEED, init, o.all_U, o.all_V, o.all_tau)
        else:
            aF, aS, aG, at = C.oracle_bnmtf_chain(R, M, lams, init, C.SEED, C.ITERATIONS)
            t1 = time.time()
            e = X.explain_bnmtf_run(R, M, lams[0], lams[1], lams[2], 1.0, 1.0, C.SEED, init, aF, aS, aG, at)
        _ORACLE[key] = (e, time.time() - t1)
    return _ORACLE[key]


@pytest.mark.parametrize("case", C.BNMF_CASES + C.BNMTF_CASES, ids=lambda c: c["id"])
def test_case_inputs_meet_the_ambiguity_cap_on_the_oracles_chain(case):
    e, secs = oracle_explained(case)
    share = e.ambiguous / float(e.draws)
    print("%s: draws %d ambiguous %.3f %% unexplained %d; explainer %.2f s" % (case["id"], e.draws, 100 * share, e.unexplained, secs))
    assert e.unexplained == 0, e.offenders()
    assert share <= C.AMBIGUITY_CAP
    assert max(e.tau_rel) < 1e-9


@pytest.mark.parametrize("tri,form", [(False, f) for f in C.forms(C.BNMF_CASES)] + [(True, f) for f in C.forms(C.BNMTF_CASES)])
def test_form_coverage_on_the_oracles_chain(tri, form):
    from bnmtf_amd._blocked import block_ranges
    cases = C.forms(C.BNMTF_CASES if tri else C.BNMF_CASES)[form]
    results = [oracle_explained(c)[0] for c in cases]
    batch = (1 if form.startswith("small") else 4) if tri else C.BATCH[form]
    blocks = [block_ranges(c["shape"][2]) for c in cases] if form == "blocks" else None
    for c, r in zip(cases, results):
        print("%s: past %d: %d, past 8: %d, regimes %s%s" % (c["id"], min(batch, 4), r.past(min(batch, 4), ("F", "G") if tri else None),
              r.past(8, ("F", "G") if tri else None), ["%.2f" % s for s in r.regime_shares()], ", S past 4: %d" % r.past(4, ("S",)) if tri else ""))
    fails = C.coverage_failures(form, batch, results, tri=tri, blocks=blocks)
    assert not fails, fails


def test_explainer_takes_seconds_at_the_largest_case():
    case = [c for c in C.BNMF_CASES if c["shape"][:3] == (640, 800, 64)][0]
    e, secs = oracle_explained(case)
    print("640 x 800, K = 64, %d iterations: %d draws explained in %.1f s" % (C.ITERATIONS, e.draws, secs))
    assert secs < 60.0
