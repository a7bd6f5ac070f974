"""The fp64 restatement of the non-probabilistic models (tests/_np_restatement.py) against the reference's own numbers
(tests/golden/np.npz): whole trajectories, the single updates and predict().  No GPU: a slip in the restatement cannot hide a
matching slip in the kernels it checks."""
import os

import numpy as np
import pytest

import _np_restatement as NR

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "np.npz"))
TOY = np.load(os.path.join(HERE, "golden", "toy_data.npz"))
GDSC = np.load(os.path.join(HERE, "golden", "gdsc.npz"))

TOL = 1e-9


def check_metrics(m, tag, it):
    for key, name in [("mse", "MSE"), ("r2", "R^2"), ("rp", "Rp"), ("idiv", "I_div")]:
        np.testing.assert_allclose(m[name], G[tag + "/" + key][it], rtol=TOL, atol=0, equal_nan=True, err_msg="%s %s it %d" % (tag, key, it))


@pytest.mark.parametrize("tag,R,M,iters", [
    ("nmf_rand", TOY["bnmf/R"], TOY["bnmf/M"], 100),
    ("nmf_ragged", G["nmf_ragged/R"], G["nmf_ragged/M"], 30),
    ("nmf_gdsc", GDSC["ex/X_min"], GDSC["ex/M"], 50),
])
def test_nmf_trajectory(tag, R, M, iters):
    Mb = M.astype(bool)
    U, V = G[tag + "/U0"], G[tag + "/V0"]
    if tag + "/idiv0" in G:
        np.testing.assert_allclose(NR.metrics(R, Mb, U @ V.T)["I_div"], G[tag + "/idiv0"], rtol=TOL)
    for it in range(iters):
        U, V = NR.ref_nmf_iteration(R, Mb, U, V)
        check_metrics(NR.metrics(R, Mb, U @ V.T), tag, it)
    np.testing.assert_allclose(U, G[tag + "/U"], rtol=TOL)
    np.testing.assert_allclose(V, G[tag + "/V"], rtol=TOL)


def test_nmtf_trajectory():
    tag = "nmtf_rand"
    R, Mb = TOY["bnmtf/R"], TOY["bnmtf/M"].astype(bool)
    F, S, Gf = G[tag + "/F0"], G[tag + "/S0"], G[tag + "/G0"]
    np.testing.assert_allclose(NR.metrics(R, Mb, F @ S @ Gf.T)["I_div"], G[tag + "/idiv0"], rtol=TOL)
    for it in range(50):
        F, S, Gf = NR.ref_nmtf_iteration(R, Mb, F, S, Gf)
        check_metrics(NR.metrics(R, Mb, F @ S @ Gf.T), tag, it)
    for name, X in zip("FSG", (F, S, Gf)):
        np.testing.assert_allclose(X, G[tag + "/" + name], rtol=TOL, err_msg=name)


def test_nmf_single_updates():
    R, Mb = TOY["bnmf/R"], TOY["bnmf/M"].astype(bool)
    U0, V0 = G["nmf_rand/U0"], G["nmf_rand/V0"]
    np.testing.assert_allclose(NR.update_U(R, Mb, U0, V0, 3), G["nmf_upd/U_after_U3"], rtol=TOL)
    np.testing.assert_allclose(NR.update_V(R, Mb, U0, V0, 5), G["nmf_upd/V_after_V5"], rtol=TOL)


@pytest.mark.parametrize("name", ["S21", "F3", "G4"])
def test_nmtf_single_updates(name):
    R, Mb = TOY["bnmtf/R"], TOY["bnmtf/M"].astype(bool)
    F, S, Gf = G["nmtf_rand/F0"], G["nmtf_rand/S0"], G["nmtf_rand/G0"]
    if name == "S21":
        S = NR.update_S(R, Mb, F, S, Gf, 2, 1)
    elif name == "F3":
        F = NR.update_F(R, Mb, F, S, Gf, 3)
    else:
        Gf = NR.update_G(R, Mb, F, S, Gf, 4)
    for n, X in zip("FSG", (F, S, Gf)):
        np.testing.assert_allclose(X, G["nmtf_upd/%s/%s" % (name, n)], rtol=TOL, err_msg=n)


@pytest.mark.parametrize("tag", ["nmf_rand", "nmf_exp"])
def test_predict(tag):
    m = NR.metrics(TOY["bnmf/R"], G[tag + "/Mpred"], G[tag + "/U"] @ G[tag + "/V"].T)
    np.testing.assert_allclose([m["MSE"], m["R^2"], m["Rp"]], G[tag + "/pred"], rtol=TOL)


# ---------------------------------------------------------------- the launch-edge cases of tests/test_np_shapes_gpu.py
SHAPES = {   # (I, J, K): (E, T, RB, n % RB, idle lanes) of the rows' and of the columns' half sweep (kernel_np.hip, np_sweep_shape)
    (37, 2048, 16): ((2, 1024, 16, 5, 0), (2, 64, 16, 0, 91)),
    (45, 2049, 33): ((4, 576, 8, 5, 255), (2, 64, 16, 1, 83)),
    (29, 4097, 64): ((8, 576, 4, 1, 511), (2, 64, 16, 1, 99)),
    (3, 8193, 65): ((16, 576, 1, 0, 1023), (2, 64, 16, 1, 125)),
    (21, 16384, 256): ((16, 1024, 1, 0, 0), (2, 64, 16, 0, 107)),
    (16383, 19, 1): ((2, 64, 16, 15, 109), (16, 1024, 1, 0, 1)),
    (2050, 4099, 24): ((8, 576, 4, 2, 509), (4, 576, 8, 3, 254)),
}


def _launch(n, m):
    E, T, RB = NR.sweep_shape(m)
    return E, T, RB, n % RB, T * E - m


def test_edge_cases_reach_every_sweep_instance_at_its_guards():
    from test_np_shapes_gpu import CASES
    assert sorted(CASES) == sorted(SHAPES)
    for (I, J, K), (rows, cols) in SHAPES.items():
        assert (_launch(I, J), _launch(J, I)) == (rows, cols), (I, J, K)
    launches = [s for pair in SHAPES.values() for s in pair]
    for E in (2, 4, 8, 16):                                        # every instance runs; those with RB > 1 with a partial last block
        mine = [s for s in launches if s[0] == E]
        assert mine and any(s[4] > 0 for s in mine), E
        assert E == 16 or any(s[3] > 0 for s in mine), E


@pytest.mark.parametrize("I,J,K", sorted(SHAPES))
def test_edge_cases_would_see_a_dropped_edge_entry(I, J, K):
    """Dropping (I - 1, J - 1), or the first observed entry of the first row of the last block of rows (or of columns), from the
    mask must move the restatement's iteration by far more than the device tests' one-iteration tolerance: those tests would
    see a kernel that skips such an entry."""
    from test_np_shapes_gpu import TOL_ONE, nmf_case
    R, M, U0, V0 = nmf_case(I, J, K)
    U, V = NR.ref_nmf_iteration(R, M, U0, V0)
    r0 = NR.edge_entries(I, J)[0][0]
    c0 = NR.edge_entries(J, I)[0][0]
    for drop in [(I - 1, J - 1), (r0, np.flatnonzero(M[r0])[0]), (np.flatnonzero(M[:, c0])[0], c0)]:
        M2 = M.copy(); M2[drop] = False
        U2, V2 = NR.ref_nmf_iteration(R, M2, U0, V0)
        moved = max(NR.rel_err(U2, U), NR.rel_err(V2, V))
        assert moved > 10 * TOL_ONE, (drop, moved)
