#!/usr/bin/env python3
"""Golden vectors of the non-probabilistic models (code/models/nmf_np.py, nmtf_np.py) by IMPORTING THE REFERENCE, with
make_golden.import_reference()'s converted copy.  What is committed is DATA ONLY: inputs and the reference's outputs.

    BNMTF_REFERENCE=<checkout> python tests/golden/make_golden_np.py   # writes tests/golden/np.npz
"""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
from make_golden import REF, quiet, rand_mask  # noqa: E402


def record_run(out, tag, model, iterations):
    """run(iterations) of the reference, with the I-divergence it prints each iteration captured."""
    idiv = []
    orig = model.compute_I_div

    def spy():
        v = orig()
        idiv.append(v)
        return v
    model.compute_I_div = spy
    with quiet(), np.errstate(all="ignore"):
        model.run(iterations)
    model.compute_I_div = orig
    out[tag + "/idiv"] = np.array(idiv)
    for key, m in [("mse", "MSE"), ("r2", "R^2"), ("rp", "Rp")]:
        out[tag + "/" + key] = np.array(model.all_performances[m])


def make_np():
    from BNMTF.code.models.nmf_np import NMF
    from BNMTF.code.models.nmtf_np import NMTF
    out = {}
    R = np.loadtxt(REF + "/data_toy/bnmf/R.txt"); M = np.loadtxt(REF + "/data_toy/bnmf/M.txt")
    I, J = R.shape
    # NMF on the toy set, two initialisations
    for tag, init, seed in [("nmf_rand", "random", 1), ("nmf_exp", "exponential", 2)]:
        np.random.seed(seed)
        n = NMF(R, M, 10)
        n.initialise(init, expo_prior=1.)
        out[tag + "/seed"] = np.array(seed)
        out[tag + "/U0"], out[tag + "/V0"] = n.U.copy(), n.V.copy()
        out[tag + "/idiv0"] = np.array(n.compute_I_div())
        record_run(out, tag, n, 100)
        out[tag + "/U"], out[tag + "/V"] = n.U.copy(), n.V.copy()
        Mp = rand_mask(np.random.RandomState(3), I, J, 0.5)
        pr = n.predict(Mp)
        out[tag + "/Mpred"], out[tag + "/pred"] = Mp, np.array([pr["MSE"], pr["R^2"], pr["Rp"]])
    # single column updates from the recorded initial state of nmf_rand
    n = NMF(R, M, 10)
    n.U, n.V = out["nmf_rand/U0"].copy(), out["nmf_rand/V0"].copy()
    n.update_U(3); out["nmf_upd/U_after_U3"] = n.U.copy()
    n.U, n.V = out["nmf_rand/U0"].copy(), out["nmf_rand/V0"].copy()
    n.update_V(5); out["nmf_upd/V_after_V5"] = n.V.copy()

    # NMF on the GDSC excerpt, K = 10
    g = np.load(os.path.join(HERE, "gdsc.npz"))
    X, Mg = g["ex/X_min"], g["ex/M"]           # (the non-negative form the experiments factorise)
    np.random.seed(4)
    n = NMF(X, Mg, 10)
    n.initialise("random")
    out["nmf_gdsc/U0"], out["nmf_gdsc/V0"] = n.U.copy(), n.V.copy()
    record_run(out, "nmf_gdsc", n, 50)
    out["nmf_gdsc/U"], out["nmf_gdsc/V"] = n.U.copy(), n.V.copy()

    # a ragged mask: rows and columns of 1-3 observed entries
    rs = np.random.RandomState(11)
    Ir, Jr = 24, 18
    Mr = np.zeros((Ir, Jr))
    for i in range(Ir):
        Mr[i, rs.choice(Jr, 1 + i % 3, replace=False)] = 1
    for j in range(Jr):
        if Mr[:, j].sum() == 0:
            Mr[rs.randint(Ir), j] = 1
    Rr = rs.rand(Ir, Jr) * 4 + 0.5
    np.random.seed(5)
    n = NMF(Rr, Mr, 3)
    n.initialise("random")
    out["nmf_ragged/R"], out["nmf_ragged/M"] = Rr, Mr
    out["nmf_ragged/U0"], out["nmf_ragged/V0"] = n.U.copy(), n.V.copy()
    record_run(out, "nmf_ragged", n, 30)
    out["nmf_ragged/U"], out["nmf_ragged/V"] = n.U.copy(), n.V.copy()

    # NMTF on the toy set
    R = np.loadtxt(REF + "/data_toy/bnmtf/R.txt"); M = np.loadtxt(REF + "/data_toy/bnmtf/M.txt")
    for tag, init_S, init_FG, seed in [("nmtf_expkm", "exponential", "kmeans", 6), ("nmtf_rand", "random", "random", 7)]:
        np.random.seed(seed); random.seed(seed)
        t = NMTF(R, M, 5, 5)
        with quiet():
            t.initialise(init_S, init_FG, expo_prior=1.)
        out[tag + "/seed"] = np.array(seed)
        out[tag + "/S0"], out[tag + "/F0"], out[tag + "/G0"] = t.S.copy(), t.F.copy(), t.G.copy()
        out[tag + "/idiv0"] = np.array(t.compute_I_div())
        record_run(out, tag, t, 50)
        out[tag + "/S"], out[tag + "/F"], out[tag + "/G"] = t.S.copy(), t.F.copy(), t.G.copy()
    # single updates from the recorded initial state of nmtf_rand
    t = NMTF(R, M, 5, 5)
    for name, call in [("S21", lambda: t.update_S(2, 1)), ("F3", lambda: t.update_F(3)), ("G4", lambda: t.update_G(4))]:
        t.S, t.F, t.G = out["nmtf_rand/S0"].copy(), out["nmtf_rand/F0"].copy(), out["nmtf_rand/G0"].copy()
        call()
        out["nmtf_upd/%s/S" % name], out["nmtf_upd/%s/F" % name], out["nmtf_upd/%s/G" % name] = t.S.copy(), t.F.copy(), t.G.copy()

    # MatrixCrossValidation(method=NMF) on the GDSC excerpt: 'ones' draws nothing, the folds come from the seeded streams
    from BNMTF.code.cross_validation.matrix_cross_validation import MatrixCrossValidation
    random.seed(8); np.random.seed(8)
    fout = os.path.join(tempfile.gettempdir(), "np_cv_golden.txt")
    cv = MatrixCrossValidation(method=NMF, X=X, M=Mg, K=5, parameter_search=[{"K": 2}, {"K": 4}],
                               train_config={"iterations": 50, "init_UV": "ones"}, file_performance=fout)
    with quiet(), np.errstate(all="ignore"):
        cv.run()
    for K in (2, 4):
        perf = cv.all_performances[cv.JSON({"K": K})]
        out["cv/K%d" % K] = np.array([perf["MSE"], perf["R^2"], perf["Rp"]])
    out["cv/seed"] = np.array(8)
    np.savez_compressed(os.path.join(HERE, "np.npz"), **out)


if __name__ == "__main__":
    make_golden.import_reference()
    make_np()
    print("np.npz", os.path.getsize(os.path.join(HERE, "np.npz")))
