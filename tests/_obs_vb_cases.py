"""What tests/test_obs_vb_gpu.py and its child processes share: the seeded variational state on the launch shapes of
tests/_obs_cases.py (the observed-entry sweep's edge cases: units of 1 .. 129 and 255 .. 257, 511 .. 513 entries as rows and as
columns, I and J around the units per block, a full matrix, ranks around the 64-lane steps), and the runs of bnmf_vb_observed
(csrc/kernel_obs_vb.hip) from it."""
import numpy as np

from bnmtf_amd import bnmf_vb_observed

from _obs_cases import PRI, SHAPES, _problem

NAMES = ("muU", "tauU", "expU", "varU", "muV", "tauV", "expV", "varV")
EXPTAU0 = 1.3


def vb_problem(M, K, seed=5):
    """R and the state the tests start from: exp = _problem's factors, var seeded, mu = exp, tau = 1."""
    I, J = M.shape
    R, U0, V0 = _problem(M, K, seed)
    rs = np.random.RandomState(9)
    varU = rs.exponential(0.05, (I, K)); varV = rs.exponential(0.05, (J, K))
    return R, dict(muU=U0.copy(), tauU=np.ones((I, K)), expU=U0.copy(), varU=varU,
                   muV=V0.copy(), tauV=np.ones((J, K)), expV=V0.copy(), varV=varV)


def seed_state(model, state, exptau=EXPTAU0):
    """The state onto a model of this package or onto the oracle (both keep the reference's attribute names)."""
    for n in NAMES:
        setattr(model, n, state[n].copy())
    model.exptau = exptau


def vb_model(M, K, seed=5):
    R, state = vb_problem(M, K, seed)
    b = bnmf_vb_observed(R, M, K, PRI, verbose=False)
    seed_state(b, state)
    return R, state, b


def vb_run(shape, parts):
    """run(n) for every n of parts on the launch shape; per call the state, the record and the ELBOs; and describe()."""
    M, K = SHAPES[shape]()
    _, _, b = vb_model(M, K)
    out = []
    for n in parts:
        b.run(n)
        out.append(dict({nm: getattr(b, nm).copy() for nm in NAMES}, exptau=np.array(b.all_exp_tau), terms=np.array(b.all_elbo_terms),
                        mse=np.array(b.all_performances["MSE"]), r2=np.array(b.all_performances["R^2"]), rp=np.array(b.all_performances["Rp"]),
                        elbo=np.array(b.all_elbo)))
    desc = b.describe()
    b.close()
    return out, desc
