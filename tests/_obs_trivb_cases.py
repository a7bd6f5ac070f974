"""What tests/test_obs_trivb_gpu.py, its child processes and tests/test_obs_trivb_cpu.py share: the launch shapes of
bnmtf_vb_observed (csrc/kernel_obs_vb.hip obs_trivb_sweep_kernel, kernel_obs_trivb.hip,
the S chain of kernel_trivb.hip), the seeded variational state they start from, the update orders, and the runs from it.

The smallest shapes at which those kernels can go wrong: units of 1 .. 513 entries as rows and as columns beside full units of
520 (every register form's edge and the long form, in each direction), ranks at the corners of the 32 x 32 tile, K L around the
chain's 64-lane steps and the permuted system's threshold, I and J around the four units per block.  EDGES says which case covers
what; tests/test_obs_trivb_cpu.py checks it against the masks and the launch rules."""
import numpy as np

from _obs_cases import SLOT_CAPS, WAVES, _counts_mask, _random_mask

PRI = dict(alpha=1., beta=1., lambdaF=0.5, lambdaS=0.5, lambdaG=0.5)
NAMES = ("muF", "tauF", "expF", "varF", "muS", "tauS", "expS", "varS", "muG", "tauG", "expG", "varG")
EXPTAU0 = 1.3
UNIT_COUNTS = [1, 2, 63, 64, 65, 129, 255, 256, 257, 511, 512, 513]     # entries of a unit, beside two full units of 520
PERMUTE_FROM = 64                  # csrc/api_obs_trivb.inc otvb_enqueue_chain: whole passes of K L >= 64 run on the permuted system

# name -> (mask, K, L)
CASES = {
    "rows": lambda: (_counts_mask(UNIT_COUNTS, 520, 1), 3, 2),
    "cols": lambda: (_counts_mask(UNIT_COUNTS, 520, 2).T.copy(), 3, 2),
}
for _k, _l in ((1, 1), (2, 3), (31, 32), (32, 1), (1, 32), (32, 32), (7, 9), (8, 8), (5, 13), (4, 32), (5, 26)):
    CASES["KL%dx%d" % (_k, _l)] = (lambda k=_k, l=_l: (_random_mask(40, 65, 0.5, 300 + 40 * k + l), k, l))
for _n in (1, WAVES, WAVES + 1):
    CASES["I%d" % _n] = (lambda n=_n: (_random_mask(n, 7, 0.6, 10 + n), 3, 2))
    CASES["J%d" % _n] = (lambda n=_n: (_random_mask(7, n, 0.6, 20 + n), 3, 2))

LONG_UNITS = {"rows": "3/0", "cols": "0/3"}          # describe()'s long_form_units=r/c; every other case: 0/0

# which case covers which edge (tests/test_obs_trivb_cpu.py checks every line against edges_of)
EDGES = dict({"row of %d" % c: "rows" for c in UNIT_COUNTS + [520]}, **{"column of %d" % c: "cols" for c in UNIT_COUNTS + [520]})
EDGES.update({"long rows": "rows", "long columns": "cols",
              "K,L=(1,1)": "KL1x1", "K,L=(2,3)": "KL2x3", "K,L=(31,32)": "KL31x32", "K,L=(32,1)": "KL32x1", "K,L=(1,32)": "KL1x32",
              "K,L=(32,32)": "KL32x32", "K,L=(3,2)": "rows",
              "KL=63": "KL7x9", "KL=64": "KL8x8", "KL=65": "KL5x13", "KL=128": "KL4x32", "KL=130": "KL5x26", "KL=1024": "KL32x32",
              "chain without the permuted system": "KL7x9", "chain on the permuted system": "KL8x8",
              "I=1": "I1", "I=4": "I4", "I=5": "I5", "J=1": "J1", "J=4": "J4", "J=5": "J5"})


def edges_of(name):
    M, K, L = CASES[name]()
    I, J = M.shape
    rows, cols = (M != 0).sum(axis=1).astype(int), (M != 0).sum(axis=0).astype(int)
    e = {"K,L=(%d,%d)" % (K, L), "KL=%d" % (K * L), "I=%d" % I, "J=%d" % J}
    e |= {"row of %d" % c for c in set(rows.tolist())} | {"column of %d" % c for c in set(cols.tolist())}
    if (rows > SLOT_CAPS[-1]).any():
        e.add("long rows")
    if (cols > SLOT_CAPS[-1]).any():
        e.add("long columns")
    e.add("chain on the permuted system" if K * L >= PERMUTE_FROM else "chain without the permuted system")
    return e


def long_units_of(name):
    M = CASES[name]()[0]
    return "%d/%d" % (((M != 0).sum(axis=1) > SLOT_CAPS[-1]).sum(), ((M != 0).sum(axis=0) > SLOT_CAPS[-1]).sum())


def problem(M, K, L, seed=5):
    """R and the state the tests start from: expectations at least 0.1, variances seeded, mu = exp, tau = 1; R is the state's own
    product E[F] E[S] E[G]^T plus unit noise.  The product grows with K L (about 0.06 K L here), so data of a fixed scale would leave a
    state of 32 x 32 sixty times too large: the first S pass then drives muS to -10^2, and the fp32 S system (kernel_ssys.hip,
    kernel_trivb.hip: called as they are) rounds its numerators in proportion to max |muS| -- 1e-6 of 160 is 1.6e-4 absolute on
    the entries of E[S] that are O(1), which is the precision of that system at such a state and says nothing about a launch
    shape.  With data at the state's own scale muS stays O(1) to O(10) at every rank."""
    I, J = M.shape
    rs = np.random.RandomState(seed)
    F, S, G = rs.exponential(0.3, (I, K)) + 0.1, rs.exponential(0.3, (K, L)) + 0.1, rs.exponential(0.3, (J, L)) + 0.1
    R = F @ S @ G.T + rs.randn(I, J)
    vF, vS, vG = rs.exponential(0.05, (I, K)), rs.exponential(0.05, (K, L)), rs.exponential(0.05, (J, L))
    return R, dict(muF=F.copy(), tauF=np.ones((I, K)), expF=F, varF=vF, muS=S.copy(), tauS=np.ones((K, L)), expS=S, varS=vS,
                   muG=G.copy(), tauG=np.ones((J, L)), expG=G, varG=vG)


def seed_state(model, state, exptau=EXPTAU0):
    """The state onto a model of this package or onto the oracle (both keep the reference's attribute names)."""
    for n in NAMES:
        setattr(model, n, state[n].copy())
    model.exptau = exptau


def orders(K, L, n, permuted):
    """[n][K L + K + L]: the identity order in every iteration, or a seeded permutation of all three lists per iteration."""
    if not permuted:
        return np.tile(np.concatenate([np.arange(K * L), np.arange(K), np.arange(L)]), (n, 1)).astype(np.int32)
    rs = np.random.RandomState(1000 + 37 * K + L)
    return np.array([np.concatenate([rs.permutation(K * L), rs.permutation(K), rs.permutation(L)]) for _ in range(n)], dtype=np.int32)


def oracle_orders(row, K, L):
    """One row of orders() as BNMTFVBOracle.sweep takes it."""
    return [(int(a) // L, int(a) % L) for a in row[:K * L]], [int(k) for k in row[K * L:K * L + K]], [int(l) for l in row[K * L + K:]]


def model(name, seed=5):
    from bnmtf_amd import bnmtf_vb_observed
    M, K, L = CASES[name]()
    R, state = problem(M, K, L, seed)
    b = bnmtf_vb_observed(R, M, K, L, PRI, verbose=False)
    seed_state(b, state)
    return R, M, K, L, state, b


def run(name, parts, permuted):
    """run(n, orders) for every n of parts on the case, the orders of one run of sum(parts) iterations dealt out in turn; per call
    the state, the record and the ELBO of its last iteration; and describe()."""
    R, M, K, L, state, b = model(name)
    od = orders(K, L, sum(parts), permuted)
    out, at = [], 0
    for n in parts:
        b.run(n, orders=od[at:at + n])
        at += n
        out.append(dict({nm: getattr(b, nm).copy() for nm in NAMES}, exptau=np.array(b.all_exp_tau), terms=np.array(b.all_elbo_terms),
                        mse=np.array(b.all_performances["MSE"]), r2=np.array(b.all_performances["R^2"]), rp=np.array(b.all_performances["Rp"]),
                        elbo=np.array(b.elbo())))
    desc = b.describe()
    b.close()
    return out, desc
