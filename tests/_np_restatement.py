"""The non-probabilistic models' multiplicative updates restated in NumPy fp64 -- the checker the device's large-shape tests trust
(tests/test_np_gpu.py, tests/test_np_shapes_gpu.py).  tests/test_np_restatement_cpu.py pins it to the reference's own numbers
(tests/golden/np.npz).

Each update is the reference's (nmf_np.py:117-121, nmtf_np.py:158-177) with P = U V^T (or F S G^T) kept current by rank-one
changes instead of being rebuilt, so every column sees the new values of the columns before it.  Masks are boolean arrays;
factors are copied, never changed in place."""
import numpy as np


def _ratio(R, M, P):
    """R / P on the mask, 0 elsewhere."""
    return np.divide(np.where(M, R, 0.0), P, out=np.zeros(P.shape), where=M)


def ref_half(R, M, U, V, cols=None):
    """U's columns `cols` (default: all) in order given V, P moved by each column's change (nmf_np.py:117-118 per column)."""
    M = np.asarray(M, dtype=bool)
    U = np.array(U, dtype=float)
    P = np.where(M, U @ V.T, 1.0)                      # (off the mask P is never used: R / P is taken as 0 there)
    Rm, Mf, Q = np.where(M, R, 0.0), M.astype(float), np.empty(P.shape)
    den = Mf @ V
    for k in (range(U.shape[1]) if cols is None else cols):
        np.divide(Rm, P, out=Q)
        new = U[:, k] * (Q @ V[:, k]) / den[:, k]
        P += np.outer(new - U[:, k], V[:, k]) * Mf
        U[:, k] = new
    return U


def ref_nmf_iteration(R, M, U, V):
    """nmf_np.py:96-99: all columns of U, then all columns of V."""
    M = np.asarray(M, dtype=bool)
    U = ref_half(R, M, U, V)
    V = ref_half(R.T, M.T, V, U)
    return U, V


def update_U(R, M, U, V, k):
    """nmf_np.py:117-118."""
    return ref_half(R, M, U, V, [k])


def update_V(R, M, U, V, k):
    """nmf_np.py:120-121."""
    return ref_half(np.asarray(R).T, np.asarray(M, dtype=bool).T, V, U, [k])


def _s_entry(R, M, F, S, G, P, k, l):
    """S[k, l] given P = F S G^T (nmtf_np.py:172-177); S and P are updated in place."""
    num = F[:, k] @ _ratio(R, M, P) @ G[:, l]
    den = F[:, k] @ M.astype(float) @ G[:, l]
    new = S[k, l] * num / den
    P += (new - S[k, l]) * np.outer(F[:, k], G[:, l])
    S[k, l] = new


def update_S(R, M, F, S, G, k, l):
    """nmtf_np.py:172-177: the new S."""
    M = np.asarray(M, dtype=bool)
    S = np.array(S, dtype=float)
    _s_entry(R, M, F, S, G, F @ S @ G.T, k, l)
    return S


def update_F(R, M, F, S, G, k):
    """nmtf_np.py:158-163: the new F."""
    return ref_half(R, M, F, G @ S.T, [k])


def update_G(R, M, F, S, G, l):
    """nmtf_np.py:165-170: the new G."""
    return ref_half(np.asarray(R).T, np.asarray(M, dtype=bool).T, G, F @ S, [l])


def ref_nmtf_iteration(R, M, F, S, G):
    """nmtf_np.py:127-135: the entries of S row by row over (k, l), then the columns of F, then those of G."""
    M = np.asarray(M, dtype=bool)
    S = np.array(S, dtype=float)
    P = F @ S @ G.T
    for k in range(S.shape[0]):
        for l in range(S.shape[1]):
            _s_entry(R, M, F, S, G, P, k, l)
    F = ref_half(R, M, F, G @ S.T)
    G = ref_half(R.T, M.T, G, F @ S)
    return F, S, G


def metrics(R, M, P):
    """n, MSE, R^2, Rp and the I-divergence sum R log(R / P) - R + P over the mask (nmf_np.py:124-148)."""
    M = np.asarray(M, dtype=bool)
    r, p = np.asarray(R, dtype=float)[M], np.asarray(P, dtype=float)[M]
    n = r.size
    sse = ((r - p) ** 2).sum()
    dr, dp = r - r.mean(), p - p.mean()
    ss_tot = (dr * dr).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        idiv = (r * np.log(r / p) - r + p).sum()
    return {"n": n, "MSE": sse / n, "R^2": 1.0 - sse / ss_tot if ss_tot != 0.0 else np.inf,
            "Rp": (dr * dp).sum() / (np.sqrt(ss_tot) * np.sqrt((dp * dp).sum())), "I_div": idiv}


# ---------------------------------------------------------------- launch shapes of the device's half sweep and problems at their edges
def sweep_shape(m):
    """(E, T, RB) of np_sweep_kernel for inner extent m (kernel_np.hip, np_sweep_shape): E entries per thread and row, T threads,
    RB rows per block."""
    e = 2
    while e < 16 and -(-m // e) > 1024:
        e *= 2
    return e, -(-(-(-m // e)) // 64) * 64, 1 if e == 16 else 32 // e


def edge_entries(n, m):
    """The rows of an n x m half sweep whose index guards a slip would hit -- the last row and the first row of the last block
    -- and, in the inner index, the last entry and the last entry of the last thread's slice (t = T - 1)."""
    E, T, RB = sweep_shape(m)
    rows = sorted({n - 1, (n - 1) // RB * RB})
    tail = [j for j in (T - 1 + T * e for e in range(E)) if j < m]
    return rows, sorted({m - 1} | ({tail[-1]} if tail else set()))


def edge_mask(I, J, seed, frac=0.5, sparse=False):
    """A training mask observing about `frac` of the entries and the last row and column.  sparse=True: the edge rows of the row
    sweep and the edge columns of the column sweep (edge_entries) hold only a few dozen entries, among them their edge entries
    and (I - 1, J - 1), so that one misplaced entry moves their update by percent rather than by 1/m.  Every row and column
    stays observed."""
    rs = np.random.RandomState(seed)
    M = rs.rand(I, J) < frac
    rows, rtail = edge_entries(I, J)
    cols, ctail = edge_entries(J, I)
    if not sparse:
        M[-1, :] = True; M[:, -1] = True
        return M
    for i in rows:
        M[i, :] = False
        M[i, rs.choice(J, min(J, 30), replace=False)] = True
        M[i, rtail] = True
    for j in cols:
        M[:, j] = False
        M[rs.choice(I, min(I, 30), replace=False), j] = True
        M[ctail, j] = True
    M[I - 1, J - 1] = True
    free_r = [i for i in range(I) if i not in rows] or [0]
    free_c = [j for j in range(J) if j not in cols] or [0]
    for j in np.flatnonzero(~M.any(axis=0)):
        M[free_r[rs.randint(len(free_r))], j] = True
    for i in np.flatnonzero(~M.any(axis=1)):
        M[i, free_c[rs.randint(len(free_c))]] = True
    return M


def edge_problem(I, J, K, seed, sparse=False, L=None):
    """Positive data of rank K (or K, L), an edge_mask and a positive starting point: (R, M, U0, V0) or (R, M, F0, S0, G0)."""
    rs = np.random.RandomState(seed)
    if L is None:
        U0, V0 = rs.rand(I, K), rs.rand(J, K)
        R = U0 @ V0.T * (0.8 + 0.4 * rs.rand(I, J))
        return R, edge_mask(I, J, seed + 1, sparse=sparse), rs.rand(I, K) + 0.1, rs.rand(J, K) + 0.1
    R = rs.rand(I, K) @ rs.rand(K, L) @ rs.rand(J, L).T * (0.8 + 0.4 * rs.rand(I, J))
    return R, edge_mask(I, J, seed + 1, sparse=sparse), rs.rand(I, K) + 0.1, rs.rand(K, L) + 0.1, rs.rand(J, L) + 0.1


def rel_err(a, b):
    """Largest entrywise relative error of a against b."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.abs(b))) if b.size else 0.0
