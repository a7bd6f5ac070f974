"""Pins of the exact S-system cases (tests/_ssys_cases.py; the GPU side: test_ssys_exact_gpu.py), on the CPU:
  (a) every case sits on the launch it names (csrc/api_models.inc: nsplit, the GEMM's column ranges, b's blocks), and its
      checked entries are exact: every intermediate within 2^24, the dropped split products zero on them;
  (b) the cases would see a wrong kernel: each mutation of the system below changes a checked output (numer or tauS);
  (c) the cases cover the launch edges and the missing-count classes."""
import numpy as np
import pytest

from _contraction_cases import DROPPED, PRODUCTS, TWO24
from _ssys_cases import (CASES, LAM, MISS_CLASSES, MU_ULPS, VB_NUMER_MAX, System, problem, row_path_ok, slots, split3, ssys_launch,
                         tri_count, tri_padded, tri_pos, vb_states)

DENSE = [c for c in CASES if c.dense]
_CACHE = {}


def _systems(case):
    """(problem, [(state, System)]) of a case, built once per session"""
    if case.id not in _CACHE:
        p = problem(case)
        _CACHE[case.id] = (p, [(st, System(p, st)) for st in p.states])
    return _CACHE[case.id]


def _launch_fields(case):
    ln = case.launch()
    return dict(tri_padded=ln["tri_padded"], nsplit=ln["nsplit"], range=ln["range"], empty=ln["empty"], bblocks=ln["bblocks"])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_sits_on_its_launch_and_is_exact(case):
    if case.expect is not None:
        assert _launch_fields(case) == case.expect
    else:
        assert not case.launch()["on"]
    p, systems = _systems(case)
    for st, s in systems:
        if st.varF is not None:
            continue
        ok = s.ok
        # the X family is exact everywhere; the split families leave out only the rows of their wide column
        assert ok.all() if st.fam == "X" else ok.sum() >= s.n2 // 2, (st.fam, ok.sum(), s.n2)
        a_k, a_l = np.divmod(np.arange(s.n2), s.L)
        kok, lok = np.zeros(s.K, bool), np.zeros(s.L, bool)
        kok[np.unique(a_k[ok])] = True; lok[np.unique(a_l[ok])] = True
        # every intermediate on a checked entry, listed: C~f (fp64 -> fp32), the Gram's partial sums and W_j, Gc, the GEMM's
        # slab / half sums (bounded by the whole sum of |split products|), Pv, b's partials and b, r = b - A S and r + S_a A_aa
        kk, ll = s.kk, s.ll
        for name in ("cf", "gram", "W"):
            v = s.budget[name]
            assert np.all((v if v.ndim == 2 else v[None])[:, kok[kk[:, 0]] | kok[kk[:, 1]]] < TWO24), (st.fam, name)
        assert np.all(s.budget["Gc"][:, lok[ll[:, 0]] | lok[ll[:, 1]]] < TWO24), st.fam
        assert np.all(s.unpack(s.budget["gemm"])[ok] < TWO24), st.fam
        assert np.all(s.budget["pv"][:, kok] < TWO24) and np.all(s.budget["b"][ok] < TWO24), st.fam
        assert np.all(s.budget["r"][ok] < TWO24), st.fam
        sA = np.abs(s.S.reshape(-1) * np.diag(s.A))
        assert np.all(sA[ok] < TWO24) and np.all(np.abs(s.num[ok]) < TWO24), st.fam
        assert np.all(s.num == np.rint(s.num)) and np.all(s.tau[ok] == np.rint(s.tau[ok])), st.fam
        # the dropped products: zero in both bf16x3 kernels wherever a checked entry reads
        for a, b in DROPPED:
            g = s.miss.T @ s.gram_prod[(a, b)]
            assert not np.any(g[:, kok[kk[:, 0]] | kok[kk[:, 1]]]), (st.fam, "scol_gram %s.%s" % (a, b))
            d = s.sW[a].astype(np.float64).T @ s.sG[b].astype(np.float64)
            assert not np.any(s.unpack(np.abs(d))[ok]), (st.fam, "ssys_gemm %s.%s" % (a, b))
        # the per-row path: the states it runs are exact there too (its own intermediates: row_path_ok)
        if st.fam == "X":
            assert row_path_ok(p, st, s).all(), case.id
    for st in vb_states(p):
        s = System(p, st, vb=True)
        assert s.ok.all(), (case.id, "VB")
        # muS = numer (1 / tau_p): an error of one unit in numer moves muS by more than twice the rounding bound
        assert np.abs(s.num).max() - LAM < VB_NUMER_MAX, np.abs(s.num).max()
        q = (s.num - LAM) / s.tau
        ulp = np.spacing(np.abs(q).astype(np.float32)).astype(np.float64)
        assert np.all(1.0 / s.tau > 2 * MU_ULPS * ulp), case.id


def _mutations(case, p, s, st):
    """name -> did this mutation move a checked output (None: not applicable to this state)"""
    out = {}
    J, K, L = case.J, case.K, case.L
    for pr in PRODUCTS:                                      # scol_gram: the product left out of the subtracted missing Gram
        d = s.miss.T @ s.gram_prod[pr]
        out["scol_gram drops %s.%s" % pr] = s.moved_by_W(d) if d.any() else None
    for a, b in PRODUCTS:                                    # ssys_gemm: the product left out of A
        d = s.sW[a].astype(np.float64).T @ s.sG[b].astype(np.float64)
        out["ssys_gemm drops %s.%s" % (a, b)] = s.moved_by_Ap(-d) if d.any() else None
    ln = ssys_launch(K, L, J)
    for r, (j0, j1) in enumerate(ln["ranges"]):
        if j0 < j1:
            d = s.W[j0:j1].T @ s.Gc[j0:j1]
            out["range %d dropped" % r] = s.moved_by_Ap(-d)
            out["range %d added twice" % r] = s.moved_by_Ap(d)
    k_of = np.repeat(np.arange(K), L)
    if K > 1:
        out["mirror write skipped"] = s.moved_by_A(-s.A * (k_of[:, None] > k_of[None, :]))
    for name, which in (("tri_pos tiles swapped in Wc", "W"), ("tri_pos tiles swapped in Gc", "G")):
        X = s.W if which == "W" else s.Gc
        n = X.shape[1]
        src = np.arange(n) ^ 32
        Xs = np.where(src[None, :] < n, X[:, np.minimum(src, n - 1)], 0.0)
        if n > 32:
            out[name] = s.moved_by_Ap((Xs - X).T @ s.Gc if which == "W" else s.W.T @ (Xs - X))
    nb = ln["bblocks"]
    out["last b block dropped"] = s.moved(-s.PvG[64 * (nb - 1):].sum(axis=0).reshape(-1))
    out["S_a A_aa dropped"] = s.moved(-s.S.reshape(-1) * np.diag(s.A))
    # the missing lists: one entry of a class column dropped (its first and its last: rows 0 / I - 1 among them), the first slot
    # of each 64-slot block read twice
    for c, j in p.cols.items():
        rows = np.flatnonzero(p.M[:, j] == 0)
        if len(rows) == 0:
            continue
        for tag, i in (("first", rows[0]), ("last", rows[-1])):
            dW = np.zeros_like(s.W); dW[j] = s.FF[i]
            out["class %s column: %s missing entry dropped" % (c, tag)] = s.moved_by_W(dW)
        for blk in range((len(rows) + 63) // 64):
            dW = np.zeros_like(s.W); dW[j] = -s.FF[rows[64 * blk]]
            out["class %s column: slot %d read twice" % (c, 64 * blk)] = s.moved_by_W(dW)
    return out


def test_each_mutation_moves_a_checked_output():
    caught = {}
    per_case_missed = []
    for case in DENSE:
        p, systems = _systems(case)
        here = {}
        for st, s in systems:
            if st.varF is not None:
                continue
            for name, got in _mutations(case, p, s, st).items():
                if got is None:
                    continue
                here[name] = here.get(name, False) or got
                if got and name not in caught:
                    caught[name] = "%s %s" % (case.id, st.fam)
        # every range, the mirror, the b block, the missing lists: caught in the case itself
        for name, got in here.items():
            if not name.startswith(("scol_gram", "ssys_gemm")) and not got:
                per_case_missed.append((case.id, name))
    for name in sorted(caught):
        print("%-50s caught by %s" % (name, caught[name]))
    want = {"scol_gram drops %s.%s" % pr for pr in PRODUCTS} | {"ssys_gemm drops %s.%s" % pr for pr in PRODUCTS}
    want |= {"mirror write skipped", "tri_pos tiles swapped in Wc", "tri_pos tiles swapped in Gc", "last b block dropped",
             "S_a A_aa dropped", "range 0 dropped", "range 0 added twice"}
    assert want <= set(caught), sorted(want - set(caught))
    assert not per_case_missed, per_case_missed
    assert any("slot 64 read twice" in n for n in caught)


def test_cases_cover_the_launch_edges_and_mask_classes():
    tk, tl, flags, classes = set(), set(), set(), set()
    for case in DENSE:
        ln = case.launch()
        tk.add(ln["tri_padded"][0]); tl.add(ln["tri_padded"][1])
        flags.add("nsplit=%s" % ln["limit"])
        if ln["empty"]:
            flags.add("empty trailing ranges")
        if ln["last"] < ln["range"]:
            flags.add("short last range")
        flags.add("J mod 16 = %d" % (case.J % 16))
        if case.J < 16:
            flags.add("J < 16")
        if case.J % 64 == 1:
            flags.add("J mod 64 = 1")
        p, _ = _systems(case)
        for c, j in p.cols.items():
            n = int((p.M[:, j] == 0).sum())
            assert n == (case.I - 1 if c == "I-1" else c), (case.id, c, n)
            assert slots(n) == {0: 0, 1: 64, 63: 64, 64: 64, 65: 128, 128: 128}.get(c, slots(case.I - 1))
            classes.add(c)
        if case.J > 1:
            if (p.M[0] == 0).any():
                flags.add("missing at row 0")
            if (p.M[-1] == 0).any():
                flags.add("missing at row I-1")
    assert tk == set(range(64, 577, 64)) and tl == set(range(64, 577, 64)), (sorted(tk), sorted(tl))
    assert flags >= {"nsplit=one", "nsplit=cap", "nsplit=tiles", "empty trailing ranges", "short last range", "J mod 16 = 1",
                     "J mod 16 = 15", "J < 16", "J mod 64 = 1", "missing at row 0", "missing at row I-1"}, flags
    assert classes == set(MISS_CLASSES), classes
    # the issue's table of launches, every row of it
    table = {(1, 1, 1): (64, 64, 1, 16, 0, 1), (10, 11, 17): (64, 128, 1, 32, 0, 1), (11, 3, 2047): (128, 64, 31, 80, 5, 32),
             (16, 20, 2049): (192, 256, 32, 80, 6, 33), (23, 25, 700): (320, 384, 10, 80, 1, 11),
             (28, 30, 3000): (448, 512, 32, 96, 0, 47), (32, 32, 4096): (576, 576, 24, 176, 0, 64),
             (32, 1, 9000): (576, 64, 32, 288, 0, 141), (3, 32, 65): (64, 576, 1, 80, 0, 2)}
    have = {(c.K, c.L, c.J) for c in DENSE}
    for (K, L, J), want in table.items():
        assert (K, L, J) in have
        ln = ssys_launch(K, L, J)
        assert (ln["tri_padded"][0], ln["tri_padded"][1], ln["nsplit"], ln["range"], ln["empty"], ln["bblocks"]) == want
    assert ssys_launch(32, 32, 4096)["last"] == 48 and ssys_launch(16, 20, 2049)["last"] == 49
    per_row = [c for c in CASES if not c.dense]
    assert per_row and all(33 <= max(c.K, c.L) <= 64 for c in per_row)


def test_packing_helpers():
    # tri_pos interleaves the two 32-wide tiles of every 64 packed pairs, and is a permutation of the padded row
    assert [tri_count(K) for K in (1, 11, 32)] == [1, 66, 528] and [tri_padded(K) for K in (1, 11, 32)] == [64, 128, 576]
    assert [tri_pos(p) for p in (0, 1, 31, 32, 33, 63, 64, 96)] == [0, 2, 62, 1, 3, 63, 64, 65]
    assert sorted(tri_pos(p) for p in range(576)) == list(range(576))
    s = split3(np.array([2 ** 17 + 3], np.float32))
    assert s["l"][0] == 0                                      # (17 bits split into hi + mid exactly: the lo families use 18)
