"""The cases of the exact S-system test on the observed-entry layout (tests/_obs_tri_cases.py), without a GPU: the integer grids
stay below 2^24 in every intermediate -- so every entry of every state is a checked one --, nothing falls into the split products
the packed GEMM drops, the model is the system of the dense layout's tests on the same data, and every launch edge the cases
module names is hit by the case it names."""
import numpy as np

import _ssys_cases as SC
from _obs_tri_cases import CASES, COL_COUNTS, EDGES, LAM, TWO24, System, edges_of, problem


def test_every_intermediate_is_an_integer_below_2_to_the_24():
    for c in CASES:
        p = problem(c)
        assert p.M.sum(axis=0).min() > 0 and p.M.sum(axis=1).min() > 0, c.id
        for st in p.states:
            s = System(p, st)
            for name, v in s.budget.items():
                assert v < TWO24, (c.id, name, v)
            assert s.budget["dropped"] == 0 and s.ok.all() and s.ok.size == c.K * c.L, c.id
            for x in (s.W, s.Gc, s.Pv, s.A, s.b, s.num):
                assert np.array_equal(x, np.rint(x)), c.id
            assert np.array_equal(s.numer.astype(np.float64), s.num - LAM)          # (the half is exact below 2^23)
            assert len(set(st.S.reshape(-1).tolist())) == c.K * c.L and st.S.min() >= 1       # distinct: a wrong A[a][a'] moves numer_a


def test_the_model_is_the_dense_layouts_system():
    """W_j summed over the observed rows is C~f minus the missing rows' products: _ssys_cases.System on the same data."""
    for c in CASES:
        if c.I * c.J > 20000:
            continue
        p = problem(c)
        dense_case = SC.Case(c.I, c.J, c.K, c.L, ("X",), None)
        for st in p.states:
            d = SC.System(SC.Problem(dense_case, p.R, p.M.astype(np.uint8), {}, []), SC.State("X", st.F, st.S, st.G))
            s = System(p, st)
            assert np.array_equal(d.A, s.A) and np.array_equal(d.b, s.b) and np.array_equal(d.numer, s.numer) and np.array_equal(d.tau, s.tau), c.id


def test_every_named_edge_is_hit_by_the_case_that_is_named_for_it():
    by_name = {c.name: c for c in CASES}
    assert len(by_name) == len(CASES)
    hit = {c.name: edges_of(c) for c in CASES}
    for edge, name in EDGES.items():
        assert edge in hit[name], (edge, name, sorted(hit[name]))
    # what the issue lists: the (K, L) pairs, the column counts beside full columns, every J, I at 1 and 5, an entry value of 0
    for kl in ((1, 1), (2, 3), (31, 32), (32, 1), (32, 32)):
        assert "K,L=(%d,%d)" % kl in EDGES
    for n in COL_COUNTS:
        assert "column of %d" % n in EDGES
    assert COL_COUNTS == (1, 63, 64, 65, 129, 513) and "column of I" in EDGES
    for J in (1, 15, 16, 17, 63, 64, 65, 130):
        assert "J=%d" % J in EDGES
    assert "I=1" in EDGES and "I=5" in EDGES and "entry value 0" in EDGES
    # the launch of the counts case: two ranges of five 16-column steps, the second short; three blocks of b
    la = by_name["counts"].launch()
    assert (la["nsplit"], la["range"], la["last"], la["bblocks"]) == (2, 80, 50, 3)
