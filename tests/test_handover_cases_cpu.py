"""The cases of tests/_handover_cases.py hit the launch-shape classes they are there for, and its routing model tells a right
table from a wrong one -- from the host layouts alone (bnmtf_slot_layout), no GPU.

What tests/test_handover_exact_gpu.py then states on the device rests on four things checked here: every branch of the hand-over
code (the packet sender's descriptor passes and run lengths, the epilogue's offset table through the panel buffers or from
global memory, padded and empty runs, empty regions) is reached by a case; the routing model accepts the tables of a host
restatement of kernel_handover.hip and rejects seven kinds of damage; q of the entries of one reader block lies further apart
than the per-entry bound, so that an entry routed to its neighbour's place cannot pass; and one entry's q replaced by zero moves
its unit's row by far more than the tolerance of the comparison with the oracle."""
import copy

import numpy as np
import pytest

import _handover_cases as H
from _handover_cases import CASES, GIBBS_CASES, VB_CASES, FALLBACK_CASES, Case
from oracle import bnmtf_oracle as O


def _ids(cases):
    return [c.name for c in cases]


def _layouts(monkeypatch, case):
    case.setenv(monkeypatch)
    return case.layouts()


# the value of the writer epilogue's ho_lds per block of (rows, cols), for the cases that are there for it: recomputed in
# _handover_cases.writer_classes from pair_base / pair_E, pw and kChipPanelStride as sweep_chip.inc / kernel_sweep_vb.hip do.
# (A restatement: nothing on the device reports which branch a block took -- the dump is read-only -- so these pins hold the
# cases to the predicate as it is written today, and a change of the kernels' condition must be repeated in writer_classes.)
EXPECT_LDS = {
    "rank_1": ([False] * 4, [False] * 3),                 # K < 2: no column K - 2 to stage under
    "rank_2": ([True] * 4, [True] * 3),
    "rank_3": ([True] * 4, [True] * 3),
    "rank_4": ([True] * 4, [True] * 3),
    "rank_33": ([True] * 7, [True] * 5),
    "table_does_not_fit": ([True, False], [True] * 207),   # 36 + 25 pieces of room: 15 pairs of 32 slot rows take 60, 16 pairs 64
    "vb_pairs": ([False] * 3, [False] * 3),                # 4 pieces > chunks2 = 2
    "vb_pairs_long_rows": ([True, True], [False] * 16),    # rows: 2 x 2 slot rows = 4 pieces <= chunks2 = 6
}


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_case_hits_its_classes(monkeypatch, case):
    LR, LC = _layouts(monkeypatch, case)
    assert (LR.f_nw, LC.f_nw) == case.nw and (LR.ho_ppb, LC.ho_ppb) == case.nw, "block shapes"
    classes, lds, (cr, cc) = H.case_classes(case, LR, LC)
    assert cr.shape == case.blocks and cc.shape == case.blocks[::-1], "block counts"
    assert (cr == cc.T).all()
    assert case.classes <= classes, sorted(case.classes - classes)
    if case.name in EXPECT_LDS:
        assert (lds[0].tolist(), lds[1].tolist()) == EXPECT_LDS[case.name]
    # the second descriptor pass for the stated block shape: more reader blocks than 16 per wave and pass
    for tag, nbo, nw, count in (("rows", case.blocks[1], case.nw[0], cr), ("cols", case.blocks[0], case.nw[1], cc)):
        assert (("pass2_nw%d_%s" % (nw, tag)) in classes) == (nbo > 16 * nw)
        if nbo > 16 * nw:       # ... and the descriptors of that pass carry entries, from every writer block
            assert (count[:, 16 * nw:].sum(axis=1) > 0).all(), count[:, 16 * nw:].sum(axis=1)


def test_every_class_is_hit(monkeypatch):
    hit = {"gibbs": set(), "vb": set()}
    for case in CASES:
        hit[case.model] |= H.case_classes(case, *_layouts(monkeypatch, case))[0]
    assert H.GIBBS_REQUIRED <= hit["gibbs"], sorted(H.GIBBS_REQUIRED - hit["gibbs"])
    assert H.VB_REQUIRED <= hit["vb"], sorted(H.VB_REQUIRED - hit["vb"])
    # ... and by a case that names the class as its purpose, not by accident
    named = {m: set().union(*[c.classes for c in CASES if c.model == m]) for m in hit}
    assert H.GIBBS_REQUIRED <= named["gibbs"] and H.VB_REQUIRED <= named["vb"]


@pytest.mark.parametrize("name,I,J,K,frac,env,which,why", FALLBACK_CASES, ids=[f[0] for f in FALLBACK_CASES])
def test_fallback_cases_have_a_direction_without_blocks(monkeypatch, name, I, J, K, frac, env, which, why):
    case = Case(name, "gibbs", I, J, K, ("uniform", frac, 0), env, None, None, "")
    L = _layouts(monkeypatch, case)
    assert L[which].ho_ppb == 0 and L[1 - which].ho_ppb == 8
    if why == "gen_units":
        assert len(L[which].gen_units) > 0 and L[which].f_nw == 8
    else:
        assert len(L[which].gen_units) == 0 and L[which].f_nw == 2


# ------------------------------------------------------------------------------------------------ the routing model
MODEL_CASES = [c for c in GIBBS_CASES if c.name in ("runs_straddle_128", "runs_straddle_256", "empty_runs_residues", "second_pass_8_waves_rows",
                                                     "nothing_missing", "table_does_not_fit")]


def _check_both(LR, LC, DR, DC):
    return H.check_routing(LR, LC, DR, DC, True), H.check_routing(LC, LR, DC, DR, False)


@pytest.mark.parametrize("case", MODEL_CASES, ids=_ids(MODEL_CASES))
def test_routing_model_accepts_the_restated_tables_and_rejects_damage(monkeypatch, case):
    LR, LC = _layouts(monkeypatch, case)
    DR, DC = H.host_tables(LR, LC)
    P, _ = _check_both(LR, LC, DR, DC)                     # P: rows write, cols read
    if P.n == 0:
        return
    sW, sR = P.sW, P.sR

    def damaged():
        return copy.deepcopy(DR), copy.deepcopy(DC)
    # a run with two entries or more, and its first two entries in slot order
    grp = P.bw * sR.nb + P.br
    g = np.nonzero(P.count.ravel() >= 2)[0][0]
    a, b = np.nonzero(grp == g)[0][:2]
    out = H.places(DR.t_out, sW.S)
    # two entries swapped inside a run
    dr, dc = damaged()
    H.set_place(dr.t_out, P.wrow[a], P.wlane[a], out[P.wrow[b], P.wlane[b]])
    H.set_place(dr.t_out, P.wrow[b], P.wlane[b], out[P.wrow[a], P.wlane[a]])
    with pytest.raises(AssertionError, match="packet's start plus the writer's rank"):
        _check_both(LR, LC, dr, dc)
    # a run shifted by one: every writer place of the run
    dr, dc = damaged()
    for e in np.nonzero(grp == g)[0]:
        H.set_place(dr.t_out, P.wrow[e], P.wlane[e], out[P.wrow[e], P.wlane[e]] + 1)
    with pytest.raises(AssertionError, match="outside its run|share a writer place"):
        _check_both(LR, LC, dr, dc)
    # ... and every reader place of it
    dr, dc = damaged()
    tin = H.places(DC.t_in, sR.S)
    for e in np.nonzero(grp == g)[0]:
        H.set_place(dc.t_in, P.rrow[e], P.rlane[e], tin[P.rrow[e], P.rlane[e]] + 1)
    with pytest.raises(AssertionError, match="packet's start plus the writer's rank"):
        _check_both(LR, LC, dr, dc)
    # an empty slot of the reader pointed at a live place, one of the writer likewise
    dr, dc = damaged()
    er, el = [x[0] for x in np.nonzero(~sR.live)]
    H.set_place(dc.t_in, er, el, tin[P.rrow[a], P.rlane[a]])
    with pytest.raises(AssertionError, match="empty slot of the reader"):
        _check_both(LR, LC, dr, dc)
    dr, dc = damaged()
    er, el = [x[0] for x in np.nonzero(~sW.live)]
    H.set_place(dr.t_out, er, el, out[P.wrow[a], P.wlane[a]])
    with pytest.raises(AssertionError, match="empty slot of the writer"):
        _check_both(LR, LC, dr, dc)
    # a packet one group of four short
    dr, dc = damaged()
    dr.pk[g // sR.nb, g % sR.nb, 1] -= 4
    with pytest.raises(AssertionError, match="padded to four"):
        _check_both(LR, LC, dr, dc)
    # a packet that starts one group early in the reader's region
    dr, dc = damaged()
    g2 = np.nonzero(P.count.ravel() >= 1)[0][-1]
    dr.pk[g2 // sR.nb, g2 % sR.nb, 2] -= 4
    with pytest.raises(AssertionError):
        _check_both(LR, LC, dr, dc)


# ------------------------------------------------------------------------------------------------ separation
def _chain_states(case):
    """the fp64 states of the per-entry data: case.sep_chain mode iterations (Gibbs), one variational iteration"""
    R, M, U0, V0, pri = case.data(case.spread)
    if case.model == "gibbs":
        Us, Vs, _ = H.gibbs_mode_chain(R, M, U0, V0, 1.0, pri, case.sep_chain)
        return Us, Vs
    o = O.BNMFVBOracle(R, M, case.K, pri)
    H.vb_set_state(o, U0, V0, 1.0)
    eU0, eV0 = o.expU.copy(), o.expV.copy()
    o.sweep()
    return [eU0, o.expU.copy()], [eV0, o.expV.copy()]


SEP_CASES = [c for c in CASES if c.mask[0] != "full"]


@pytest.mark.parametrize("case", SEP_CASES, ids=_ids(SEP_CASES))
def test_q_of_a_reader_block_lies_further_apart_than_the_bound(monkeypatch, case):
    """A cap, not a measurement: below 1 % of the entries of either region have another q of the same reader block within twice
    their bound, after one mode iteration and after three (one variational iteration; table_does_not_fit after one only: see
    sep_chain in _handover_cases.py).  The states are the fp64 chain's; the GPU test repeats the statement on the device's own
    states.  After draws the states are the device's alone: there the GPU test prints the share."""
    LR, LC = _layouts(monkeypatch, case)
    Us, Vs = _chain_states(case)
    for region, P in (("cols", H.pairing(LR, LC, True)), ("rows", H.pairing(LC, LR, False))):
        for n in sorted({1, case.sep_chain}):
            q, bound = H.chain_reference(Us[:n + 1], Vs[:n + 1], case.K, case.KP, region, P.i, P.j)
            assert (bound > 0).all() and (bound < 1e-4 * np.abs(q).max()).all()
            share = H.close_share(q, bound, P.br)
            assert share < 0.01, "%s region after %d: %.4f of the entries have a neighbour within twice the bound" % (region, n, share)


# ------------------------------------------------------------------------------------------------ sensitivity of the reader side
@pytest.mark.parametrize("case", SEP_CASES, ids=_ids(SEP_CASES))
def test_one_q_replaced_by_zero_moves_its_row_by_20_tolerances(monkeypatch, case):
    """(The variational cases too, on their masks and data with the mode update: a q read as zero enters their numerator the same way.)
    The reader side compares U and V with the oracle per element, scaled by the row's largest value, to READER_TOL.  A reader
    that took zero for ONE missing entry of a unit sees that entry's q as part of the residual: in the residual form, E_ij = q_ij
    instead of 0.  For 99 % of the units of a case (both directions) that moves the unit's row by 20 tolerances or more."""
    from _residual_form import mode_sweep
    R, M, U0, V0, pri = case.data(0.0)
    moved = []
    for X0, Y0, Mm, Rm, lam in ((U0, V0, M, R, pri["lambdaU"]), (V0, U0, np.ascontiguousarray(M.T), np.ascontiguousarray(R.T), pri["lambdaV"])):
        E = Mm * (Rm - X0 @ Y0.T)
        X = X0.copy(); mode_sweep(E.copy(), X, Y0, Mm, 1.0, lam)
        units = np.nonzero((Mm == 0).any(axis=1))[0]
        first = (Mm[units] == 0).argmax(axis=1)
        E2 = E.copy(); E2[units, first] = (X0[units] * Y0[first]).sum(axis=1)
        X2 = X0.copy(); mode_sweep(E2, X2, Y0, Mm, 1.0, lam)
        moved.append(np.abs(X2 - X)[units].max(axis=1) / np.abs(X)[units].max(axis=1))
    moved = np.concatenate(moved)
    assert np.mean(moved >= 20 * H.READER_TOL) >= 0.99, np.mean(moved >= 20 * H.READER_TOL)
