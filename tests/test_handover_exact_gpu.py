"""The q hand-over between the half sweeps, entry by entry, at every launch shape (cases and routing model:
tests/_handover_cases.py; the classes the cases hit: tests/test_handover_cases_cpu.py).

Three statements per case, each through the library's read-only entry bnmtf_handover_dump:
  tables   -- exact integers: the routing model follows every entry of the mask from its slot at the writer through the staging
              area and the packet into the reader's region, and every empty slot to the zeros;
  regions  -- every handed-over fp32 value against the fp64 dot product of the states the device reported, within the forward
              error bound of the chain of fp32 operations that made it (derived in _handover_cases.chain_reference), after one
              and three mode iterations and after two iterations of draws; the 32 zeros behind every block's runs exactly 0.0;
  reader   -- two mode iterations with the hand-over against the fp64 oracle, per element scaled by the row's largest value,
              to 8 x the largest deviation of the pre-pass run (BNMTF_HANDOVER=0: the parent's code) over all cases.
One wrong entry is an O(q) error against a bound of a few fp32 roundings; the existing hand-over tests see it only after a
column update over hundreds of entries has diluted it."""
import re

import numpy as np
import pytest

import _handover_cases as H
from _handover_cases import GIBBS_CASES, VB_CASES, FALLBACK_CASES, Case
from bnmtf_amd import _lib, bnmf_gibbs_optimised, bnmf_vb_optimised
from oracle import bnmtf_oracle as O

pytestmark = pytest.mark.gpu

BNMTF_ESTATE = -5


def _ids(cases):
    return [c.name for c in cases]


def _model(case, R, M, pri):
    if case.model == "gibbs":
        b = bnmf_gibbs_optimised(R, M, case.K, pri, verbose=False, seed=5)
    else:
        b = bnmf_vb_optimised(R, M, case.K, pri, verbose=False)
    d = b.describe()
    assert "handover=1" in d, d
    assert tuple(int(x) for x in re.findall(r"sweep_nw=(\d+)", d)) == case.nw, d
    return b


def _dumps(b):
    return H.handover_dump(b._handle(), 0), H.handover_dump(b._handle(), 1)


def _routing(case, b):
    """the routing model on the handle's tables: (entries of the cols region: rows write, cols read; entries of the rows region)"""
    LR, LC = case.layouts()
    DR, DC = _dumps(b)
    assert (DR.blocks, DC.blocks) == case.blocks and (DR.ppb, DC.ppb) == case.nw
    return H.check_routing(LR, LC, DR, DC, True), H.check_routing(LC, LR, DC, DR, False)


ALL = GIBBS_CASES + VB_CASES


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_tables_route_every_entry(monkeypatch, case):
    """Exact integers, after bnmtf_create: every missing entry's writer place is its own inside the run (bw, br) that pk describes;
    pk starts and lengths are multiples of 4 and the runs disjoint in the staging areas and in the regions, below the 32 zeros of
    their region; the reader's place is the packet's region start plus the same rank; every empty slot points into the zeros
    (reader) or the dump words behind the runs (writer); every place and region size fits 16 bits and ho_lds_floats; region
    offsets are ascending multiples of 256.  The regions themselves are all zero and flagged as not filled."""
    case.setenv(monkeypatch)
    R, M, U0, V0, pri = case.data(case.spread)
    b = _model(case, R, M, pri)
    Pc, Pr = _routing(case, b)
    assert Pc.n == Pr.n == int((M == 0).sum())
    for D in _dumps(b):
        assert D.filled == 0 and D.regions_current == 0 and not D.region.any()
        assert len(D.region) == int(D.region_ofs[-1]) + 256


def _set_and_run(case, b, U0, V0, n, mode):
    """from the set state: the states the device reports, as lists [X_0 .. X_n] of fp32 values"""
    if case.model == "gibbs":
        b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.0
        b.run(n, update="mode") if mode else b.run(n)
        return [U0] + [np.array(x) for x in b.all_U], [V0] + [np.array(x) for x in b.all_V]
    assert n == 1
    H.vb_set_state(b, U0, V0, 1.0)
    eU0, eV0 = b.expU.astype(np.float32).astype(np.float64), b.expV.astype(np.float32).astype(np.float64)
    b.run(1)
    return [eU0, b.expU.copy()], [eV0, b.expV.copy()]


def _check_regions(case, b, P, Us, Vs, what, cap_share):
    """both regions against the chain of the reported states; returns the largest error / bound"""
    worst = 0.0
    DR, DC = _dumps(b)
    assert DR.filled == 1 and DR.regions_current == 1, "the run left the rows region filled"
    for region, Pn, D in (("cols", P[0], DC), ("rows", P[1], DR)):
        # the 32 zeros behind every block's runs
        assert not D.region[Pn.zeros[:, None] + np.arange(32)[None, :]].any(), "%s: %s region: zeros overwritten" % (what, region)
        if Pn.n == 0:
            continue
        q, bound = H.chain_reference(Us, Vs, case.K, case.KP, region, Pn.i, Pn.j)
        got = D.region[Pn.gidx].astype(np.float64)
        ratio = np.abs(got - q) / bound
        share = H.close_share(q, bound, Pn.br)
        print("HO-MEASURE %s %s %s region: max error/bound %.3f, median %.3f; %.4f of the entries within twice the bound of a neighbour"
              % (case.name, what, region, ratio.max(), np.median(ratio), share))
        if cap_share:
            assert share < 0.01, "%s: %s region: %.4f of the entries have a neighbour within twice the bound" % (what, region, share)
        bad = np.nonzero(~(ratio <= 1.0))[0]
        assert len(bad) == 0, "%s: %s region: %d of %d entries off by more than the bound, first (i=%d, j=%d): %r for %r (bound %.3g)" % (
            what, region, len(bad), Pn.n, Pn.i[bad[0]], Pn.j[bad[0]], got[bad[0]], q[bad[0]], bound[bad[0]])
        worst = max(worst, float(ratio.max()))
    return worst


@pytest.mark.parametrize("case", GIBBS_CASES, ids=_ids(GIBBS_CASES))
def test_regions_hold_q_of_every_entry_gibbs(monkeypatch, case):
    """run(1, update='mode') from a set state, refresh off: the rows region holds q of (U_1, V_1), the cols region q of (U_1, V_0),
    every entry within the chain's forward error bound of the fp64 dot product of the reported states; again from the set state
    after run(3, update='mode') (a chain three times as long) and after run(2) of draws.

    Largest error / bound on an MI355X, over both regions and the three runs (the bound is a worst case over c = KP + 2 K H
    roundings that mostly cancel: the ratio stays far below 1):
      runs_straddle_128          mode x 1 0.113, mode x 3 0.092, draws x 2 0.086
      runs_straddle_256          mode x 1 0.124, mode x 3 0.113, draws x 2 0.107
      runs_all_long              mode x 1 0.119, mode x 3 0.123, draws x 2 0.104
      runs_many_trips            mode x 1 0.107, mode x 3 0.104, draws x 2 0.082
      second_pass_16_waves       mode x 1 0.117, mode x 3 0.096, draws x 2 0.109
      second_pass_8_waves_rows   mode x 1 0.118, mode x 3 0.103, draws x 2 0.106
      second_pass_8_waves_cols   mode x 1 0.128, mode x 3 0.109, draws x 2 0.097
      empty_runs_sparse          mode x 1 0.110, mode x 3 0.072, draws x 2 0.085
      empty_runs_residues        mode x 1 0.087, mode x 3 0.056, draws x 2 0.044
      nothing_missing            mode x 1 0.000, mode x 3 0.000, draws x 2 0.000
      rank_1                     mode x 1 0.054, mode x 3 0.082, draws x 2 0.060
      rank_2                     mode x 1 0.086, mode x 3 0.123, draws x 2 0.073
      rank_3                     mode x 1 0.074, mode x 3 0.088, draws x 2 0.070
      rank_4                     mode x 1 0.098, mode x 3 0.086, draws x 2 0.075
      rank_33                    mode x 1 0.082, mode x 3 0.059, draws x 2 0.050
      table_does_not_fit         mode x 1 0.102, mode x 3 0.134, draws x 2 0.095
      per_wave_sampler           mode x 1 0.113, mode x 3 0.092, draws x 2 0.086
    The separation of q inside a reader block (under 1 % of the entries with a neighbour within twice the bound) is asserted on
    the device's states after the mode iterations, as the CPU file asserts it on the fp64 chain's (table_does_not_fit after the
    one iteration only, 1.3 % after three: sep_chain in _handover_cases.py); after the draws, whose states no host chain
    foretells, the share is printed (3.4 % in the 32 000-entry rows blocks of table_does_not_fit, 1.3 % for rank_33, below
    1 % everywhere else)."""
    case.setenv(monkeypatch)
    R, M, U0, V0, pri = case.data(case.spread)
    b = _model(case, R, M, pri)
    P = _routing(case, b)
    worst = {}
    for what, n, mode in (("mode x 1", 1, True), ("mode x 3", 3, True), ("draws x 2", 2, False)):
        Us, Vs = _set_and_run(case, b, U0, V0, n, mode)
        assert all(np.isfinite(x).all() for x in Us + Vs)
        worst[what] = _check_regions(case, b, P, Us, Vs, what, cap_share=(mode and n <= case.sep_chain))
    print("HO-RATIO %s: %s" % (case.name, ", ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("case", VB_CASES, ids=_ids(VB_CASES))
def test_regions_hold_q_of_every_entry_vb(monkeypatch, case):
    """The same for one variational iteration, the states being E[U] and E[V]: the pair-panel kernel (BNMTF_VB_PATH=pairs,
    16-wave blocks) and the on-chip kernel with the masked sums (=masked, 16- and 8-wave blocks).

    Largest error / bound on an MI355X:
      vb_pairs                   0.085
      vb_pairs_long_rows         0.075
      vb_masked_16_waves         0.073
      vb_masked_8_waves          0.073"""
    case.setenv(monkeypatch)
    R, M, U0, V0, pri = case.data(case.spread)
    b = _model(case, R, M, pri)
    P = _routing(case, b)
    Us, Vs = _set_and_run(case, b, U0, V0, 1, True)
    assert ("vb_sweep=" + case.env["BNMTF_VB_PATH"]) in b.describe(), b.describe()
    worst = _check_regions(case, b, P, Us, Vs, "vb x 1", cap_share=True)
    print("HO-RATIO %s: vb x 1 %.3f" % (case.name, worst))


# ------------------------------------------------------------------------------------------------ the reader side
def _row_scaled(x, ref):
    ref = np.asarray(ref)
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    return float((np.abs(np.asarray(x) - ref) / np.where(scale > 0, scale, 1.0)).max())


def _oracle_two_iterations(case, R, M, U0, V0, pri):
    """(U, V, tau) of iterations 1 and 2: the as-written oracle, or its residual form for the 4100- and 8200-unit cases"""
    if case.model == "vb":
        o = O.BNMFVBOracle(R, M, case.K, pri)
        H.vb_set_state(o, U0, V0, 1.0)
        o.sweep(); o.sweep()
        return o.expU, o.expV, o.exptau
    if max(case.I, case.J) >= 4000:
        Us, Vs, taus = H.gibbs_mode_chain(R, M, U0, V0, 1.0, pri, 2)
        return np.array(Us[1:]), np.array(Vs[1:]), np.array(taus)
    o = O.BNMFGibbsOracle(R, M, case.K, pri)
    o.U, o.V, o.tau = U0.copy(), V0.copy(), 1.0
    o.run(2, draw=False)
    return o.all_U, o.all_V, o.all_tau


def _device_two_iterations(case, R, M, U0, V0, pri):
    if case.model == "vb":
        b = bnmf_vb_optimised(R, M, case.K, pri, verbose=False)
        H.vb_set_state(b, U0, V0, 1.0)
        b.run(2)
        return b.describe(), (b.expU, b.expV, b.exptau)
    b = bnmf_gibbs_optimised(R, M, case.K, pri, verbose=False, seed=5)
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.0
    b.run(2, update="mode")
    return b.describe(), (np.array(b.all_U), np.array(b.all_V), np.array(b.all_tau))


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_reader_side_follows_the_oracle(monkeypatch, case):
    """run(2, update='mode') (VB: run(2)) with the hand-over -- the second iteration's rows sweep and both cols sweeps start from
    a region instead of the pre-pass -- against the fp64 oracle, per element of U, V and tau scaled by the row's largest value.
    The tolerance READER_TOL is 8 x the largest deviation of the PRE-PASS run from the oracle over all cases, as one number;
    test_handover_cases_cpu.py shows that one entry's q taken as zero moves its row by 20 tolerances or more.

    Deviation of the pre-pass run from the oracle on an MI355X (U, V, tau), and of the hand-over run:
      runs_straddle_128          pre-pass 1.21e-06 9.37e-07 1.67e-07   hand-over 1.07e-06 1.07e-06 1.08e-06
      runs_straddle_256          pre-pass 2.85e-06 2.47e-06 6.41e-07   hand-over 2.78e-06 2.56e-06 7.28e-07
      runs_all_long              pre-pass 1.74e-06 1.93e-06 8.05e-07   hand-over 2.13e-06 1.92e-06 3.34e-07
      runs_many_trips            pre-pass 1.22e-06 2.20e-06 4.29e-07   hand-over 2.32e-06 1.43e-06 1.30e-07
      second_pass_16_waves       pre-pass 1.13e-06 1.84e-06 4.12e-07   hand-over 1.13e-06 1.89e-06 4.14e-07
      second_pass_8_waves_rows   pre-pass 1.47e-06 2.71e-06 3.71e-07   hand-over 1.19e-06 3.01e-06 3.62e-07
      second_pass_8_waves_cols   pre-pass 3.05e-06 1.36e-06 8.39e-07   hand-over 2.38e-06 1.55e-06 1.24e-06
      empty_runs_sparse          pre-pass 1.95e-06 1.85e-06 6.05e-07   hand-over 1.54e-06 2.41e-06 6.75e-07
      empty_runs_residues        pre-pass 1.77e-06 1.96e-06 8.21e-07   hand-over 1.64e-06 2.10e-06 3.62e-07
      nothing_missing            pre-pass 6.27e-07 8.30e-07 7.70e-08   hand-over 6.27e-07 8.30e-07 7.70e-08
      rank_1                     pre-pass 3.40e-07 2.61e-07 7.78e-08   hand-over 3.40e-07 2.61e-07 5.34e-08
      rank_2                     pre-pass 7.74e-07 6.95e-07 3.13e-07   hand-over 9.01e-07 7.78e-07 2.04e-07
      rank_3                     pre-pass 1.01e-06 7.43e-07 3.58e-07   hand-over 1.23e-06 7.01e-07 3.89e-07
      rank_4                     pre-pass 2.03e-06 1.15e-06 3.67e-07   hand-over 1.34e-06 1.33e-06 7.88e-07
      rank_33                    pre-pass 7.36e-06 9.88e-06 6.93e-06   hand-over 6.52e-06 9.14e-06 2.72e-06
      table_does_not_fit         pre-pass 6.57e-07 1.07e-06 7.24e-08   hand-over 6.57e-07 1.07e-06 6.70e-08
      per_wave_sampler           pre-pass 1.21e-06 9.37e-07 1.67e-07   hand-over 1.07e-06 1.07e-06 1.08e-06
      vb_pairs                   pre-pass 1.03e-06 1.54e-06 2.69e-07   hand-over 1.07e-06 1.17e-06 5.95e-07
      vb_pairs_long_rows         pre-pass 1.31e-06 2.40e-06 2.37e-07   hand-over 1.10e-06 2.72e-06 1.96e-07
      vb_masked_16_waves         pre-pass 1.07e-06 2.10e-06 1.02e-07   hand-over 1.17e-06 1.89e-06 8.66e-07
      vb_masked_8_waves          pre-pass 1.20e-06 2.02e-06 2.79e-07   hand-over 9.98e-07 1.58e-06 6.79e-08
    The largest pre-pass deviation is rank_33's 9.88e-06 (V): READER_TOL = 8 x 9.88e-06 = 7.9e-05."""
    R, M, U0, V0, pri = case.data(0.0)
    ref = _oracle_two_iterations(case, R, M, U0, V0, pri)
    dev = {}
    for ho in ("0", "1"):
        case.setenv(monkeypatch, BNMTF_HANDOVER=ho)
        d, got = _device_two_iterations(case, R, M, U0, V0, pri)
        assert ("handover=%s" % ho) in d and tuple(int(x) for x in re.findall(r"sweep_nw=(\d+)", d)) == case.nw, d
        dev[ho] = (_row_scaled(got[0], ref[0]), _row_scaled(got[1], ref[1]), float(np.max(np.abs(np.asarray(got[2]) / np.asarray(ref[2]) - 1.0))))
    print("HO-DEVIATION %s: pre-pass %.2e %.2e %.2e, hand-over %.2e %.2e %.2e" % ((case.name,) + dev["0"] + dev["1"]))
    assert max(dev["1"]) <= H.READER_TOL, dev


# ------------------------------------------------------------------------------------------------ where the tables must not be built
@pytest.mark.parametrize("name,I,J,K,frac,env,which,why", FALLBACK_CASES, ids=[f[0] for f in FALLBACK_CASES])
def test_no_tables_where_a_direction_cannot_hand_over(monkeypatch, name, I, J, K, frac, env, which, why):
    """A unit left to the generic kernel, or a direction whose block shape is not 8 or 16 waves: BNMTF_HANDOVER=1 builds nothing,
    bnmtf_handover_dump says so, and the run follows the oracle through its pre-pass."""
    case = Case(name, "gibbs", I, J, K, ("uniform", frac, 0), env, None, None, "")
    case.setenv(monkeypatch)
    R, M, U0, V0, pri = case.data(0.0)
    b = bnmf_gibbs_optimised(R, M, K, pri, verbose=False, seed=5)
    d = b.describe()
    assert "handover=0" in d, d
    assert (int(re.findall(r"generic_units=(\d+)", d)[which]) > 0) == (why == "gen_units"), d
    info = np.zeros(H.DUMP_INFO_LEN, dtype=np.int64)
    for w in (0, 1):
        assert H.raw_dump(b._handle(), w, info, [None] * 5) == BNMTF_ESTATE
    assert "no hand-over tables" in _lib.lib().bnmtf_last_error().decode()
    b.U, b.V, b.tau = U0.copy(), V0.copy(), 1.0
    b.run(2, update="mode")
    Us, Vs, taus = H.gibbs_mode_chain(R, M, U0, V0, 1.0, pri, 2)
    dev = (_row_scaled(np.array(b.all_U), np.array(Us[1:])), _row_scaled(np.array(b.all_V), np.array(Vs[1:])),
           float(np.max(np.abs(np.asarray(b.all_tau) / np.asarray(taus) - 1.0))))
    print("HO-DEVIATION %s (no hand-over): %.2e %.2e %.2e" % ((name,) + dev))
    assert max(dev) <= H.READER_TOL, dev
