"""The slot layout of the on-chip sweeps (csrc/slot_layout.hip), through the library's host-only entry bnmtf_slot_layout: the
tables bnmtf_create uploads for one direction and the block shape it chooses, from seeded masks.  The statements below are what
the sweep kernels assume of the tables (sweep_chip.inc, kernel_sweep_unit.hip, kernel_handover.hip) -- they do not rebuild them.
No GPU needed."""
import os
import re

import numpy as np
import pytest

from _slot_layout import INFO, TABLES, raw_call, missing_lists, random_missing, slot_layout

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bnmtf_amd", "csrc")


def _const(name, fname="kernels.h"):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read()).group(1))


K_FAST_MAX_SLOTS, K_WIDE_MAX_SLOTS = _const("kFastMaxSlots"), _const("kWideMaxSlots")
K_UNIT_MAX_UNITS, K_UNIT_MAX_SLOTS = _const("kUnitMaxUnits"), _const("kUnitMaxSlots")
K_CHIP_PANEL = _const("kChipPanelStride", "sweep_chip.inc")
SWITCHES = ("BNMTF_WIDE", "BNMTF_FAST_NW", "BNMTF_UNIT", "BNMTF_UNIT_NW", "BNMTF_NO_CHUNKS", "BNMTF_VB_PATH", "BNMTF_BALANCE",
            "BNMTF_TURNS", "BNMTF_TWIN", "BNMTF_HOST_THREADS")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _slots_of(cnt):
    """E of a 32-lane unit of cnt missing entries: max(2, even_up(ceil(cnt / 32)))"""
    e = -(-np.asarray(cnt) // 32)
    return np.maximum(2, e + (e & 1))


def _lists(miss):
    return [np.nonzero(row)[0].astype(np.uint32) for row in miss]


def _parked_expected(classes, E):
    return sum(max(0, len(c) - E) for c in classes)


def _check_common(L, miss):
    """What holds of every pair layout: the unit map, the prefix sums, the packed table, the block of every slot row."""
    n = miss.shape[0]
    um = L.unit_map.reshape(-1, 2)
    assert L.sizes["unit_map"] == 2 * L.npairs and L.sizes["pair_E"] == L.npairs == L.sizes["pair_base"]
    assert sorted(um[um >= 0].tolist()) == list(range(n)) and (um >= -1).all()
    assert (L.pair_E[(um < 0).all(axis=1)] == 0).all()
    assert (L.pair_base == np.concatenate([[0], np.cumsum(L.pair_E)[:-1]])).all() and L.slots == int(L.pair_E.sum())
    assert L.emax == int(L.pair_E.max())
    assert L.off.shape == (max(L.slots, 1), 64) and L.off16.shape == (max(L.slots // 2, 1), 64)
    assert L.pair_ok == (L.mz + 32 < 65536) and L.mz == -(-L.m // 32) * 32 and L.pw == -(-(L.mz + 32) // 256) * 256
    if L.pair_ok and L.slots:
        assert (L.off16[:L.slots // 2] == (L.off[0:L.slots:2] | (L.off[1:L.slots:2] << 16))).all()
    if L.ho_ppb > 0:
        assert L.ho_ppb == L.f_nw and L.sizes["row_blk"] == max(L.slots, 1)
        assert (L.row_blk[:L.slots] == np.repeat(np.arange(L.npairs) // L.ho_ppb, L.pair_E)).all()
    else:
        assert L.sizes["row_blk"] == 0
    return um


def _check_pairs_one_chunk(L, miss):
    assert L.nch == 1 and L.pw_chunk == L.pw
    um = _check_common(L, miss)
    lists = _lists(miss)
    E_unit = _slots_of(miss.sum(axis=1))
    sent = (L.mz + np.arange(32)).astype(np.uint32)
    for p in range(L.npairs):
        E, base = int(L.pair_E[p]), int(L.pair_base[p])
        assert E == max([int(E_unit[u]) for u in um[p] if u >= 0], default=0)
        for hh in range(2):
            blk = L.off[base:base + E, hh * 32:hh * 32 + 32]
            real = blk != sent[None, :]
            u = um[p, hh]
            if u < 0:
                assert not real.any()
                continue
            vals = blk[real]
            assert (np.sort(vals) == lists[u]).all() and len(vals) == len(lists[u])
            lane = np.nonzero(real)[1]
            classes = [lists[u][lists[u] % 32 == r] for r in range(32)]
            assert int(((vals & 31) != lane).sum()) == _parked_expected(classes, int(E_unit[u]))     # balancing parks only what overflows


def _check_unit_tables(L, miss):
    n = miss.shape[0]
    assert L.uw_ok == 1 and (L.u_unit_map == np.repeat(np.arange(n), 2)).all()
    rows = np.empty((2 * L.u_off16.shape[0], 64), dtype=np.uint32)
    rows[0::2] = L.u_off16 & 0xFFFF; rows[1::2] = L.u_off16 >> 16
    assert (L.u_pair_base == np.concatenate([[0], np.cumsum(L.u_pair_E)[:-1]])).all() and rows.shape[0] == int(L.u_pair_E.sum())
    assert L.u_emax == int(L.u_pair_E.max()) <= K_UNIT_MAX_SLOTS
    sent = (L.mz + (np.arange(64) & 31)).astype(np.uint32)
    for u, lst in enumerate(_lists(miss)):
        blk = rows[int(L.u_pair_base[u]):int(L.u_pair_base[u]) + int(L.u_pair_E[u])]
        real = blk != sent[None, :]
        assert (np.sort(blk[real]) == lst).all() and real.sum() == len(lst)
        E_half = []
        for hh in range(2):
            half, hreal = blk[:, hh * 32:hh * 32 + 32], real[:, hh * 32:hh * 32 + 32]
            vals, lane = half[hreal], np.nonzero(hreal)[1]
            # the alternating deal: residue class r goes in turn to lanes r and r + 32
            classes = [lst[lst % 32 == r][hh::2] for r in range(32)]
            assert all((np.sort(vals[vals % 32 == r]) == classes[r]).all() for r in range(32))
            E_half.append(int(_slots_of(len(vals))))
            assert int(((vals & 31) != lane).sum()) == _parked_expected(classes, E_half[-1])       # own residue, or parked
        assert int(L.u_pair_E[u]) == max(E_half)


def _no_unit_tables(L):
    assert L.uw_ok == 0 and L.u_emax == 0
    assert all(L.sizes[t] == 0 for t in ("u_unit_map", "u_pair_E", "u_pair_base", "u_off16"))


EDGES = [(1, 33, 0.5), (1, 40, 0.0), (7, 33, 0.4), (5, 100, 0.6), (33, 130, 0.5), (64, 1000, 0.3), (192, 130, 0.5), (150, 77, 0.05)]


@pytest.mark.parametrize("n,m,frac", EDGES)
def test_pair_and_unit_tables_hold_every_missing_entry_once(n, m, frac):
    """One chunk, no switches: a single unit, odd unit counts, m = 33 and other extents that are no multiple of 32, a unit
    without a missing entry (two rows of sentinels)."""
    rs = np.random.RandomState(1000 * n + m)
    miss = random_missing(rs, n, m, frac)
    miss[n // 2] = False
    L = slot_layout(miss)
    _check_pairs_one_chunk(L, miss)
    assert L.npairs == (n + 1) // 2 and (np.diff(L.pair_E.astype(int)) <= 0).all()           # descending slot counts
    assert L.sizes["gen_units"] == 0 and L.use_wide == 0 and L.vb_path == 0
    assert L.stats_blocks >= -(-L.npairs // L.f_nw) + 2
    _check_unit_tables(L, miss)
    um = L.unit_map.reshape(-1, 2)
    p_empty = int(np.nonzero(um == n // 2)[0][0])
    hh = int(np.nonzero(um[p_empty] == n // 2)[0][0])
    assert (L.off[int(L.pair_base[p_empty]):int(L.pair_base[p_empty]) + 2, hh * 32:hh * 32 + 32] == L.mz + np.arange(32)).all()


def _wide_slot(pi, wide_blocks):
    """slot_layout.hip, slot_of: descending rank pi -> the pair's place.  Ranks are dealt to the blocks boustrophedon, round r of
    wide_blocks ranks going to wave 4 (3 - r // 4) + (r % 4, reversed in odd groups of four rounds) of every block: the lightest
    quarter on waves 0-3."""
    r, c = divmod(pi, wide_blocks)
    blk = wide_blocks - 1 - c if r & 1 else c
    t, sx = r >> 2, r & 3
    return blk * 16 + 4 * (3 - t) + (3 - sx if t & 1 else sx)


@pytest.mark.parametrize("n,m", [(70, 200), (33, 77), (515, 130)])
def test_wide_shape_deals_the_descending_pairs_to_the_blocks(monkeypatch, n, m):
    monkeypatch.setenv("BNMTF_WIDE", "1")
    rs = np.random.RandomState(n)
    miss = rs.uniform(size=(n, m)) < rs.uniform(0.0, 0.9, size=n)[:, None]
    L = slot_layout(miss)
    _check_pairs_one_chunk(L, miss)
    assert L.wide_can == 1 and L.use_wide == 1 and L.f_nw == 16 and L.npairs % 16 == 0 and L.sizes["gen_units"] == 0
    wide_blocks = L.npairs // 16
    assert wide_blocks == -(-((n + 1) // 2) // 16)
    E_desc = np.sort(_slots_of(miss.sum(axis=1)))[::-1]
    place = np.array([_wide_slot(pi, wide_blocks) for pi in range((n + 1) // 2)])
    assert len(set(place.tolist())) == len(place) and place.max() < L.npairs
    assert (L.pair_E[place] == E_desc[0::2]).all()               # a pair's slot rows: its fuller unit's, the first of the two ranks
    assert L.pair_E.sum() == E_desc[0::2].sum()                   # (the places no rank reaches are padding)
    _no_unit_tables(L)                                            # BNMTF_WIDE is present


def test_two_chunks_keep_chunk_local_indices(monkeypatch):
    m = K_CHIP_PANEL - 32 + 1                  # the first inner extent whose panel (round_up(mz + 32, 256) floats) does not fit one buffer
    n = 5
    rs = np.random.RandomState(5)
    miss = random_missing(rs, n, m, 0.05)
    miss[3] = False
    L = slot_layout(miss)
    assert L.nch == 2 and L.f_nw == 8 and L.mh % 256 == 0 and 0 < L.mh < m and L.pw_chunk <= K_CHIP_PANEL and L.pw1 <= L.pw_chunk
    assert L.use_wide == 0 and L.wide_can == 0 and L.ho_ppb == 0
    um = _check_common(L, miss)
    _no_unit_tables(L)
    lists = _lists(miss)
    cnt0 = np.array([(l < L.mh).sum() for l in lists]); cnt1 = miss.sum(axis=1) - cnt0
    E_unit = 2 * np.maximum(_slots_of(cnt0), _slots_of(cnt1))
    for p in range(L.npairs):
        E, base = int(L.pair_E[p]), int(L.pair_base[p])
        assert E == max(int(E_unit[u]) for u in um[p] if u >= 0) and E % 4 == 0
        for hh in range(2):
            u = um[p, hh]
            found = []
            for ch, (r0, r1, s0, lo) in enumerate(((0, E // 2, L.mh, 0), (E // 2, E, L.mz - L.mh, L.mh))):
                blk = L.off[base + r0:base + r1, hh * 32:hh * 32 + 32]
                real = blk != (s0 + np.arange(32))[None, :]
                assert (blk[real] < s0).all()                                    # chunk-local
                found.append(blk[real].astype(np.int64) + lo)
            got = np.sort(np.concatenate(found))
            assert (got == (lists[u] if u >= 0 else [])).all() and len(got) == (len(lists[u]) if u >= 0 else 0)
            if u >= 0:
                assert (found[0] < L.mh).all() and (found[1] >= L.mh).all()
    monkeypatch.setenv("BNMTF_NO_CHUNKS", "1")
    assert slot_layout(miss).nch == 1


def test_a_unit_beyond_the_block_shape_goes_to_the_generic_kernel_with_its_partner():
    m, n = K_FAST_MAX_SLOTS * 32 + 300, 6
    rs = np.random.RandomState(11)
    miss = random_missing(rs, n, m, 0.1)
    miss[3] = True; miss[3, :200] = False                      # more than kFastMaxSlots * 32 missing entries
    assert miss[3].sum() > K_FAST_MAX_SLOTS * 32
    L = slot_layout(miss)
    _check_pairs_one_chunk(L, miss)
    um = L.unit_map.reshape(-1, 2)
    p = int(np.nonzero(um == 3)[0][0])
    assert L.use_wide == 0 and L.wide_can == 0 and L.emax > K_FAST_MAX_SLOTS
    assert sorted(L.gen_units.tolist()) == sorted(um[p].tolist()) and len(L.gen_units) == 2
    assert L.ho_ppb == 0
    _check_unit_tables(L, miss)                                 # (dealt to both halves of a wave the unit fits kUnitMaxSlots)


def test_unit_tables_are_absent_beyond_their_limits_and_under_the_switches(monkeypatch):
    rs = np.random.RandomState(3)
    sparse = random_missing(rs, K_UNIT_MAX_UNITS + 1, 40, 0.1)
    _no_unit_tables(slot_layout(sparse))
    _check_unit_tables(slot_layout(sparse[:K_UNIT_MAX_UNITS]), sparse[:K_UNIT_MAX_UNITS])
    m = 64 * K_UNIT_MAX_SLOTS + 200
    full = random_missing(rs, 4, m, 0.1)
    full[1, :64 * K_UNIT_MAX_SLOTS + 2] = True                  # one lane list more than kUnitMaxSlots rows hold
    _no_unit_tables(slot_layout(full))
    miss = random_missing(rs, 40, 130, 0.5)
    for name, value in (("BNMTF_WIDE", "0"), ("BNMTF_WIDE", "1"), ("BNMTF_FAST_NW", "8"), ("BNMTF_FAST_NW", "2"), ("BNMTF_UNIT", "0")):
        monkeypatch.setenv(name, value)
        L = slot_layout(miss)
        _no_unit_tables(L)
        _check_pairs_one_chunk(L, miss)
        if name == "BNMTF_FAST_NW":
            assert L.f_nw == int(value)
        monkeypatch.delenv(name)
    monkeypatch.setenv("BNMTF_UNIT", "1")
    monkeypatch.setenv("BNMTF_UNIT_NW", "8")
    L = slot_layout(miss)
    _check_unit_tables(L, miss)
    assert L.u_nw == 8
    monkeypatch.setenv("BNMTF_VB_PATH", "masked")
    assert slot_layout(miss).vb_path == 1
    monkeypatch.setenv("BNMTF_VB_PATH", "pairs")
    assert slot_layout(miss).vb_path == 2


@pytest.mark.parametrize("n,f_nw,use_wide", [(254, 8, 0), (255, 2, 0), (2046, 2, 0), (2047, 4, 0), (4094, 4, 0), (4095, 8, 0),
                                             (2 * 16 * 191, 8, 0), (2 * 16 * 191 + 1, 16, 1)])
def test_shape_policy_without_switches(n, f_nw, use_wide):
    """Waves per block by the pair count: 8 from 8 x 256 pairs, 4 from 4 x 256, 2 from 2 x 64, 8 below; the 16-wave shape exactly
    from 192 blocks of 16 pairs."""
    miss = random_missing(np.random.RandomState(n), n, 40, 0.1)
    L = slot_layout(miss, KP=64)
    _check_common(L, miss)
    assert (L.f_nw, L.use_wide, L.wide_can) == (f_nw, use_wide, 1)
    assert L.npairs == (192 * 16 if use_wide else (n + 1) // 2)
    assert L.ho_ppb == (f_nw if f_nw in (8, 16) else 0)
    assert L.uw_ok == (n <= K_UNIT_MAX_UNITS)
    assert L.stats_blocks == max(-(-L.npairs // f_nw), -(-L.npairs // 8), -(-n // L.u_nw) if L.uw_ok else 0) + 2
    if use_wide:
        E_desc = np.sort(_slots_of(miss.sum(axis=1)))[::-1]
        place = np.array([_wide_slot(pi, 192) for pi in range((n + 1) // 2)])
        assert (L.pair_E[place] == E_desc[0::2]).all()
    else:
        assert (np.diff(L.pair_E.astype(int)) <= 0).all()


@pytest.mark.parametrize("n,u_nw", [(1024, 4), (1025, 8)])
def test_unit_waves_per_block(n, u_nw):
    miss = random_missing(np.random.RandomState(n), n, 40, 0.1)
    L = slot_layout(miss)
    assert (L.uw_ok, L.u_nw) == (1, u_nw)
    assert L.stats_blocks == max(-(-L.npairs // L.f_nw), -(-L.npairs // 8), -(-n // u_nw)) + 2


def test_tables_do_not_depend_on_the_thread_count(monkeypatch):
    miss = random_missing(np.random.RandomState(8), 640, 300, 0.2)
    a = slot_layout(miss)
    monkeypatch.setenv("BNMTF_HOST_THREADS", "1")
    b = slot_layout(miss)
    assert all(getattr(a, k) == getattr(b, k) for k in INFO)
    assert all(getattr(a, t).tobytes() == getattr(b, t).tobytes() for t, _ in TABLES)
    _check_pairs_one_chunk(a, miss)


def test_what_the_entry_refuses():
    from bnmtf_amd import _lib
    ptr, idx = missing_lists(np.array([[1, 0, 1], [0, 0, 1]], dtype=bool))
    info = np.zeros(32, dtype=np.int64)
    none = [None] * len(TABLES)

    def refused(*args):
        with pytest.raises(_lib.BnmtfError) as e:
            _lib.check(raw_call(*args))
        return str(e.value)

    assert raw_call(2, 3, 32, 1, ptr, idx, info, none) == 0
    assert "null argument" in refused(2, 3, 32, 1, None, idx, info, none)
    assert "null argument" in refused(2, 3, 32, 1, ptr, idx, None, none)
    assert "null argument" in refused(2, 3, 32, 1, ptr, None, info, none)
    assert "unsupported shape" in refused(0, 3, 32, 1, ptr, idx, info, none)
    assert "unsupported shape" in refused(2, 3, 48, 1, ptr, idx, info, none)
    assert "unsupported shape" in refused(2, 3, 32, 0, ptr, idx, info, none)
    assert "must ascend and lie below m=2" in refused(2, 2, 32, 1, ptr, idx, info, none)
    assert "must ascend" in refused(2, 3, 32, 1, ptr, idx[::-1].copy(), info, none)
    assert "bad list bounds" in refused(2, 3, 32, 1, np.array([0, 4, 2], dtype=np.uint32), idx, info, none)
