"""Shared by tests/test_handover_cases_cpu.py and tests/test_handover_exact_gpu.py: the q hand-over between the half sweeps
(csrc/kernel_handover.hip, the writer epilogue / reader prologue of sweep_chip.inc and kernel_sweep_vb.hip, ho_send_packets and
ho_issue_region of sweep_common.h) -- a NumPy face of the library's read-only diagnostic entry bnmtf_handover_dump, a NumPy
routing model that follows one entry of the mask from its slot at the writer through the staging area and the packet into the
reader's region, a host restatement of the seven table kernels, and the seeded cases with the launch-shape classes each of them
is there for.

An entry (i, j) of the mask sits in a slot of the rows layout (unit i, inner index j) and in one of the cols layout (unit j, inner
index i).  The position of an entry INSIDE its run is handed out by an LDS atomic on the device, so no table can be compared with
a golden file; what can be stated is the routing invariant: the writer's place of an entry, minus its run's start, plus the
packet's start in the reader's region is the place the reader takes for the same entry."""
import os
import re
from types import SimpleNamespace

import numpy as np

from bnmtf_amd import _lib
from _slot_layout import slot_layout

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bnmtf_amd", "csrc")
# every switch that decides the block shapes or the hand-over: a case sets the ones it names and clears the others
SWITCHES = ("BNMTF_WIDE", "BNMTF_FAST_NW", "BNMTF_UNIT", "BNMTF_UNIT_NW", "BNMTF_NO_CHUNKS", "BNMTF_VB_PATH", "BNMTF_BALANCE",
            "BNMTF_TURNS", "BNMTF_TWIN", "BNMTF_HOST_THREADS", "BNMTF_HANDOVER", "BNMTF_HANDOVER_REFRESH", "BNMTF_SPLIT",
            "BNMTF_VB_GENERIC", "BNMTF_TAIL")
U32 = 2.0 ** -24                # unit roundoff of fp32

# ------------------------------------------------------------------------------------------------ the diagnostic entry
DUMP_INFO = ("blocks", "other_blocks", "lds_floats", "ppb", "filled", "regions_current")
DUMP_ARRAYS = (("t_in", np.uint32), ("t_out", np.uint32), ("pk", np.uint32), ("region_ofs", np.uint32), ("region", np.float32))
DUMP_INFO_LEN = 11              # BNMTF_HANDOVER_INFO_LEN


def raw_dump(h, which, info, arrays):
    return _lib.lib().bnmtf_handover_dump(h, int(which), _lib.ptr(info), *[_lib.ptr(a) for a in arrays])


def handover_dump(h, which):
    """Direction `which` (0 rows, 1 cols) of handle h: the scalars (DUMP_INFO) and the five arrays, t_in / t_out as [.][64] words,
    pk as [blocks][other blocks][3].  Two calls: the sizes, then the data."""
    info = np.zeros(DUMP_INFO_LEN, dtype=np.int64)
    _lib.check(raw_dump(h, which, info, [None] * len(DUMP_ARRAYS)))
    assert len(DUMP_INFO) + len(DUMP_ARRAYS) == DUMP_INFO_LEN
    arrays = [np.zeros(int(s), dtype=dt) for (_, dt), s in zip(DUMP_ARRAYS, info[len(DUMP_INFO):])]
    info2 = np.zeros(DUMP_INFO_LEN, dtype=np.int64)
    _lib.check(raw_dump(h, which, info2, arrays))
    assert (info == info2).all()
    d = SimpleNamespace(**{k: int(v) for k, v in zip(DUMP_INFO, info)}, **{name: a for (name, _), a in zip(DUMP_ARRAYS, arrays)})
    d.t_in = d.t_in.reshape(-1, 64); d.t_out = d.t_out.reshape(-1, 64); d.pk = d.pk.reshape(d.blocks, d.other_blocks, 3)
    return d


# ------------------------------------------------------------------------------------------------ slots and places
def pad4(v):
    return (np.asarray(v) + 3) & ~3


def slots(L):
    """Every slot (row, lane) of a layout: its unit and inner index [slot rows][64], whether it holds an entry, and the block of
    every slot row (blocks of ho_ppb pairs: the unit waves of the sweep kernel's block shape)."""
    assert L.ho_ppb > 0 and len(L.gen_units) == 0
    pair = np.repeat(np.arange(L.npairs), L.pair_E)
    unit = L.unit_map.reshape(-1, 2)[pair][:, np.arange(64) >> 5].astype(np.int64)
    inner = L.off[:L.slots].astype(np.int64)
    return SimpleNamespace(S=L.slots, unit=unit, inner=inner, live=(unit >= 0) & (inner < L.m), blk=pair // L.ho_ppb,
                           nb=-(-L.npairs // L.ho_ppb), lane=np.broadcast_to(np.arange(64), unit.shape))


def places(words, S):
    """The 16-bit places of slots (row, lane), [S][64]: rows 2r and 2r + 1 of a lane share word [r][lane] (low half: row 2r)."""
    w = np.asarray(words).reshape(-1, 64)
    out = np.empty((2 * w.shape[0], 64), dtype=np.int64)
    out[0::2] = w & 0xFFFF; out[1::2] = w >> 16
    assert out.shape[0] >= S
    return out[:S]


def set_place(words, row, lane, value):
    sh = 16 * (row & 1)
    words[row >> 1, lane] = (int(words[row >> 1, lane]) & ~(0xFFFF << sh) & 0xFFFFFFFF) | ((int(value) & 0xFFFF) << sh)


def _pack(pl):
    if pl.shape[0] & 1:
        pl = np.concatenate([pl, np.zeros((1, 64), dtype=pl.dtype)])
    return (pl[0::2] | (pl[1::2] << 16)).astype(np.uint32)


def pairing(LW, LRd, w_is_rows):
    """The entries of the mask in the order of the writer's live slots (row-major): the matrix index (i, j), the writer's block
    and (row, lane), the reader's block and (row, lane) of the same entry.  Fails if the two layouts do not hold the same mask."""
    J = LW.m if w_is_rows else LW.n
    sW, sR = slots(LW), slots(LRd)
    wr, wl = np.nonzero(sW.live)
    rr, rl = np.nonzero(sR.live)
    uW, jW = sW.unit[wr, wl], sW.inner[wr, wl]
    uR, jR = sR.unit[rr, rl], sR.inner[rr, rl]
    i, j = (uW, jW) if w_is_rows else (jW, uW)
    kW = i * J + j
    kR = (jR * J + uR) if w_is_rows else (uR * J + jR)
    order = np.argsort(kR)
    assert len(kW) == len(kR) and len(np.unique(kW)) == len(kW) and (np.sort(kW) == kR[order]).all(), "the two layouts hold different masks"
    at = order[np.searchsorted(kR[order], kW)]
    return SimpleNamespace(i=i, j=j, n=len(kW), sW=sW, sR=sR, wrow=wr, wlane=wl, bw=sW.blk[wr], rrow=rr[at], rlane=rl[at], br=sR.blk[rr[at]],
                           count=np.bincount(sW.blk[wr] * sR.nb + sR.blk[rr[at]], minlength=sW.nb * sR.nb).reshape(sW.nb, sR.nb))


def run_lengths(LR, LC):
    """count[bw][br] of both writer / reader pairs, from the host layouts alone: (rows -> cols, cols -> rows)"""
    return pairing(LR, LC, True).count, pairing(LC, LR, False).count


# ------------------------------------------------------------------------------------------------ the routing model
def check_routing(LW, LRd, DW, DRd, w_is_rows):
    """One writer / reader pair of directions: the writer's layout and dump (t_out, pk), the reader's (t_in, region_ofs).  Asserts
    the routing invariant for every entry and every empty slot, and returns the pairing with, per entry, its rank in its run and
    its index in the reader's regions (`gidx`: where the packet puts it = where the reader takes it from)."""
    P = pairing(LW, LRd, w_is_rows)
    sW, sR = P.sW, P.sR
    assert DW.blocks == sW.nb and DW.other_blocks == sR.nb and DRd.blocks == sR.nb and DRd.other_blocks == sW.nb, "block counts"
    assert DW.ppb == LW.ho_ppb and DRd.ppb == LRd.ho_ppb
    pk = DW.pk.astype(np.int64)
    s, c, g = pk[:, :, 0], pk[:, :, 1], pk[:, :, 2]
    rofs = DRd.region_ofs.astype(np.int64)
    out, tin = places(DW.t_out, sW.S), places(DRd.t_in, sR.S)
    # the packets: multiples of four entries, exactly the run's entries padded, disjoint at both ends, inside the reader's region
    assert (s % 4 == 0).all() and (c % 4 == 0).all() and (g % 4 == 0).all(), "packet starts and lengths are multiples of 4"
    assert (c == pad4(P.count)).all(), "a packet's length is its run's entry count padded to four"
    assert rofs[0] == 0 and (rofs % 256 == 0).all() and (np.diff(rofs) > 0).all(), "region offsets: ascending multiples of 256"
    assert (np.diff(rofs) <= 65536).all() and (np.diff(rofs) <= DRd.lds_floats).all(), "a region fits its 16-bit places and the block's LDS"
    for bw in range(sW.nb):
        o = np.lexsort((c[bw], s[bw]))
        assert (s[bw][o][:-1] + c[bw][o][:-1] <= s[bw][o][1:]).all(), "runs overlap in the staging area of block %d" % bw
    for br in range(sR.nb):
        o = np.lexsort((c[:, br], g[:, br]))
        assert (g[:, br][o][:-1] + c[:, br][o][:-1] <= g[:, br][o][1:]).all(), "runs overlap in region %d" % br
        assert (g[:, br] >= rofs[br]).all() and (g[:, br] + c[:, br] <= rofs[br + 1] - 32).all(), "a run leaves region %d or its 32 zeros no room" % br
    stotal = (s + c).max(axis=1)                                   # the end of the runs in every staging area
    rdata = (g + c).max(axis=0) - rofs[:-1]                        # ... and in every region
    assert (stotal + 32 <= 65536).all() and (stotal + 32 + 256 <= DW.lds_floats).all(), "a staging area fits its 16-bit places and the block's LDS"
    # every entry: a place of its own inside the run (bw, br), and the reader takes the packet's start plus the same rank
    p_out, p_in = out[P.wrow, P.wlane], tin[P.rrow, P.rlane]
    rank = p_out - s[P.bw, P.br]
    assert ((rank >= 0) & (rank < P.count[P.bw, P.br])).all(), "a writer place outside its run"
    assert len(np.unique(P.bw * 65536 + p_out)) == P.n, "two entries share a writer place"
    assert (p_in == g[P.bw, P.br] - rofs[P.br] + rank).all(), "the reader's place is not the packet's start plus the writer's rank"
    # every empty slot: the writer's zero goes to the 32 dump words behind the runs, the reader takes one of the 32 zeros
    er, el = np.nonzero(~sW.live)
    d = out[er, el] - stotal[sW.blk[er]]
    assert ((d >= 0) & (d < 32)).all(), "an empty slot of the writer does not point at the dump words"
    er, el = np.nonzero(~sR.live)
    d = tin[er, el] - rdata[sR.blk[er]]
    assert ((d >= 0) & (d < 32)).all(), "an empty slot of the reader does not point at the zeros"
    P.rank = rank; P.gidx = rofs[P.br] + p_in; P.zeros = rofs[:-1] + rdata
    return P


def host_tables(LR, LC):
    """kernel_handover.hip restated on the host for both writer / reader pairs, with the places inside a run in the order of the
    writer's slots: (rows dump, cols dump) without regions, shaped like handover_dump's."""
    D = [SimpleNamespace(ppb=L.ho_ppb, lds_floats=0, filled=0, regions_current=0) for L in (LR, LC)]
    for w in (0, 1):
        LW, LRd, DW, DRd = (LR, LC, D[0], D[1]) if w == 0 else (LC, LR, D[1], D[0])
        P = pairing(LW, LRd, w == 0)
        sW, sR = P.sW, P.sR
        cp = pad4(P.count)
        sbase = np.cumsum(cp, axis=1) - cp                          # ho_scan_kernel: block bw's runs behind one another ...
        stotal = cp.sum(axis=1)
        rbase = np.cumsum(cp, axis=0) - cp                          # ... and region br's
        rdata = cp.sum(axis=0)
        rsize = (rdata + 32 + 255) & ~255
        rofs = np.concatenate([[0], np.cumsum(rsize)])              # ho_region_starts_kernel
        grp = P.bw * sR.nb + P.br
        o = np.argsort(grp, kind="stable")
        rank = np.empty(P.n, dtype=np.int64)
        rank[o] = np.arange(P.n) - (np.cumsum(P.count.ravel()) - P.count.ravel())[grp[o]]      # ho_destination_kernel, in slot order
        t_out = stotal[sW.blk][:, None] + (sW.lane & 31)            # ho_tables_kernel
        t_out[P.wrow, P.wlane] = sbase[P.bw, P.br] + rank
        t_in = rdata[sR.blk][:, None] + (sR.lane & 31)              # ho_reader_default_kernel
        t_in[P.rrow, P.rlane] = rbase[P.bw, P.br] + rank
        DW.t_out = _pack(t_out); DRd.t_in = _pack(t_in)
        DW.pk = np.stack([sbase, cp, rofs[:-1][None, :] + rbase], axis=2).astype(np.uint32)        # ho_packets_kernel
        DRd.region_ofs = rofs.astype(np.uint32)
        DW.blocks = DRd.other_blocks = sW.nb
        DW.lds_floats = max(DW.lds_floats, int(stotal.max()) + 256 + 32); DRd.lds_floats = max(DRd.lds_floats, int(rsize.max()))
    return D[0], D[1]


# ------------------------------------------------------------------------------------------------ the chain's exact q and its bound
def chain_reference(U_states, V_states, K, KP, region, i, j):
    """q of entries (i, j) as the hand-over carries it after n = len(U_states) - 1 iterations of (rows half sweep, cols half sweep)
    from the set state (U_states[0], V_states[0]), and the forward error bound of the chain of fp32 operations that made it.
    The states are the fp32 values the device holds, as float64.  region "rows" (what the rows sweep reads: written by the last
    cols sweep) holds q of (U_n, V_n) after 2 n half sweeps, region "cols" q of (U_n, V_{n-1}) after 2 n - 1.
    The chain: a KP-term fmaf dot of the set state (the first rows sweep's pre-pass), then per half sweep and column k one
    delta_k = fl(x_new - x_old) and one q = fmaf(delta_k, w_k, q), w the other factor as that half sweep saw it.  Every one of the
    c = KP + 2 K H operations rounds a value whose magnitude is at most S = sum_k |u_k v_k| (set state) + sum |delta_k w_k| (all
    half sweeps), so |q_fp32 - q_exact| <= c 2^-24 S / (1 - c 2^-24): derived, not measured."""
    n = len(U_states) - 1
    U = [np.asarray(x, dtype=np.float64)[i] for x in U_states]
    V = [np.asarray(x, dtype=np.float64)[j] for x in V_states]
    S = np.abs(U[0] * V[0]).sum(axis=1)
    H = 0
    for t in range(1, n + 1):
        S += np.abs((U[t] - U[t - 1]) * V[t - 1]).sum(axis=1); H += 1
        if t < n or region == "rows":
            S += np.abs((V[t] - V[t - 1]) * U[t]).sum(axis=1); H += 1
    q = (U[n] * (V[n] if region == "rows" else V[n - 1])).sum(axis=1)
    c = KP + 2 * K * H
    return q, c * U32 * S / (1.0 - c * U32)


def close_share(q, bound, blk):
    """The share of entries whose nearest other q in the same reader block lies within twice the entry's bound: below it a
    misrouted entry could pass for its neighbour."""
    close = np.zeros(len(q), dtype=bool)
    o = np.lexsort((q, blk))
    qs, bs = q[o], blk[o]
    gap = np.full(len(q) + 1, np.inf)
    same = bs[1:] == bs[:-1]
    gap[1:-1][same] = np.diff(qs)[same]
    close[o] = np.minimum(gap[:-1], gap[1:]) <= 2 * bound[o]
    return float(close.mean()) if len(q) else 0.0


# ------------------------------------------------------------------------------------------------ the cases
def _const(name, fname):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read()).group(1))


K_CHIP_PANEL = _const("kChipPanelStride", "sweep_chip.inc")         # STRIDE of the writer epilogue's two panel buffers


class Case:
    """name; model "gibbs" / "vb"; I x J of rank K; mask = ("uniform", share missing, seed) | ("full",) | ("rowcount", missing per row, seed);
    env: the switches beside BNMTF_HANDOVER=1 and BNMTF_HANDOVER_REFRESH=1000000; nw / blocks: (rows, cols) as describe() and the
    dump must report them; classes: what the case is there for (test_handover_cases_cpu.py asserts them from the host layouts)."""

    def __init__(self, name, model, I, J, K, mask, env, nw, blocks, classes):
        self.name, self.model, self.I, self.J, self.K, self.mask, self.nw, self.blocks = name, model, I, J, K, mask, nw, blocks
        self.env = dict(env, BNMTF_HANDOVER="1", BNMTF_HANDOVER_REFRESH="1000000")
        self.classes = frozenset(classes.split())
        self.KP = 32 if K <= 32 else 64

    def __repr__(self):
        return self.name

    def setenv(self, monkeypatch, **more):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, v in dict(self.env, **more).items():
            monkeypatch.setenv(name, v)

    def missing(self):
        """[I][J] booleans: the missing entries; never a whole row or column"""
        if self.mask[0] == "full":
            return np.zeros((self.I, self.J), dtype=bool)
        rs = np.random.RandomState(self.mask[-1])
        if self.mask[0] == "rowcount":                    # every row misses exactly mask[1] columns: the same slot rows for every unit
            miss = np.zeros((self.I, self.J), dtype=bool)
            for i in range(self.I):
                miss[i, rs.choice(self.J, self.mask[1], replace=False)] = True
            assert not miss.all(axis=0).any()
            return miss
        miss = rs.uniform(size=(self.I, self.J)) < self.mask[1]
        miss[np.arange(self.I), rs.randint(0, self.J, self.I)] = False
        miss[rs.randint(0, self.I, self.J), np.arange(self.J)] = False
        return miss

    def layouts(self):
        """(rows, cols) host layouts of the case's mask under the switches in force (the caller has called setenv)"""
        miss = self.missing()
        return slot_layout(miss, KP=self.KP), slot_layout(np.ascontiguousarray(miss.T), KP=self.KP)

    def data(self, spread):
        """R, M, the set state (U0, V0) as fp32 values, the priors.  Exponential factors times a row / column scale exp(uniform(-spread,
        spread)); the set state is the truth times exp(s N(0, 1)), s = 0.05 with a spread, else 0.3.  spread = SPREAD: q of a reader block's entries ranges over
        many decades, which keeps neighbours in the sorted list further apart than the per-entry bound (the separation condition
        of test_handover_cases_cpu.py; relative noise and a lambda of nothing -- the precision of a mode iteration's tau follows the largest entries -- keep the mode update away from zero rows, whose q would
        tie).  spread = 0: data of one scale with additive noise for the runs against the oracle, the factors 0.5 + exponential(0.5): no
        entry of a factor is so small that an error in one q next to it would go unseen (the sensitivity condition of the CPU file)."""
        rs = np.random.RandomState(1000 + self.I + self.J + self.K)
        I, J, K = self.I, self.J, self.K
        if spread:
            Ut = rs.exponential(1.0, (I, K)) * np.exp(rs.uniform(-spread, spread, (I, 1)))
            Vt = rs.exponential(1.0, (J, K)) * np.exp(rs.uniform(-spread, spread, (J, 1)))
        else:
            Ut, Vt = 0.5 + rs.exponential(0.5, (I, K)), 0.5 + rs.exponential(0.5, (J, K))
        R = Ut @ Vt.T
        R = R * np.abs(1.0 + 0.02 * rs.randn(I, J)) if spread else R + 0.5 * rs.randn(I, J)
        R = R.astype(np.float32).astype(np.float64)          # (what the device holds)
        U0 = (Ut * np.exp((0.05 if spread else 0.3) * rs.randn(I, K))).astype(np.float32).astype(np.float64)
        V0 = (Vt * np.exp((0.05 if spread else 0.3) * rs.randn(J, K))).astype(np.float32).astype(np.float64)
        lam = 1e-30 if spread else 0.1
        return R, (~self.missing()).astype(np.float64), U0, V0, dict(alpha=1.0, beta=1.0, lambdaU=lam, lambdaV=lam)


SPREAD = 8.0


def writer_classes(LW, LRd, count, K, model, vb_path=None):
    """(The ho_lds predicate below is a host restatement of sweep_chip.inc / kernel_sweep_vb.hip: the read-only dump cannot observe
    which branch a block took, so a change of the kernels' condition has to be made here as well -- the constants it uses are
    parsed from the sources, the formula is not.)
    The launch-shape classes one writer direction hits, from the host layouts alone: the packet sender's descriptor passes and
    run lengths (sweep_common.h ho_send_packets: count is [writer blocks][reader blocks]) and the epilogue's offset table (through
    the panel buffers or from global memory: sweep_chip.inc / kernel_sweep_vb.hip ho_lds, per writer block)."""
    nw, nb, nbo = LW.ho_ppb, count.shape[0], count.shape[1]
    out = set()
    if nbo > 16 * nw:
        out.add("pass2_nw%d" % nw)                       # a second pass of the p0 loop
    if (nbo % 16) % 4:
        out.add("phantom_packets")                       # np no multiple of 4: pa / pb >= np
    if nbo > 16 and nbo % 16 == 1:
        out.add("np1_after_full16")
    c = pad4(count)
    for name, hit in (("run0", c == 0), ("run_le128", (c > 0) & (c <= 128)), ("run_le256", (c > 128) & (c <= 256)), ("run_long", c > 256),
                      ("run_long_trips", c > 512)):
        if hit.any():
            out.add(name)
    out |= {"res%d" % r for r in np.unique(count[count > 0] % 4)}
    if count.sum() == 0:
        out.add("empty_regions")
    # slot-pair rows of every block -> pieces of 256 words of its slice of t_out
    rows2 = np.bincount(np.arange(LW.npairs) // nw, weights=LW.pair_E, minlength=nb).astype(np.int64) // 2
    ho_np = (rows2 + 3) // 4
    PW = LW.pw // 256
    if model == "gibbs" or vb_path == "masked":          # sweep_chip.inc (the VB update on the on-chip kernel: MODE = kSweepVB)
        odd = (K - 2) & 1
        na, nbuf = (PW if odd else K_CHIP_PANEL // 256), (K_CHIP_PANEL // 256 if odd else PW)
        lds = (K >= 2) & (ho_np - na <= nbuf)
        if K < 2:
            out.add("lds_off_K1")
        else:
            out.add("lds_K_odd" if odd else "lds_K_even")
            if K == 2:
                out.add("lds_K2")
            if lds.any():
                out.add("lds_on")
            if (lds & (ho_np > na)).any():
                out.add("lds_both_buffers")
            if (~lds).any():
                out.add("lds_nofit")
        if K > 32:
            out.add("NX2")
    else:                                                # kernel_sweep_vb.hip: ho_np <= chunks2
        lds = (K >= 2) & (ho_np <= 2 * PW)
        out.add("vb_lds_on" if lds.any() else "vb_lds_off")
        if K >= 2 and (~lds).any():
            out.add("vb_lds_nofit")
    return out, lds


def case_classes(case, LR, LC):
    """classes of both writers, with the writer named where the issue is one-sided: pass2_nw8 as rows / as cols writer"""
    cr, cc = run_lengths(LR, LC)
    vbp = case.env.get("BNMTF_VB_PATH")
    a, lds_r = writer_classes(LR, LC, cr, case.K, case.model, vbp)
    b, lds_c = writer_classes(LC, LR, cc, case.K, case.model, vbp)
    out = a | b | {x + "_rows" for x in a if x.startswith("pass2")} | {x + "_cols" for x in b if x.startswith("pass2")}
    if case.env.get("BNMTF_SPLIT") == "0":
        out = {x for x in out if not x.startswith("lds_")} | {"lds_off_split0"}
    if case.model == "vb":
        out.add("vb_" + vbp)
    return out, (lds_r, lds_c), (cr, cc)


_W = {"BNMTF_WIDE": "1"}
_RES = "res0 res1 res2 res3"
# Gibbs / ICM (sweep_chip.inc).  Block counts and run lengths come from a search over seeds with bnmtf_slot_layout on the CPU.
GIBBS_CASES = [
    Case("runs_straddle_128", "gibbs", 70, 90, 4, ("uniform", 0.2, 0), _W, (16, 16), (3, 3), "run_le128 run_le256 phantom_packets lds_on lds_K_even " + _RES),
    Case("runs_straddle_256", "gibbs", 513, 389, 8, ("uniform", 0.3, 0), _W, (16, 16), (17, 13), "run_le256 run_long np1_after_full16 phantom_packets " + _RES),
    Case("runs_all_long", "gibbs", 200, 300, 5, ("uniform", 0.4, 0), _W, (16, 16), (7, 10), "run_long lds_K_odd lds_both_buffers"),
    Case("runs_many_trips", "gibbs", 64, 64, 3, ("uniform", 0.6, 0), _W, (16, 16), (2, 2), "run_long_trips lds_K_odd"),
    Case("second_pass_16_waves", "gibbs", 40, 8200, 5, ("uniform", 0.03, 0), _W, (16, 16), (2, 257), "pass2_nw16_rows np1_after_full16"),
    Case("second_pass_8_waves_rows", "gibbs", 40, 4100, 6, ("uniform", 0.1, 0), {}, (8, 8), (3, 257), "pass2_nw8_rows np1_after_full16 lds_on"),
    Case("second_pass_8_waves_cols", "gibbs", 4100, 40, 6, ("uniform", 0.1, 0), {}, (8, 8), (257, 3), "pass2_nw8_cols np1_after_full16 lds_on"),
    Case("empty_runs_sparse", "gibbs", 40, 250, 8, ("uniform", 0.01, 0), {}, (8, 8), (3, 16), "run0 run_le128"),
    Case("empty_runs_residues", "gibbs", 100, 100, 7, ("uniform", 0.02, 0), {}, (8, 8), (7, 7), "run0 run_le128 " + _RES),
    Case("nothing_missing", "gibbs", 100, 100, 3, ("full",), {}, (8, 8), (7, 7), "empty_regions run0"),
    Case("rank_1", "gibbs", 64, 40, 1, ("uniform", 0.3, 0), {}, (8, 8), (4, 3), "lds_off_K1"),
    Case("rank_2", "gibbs", 64, 40, 2, ("uniform", 0.3, 0), {}, (8, 8), (4, 3), "lds_K2 lds_K_even lds_on"),
    Case("rank_3", "gibbs", 64, 40, 3, ("uniform", 0.3, 0), {}, (8, 8), (4, 3), "lds_K_odd lds_on lds_both_buffers"),
    Case("rank_4", "gibbs", 64, 40, 4, ("uniform", 0.3, 0), {}, (8, 8), (4, 3), "lds_K_even lds_on"),
    Case("rank_33", "gibbs", 200, 150, 33, ("uniform", 0.2, 0), _W, (16, 16), (7, 5), "NX2 lds_K_odd lds_on"),
    Case("table_does_not_fit", "gibbs", 62, 6600, 2, ("rowcount", 1000, 0), _W, (16, 16), (2, 207), "lds_nofit lds_on lds_both_buffers lds_K_even lds_K2"),
    Case("per_wave_sampler", "gibbs", 70, 90, 4, ("uniform", 0.2, 0), dict(_W, BNMTF_SPLIT="0"), (16, 16), (3, 3), "lds_off_split0"),
]
# variational (api_models.inc: the pair-panel kernel of kernel_sweep_vb.hip hands q over in its 16-wave shape, the on-chip kernel
# with the masked sums in the 8- and the 16-wave shape)
VB_CASES = [
    Case("vb_pairs", "vb", 70, 90, 4, ("uniform", 0.2, 0), dict(_W, BNMTF_VB_PATH="pairs"), (16, 16), (3, 3), "vb_pairs vb_lds_nofit run_le128 run_le256 phantom_packets"),
    Case("vb_pairs_long_rows", "vb", 40, 500, 6, ("uniform", 0.05, 0), dict(_W, BNMTF_VB_PATH="pairs"), (16, 16), (2, 16), "vb_pairs vb_lds_on vb_lds_nofit"),
    Case("vb_masked_16_waves", "vb", 70, 90, 4, ("uniform", 0.2, 0), dict(_W, BNMTF_VB_PATH="masked"), (16, 16), (3, 3), "vb_masked lds_on lds_K_even run_le256"),
    Case("vb_masked_8_waves", "vb", 150, 77, 3, ("uniform", 0.3, 0), {"BNMTF_VB_PATH": "masked"}, (8, 8), (10, 5), "vb_masked lds_on lds_K_odd lds_both_buffers"),
]
CASES = GIBBS_CASES + VB_CASES
for _c in CASES:
    _c.spread = 3.0 if _c.model == "vb" else (12.0 if _c.name == "table_does_not_fit" else SPREAD)
    # the longest mode chain after which the separation condition is asserted (CPU and GPU files).  table_does_not_fit cannot
    # be smaller -- a block whose offset table does not fit has > 8 (36 + pw / 256) slot rows of 64 lanes: 32 000 entries in one
    # reader block -- and with the bound of the three-iteration chain (c = 32 + 24) 1.3 % of them have a neighbour within
    # twice the bound at any spread whose squares fp32 still holds: asserted after one iteration there, printed after three
    _c.sep_chain = 1 if _c.model == "vb" or _c.name == "table_does_not_fit" else 3
# every class of the code's branches (the issue's list), to be hit by at least one Gibbs case ...
GIBBS_REQUIRED = frozenset(("pass2_nw16_rows pass2_nw8_rows pass2_nw8_cols phantom_packets np1_after_full16 run0 run_le128 run_le256 run_long "
                            "run_long_trips res0 res1 res2 res3 lds_off_K1 lds_K2 lds_K_odd lds_K_even lds_on lds_both_buffers lds_nofit "
                            "lds_off_split0 NX2 empty_regions").split())
# ... and, where it applies to the variational sweeps, by one of theirs
VB_REQUIRED = frozenset("vb_pairs vb_masked vb_lds_on vb_lds_nofit lds_on lds_K_odd lds_K_even run_le128 run_le256 phantom_packets".split())

# where the tables must NOT be built: (name, I, J, K, share missing, switches, the direction without blocks, why)
FALLBACK_CASES = [
    ("generic_units", 40, 4100, 3, 0.5, {}, 0, "gen_units"),          # rows of ~2050 missing entries: more slot rows than the on-chip kernel takes
    ("edge_160x1500", 160, 1500, 5, 0.9, {}, 1, "f_nw"),              # tests/test_edge_cases_gpu.py's shape: 750 pairs of columns run 2-wave blocks
    ("two_wave_columns", 200, 300, 4, 0.4, {}, 1, "f_nw"),            # 150 pairs of columns: 2-wave blocks
]


# ------------------------------------------------------------------------------------------------ fp64 chains on the host
def gibbs_mode_chain(R, M, U0, V0, tau0, pri, n):
    """n mode iterations in the residual form (tests/_residual_form.py) from the set state: ([U_0..U_n], [V_0..V_n], [tau_1..tau_n])"""
    from _residual_form import mode_sweep
    U, V, tau = U0.copy(), V0.copy(), float(tau0)
    Mt = np.ascontiguousarray(M.T)
    E = M * (R - U @ V.T)
    Us, Vs, taus = [U0.copy()], [V0.copy()], []
    for _ in range(n):
        mode_sweep(E, U, V, M, tau, pri["lambdaU"])
        Et = np.ascontiguousarray(E.T)
        mode_sweep(Et, V, U, Mt, tau, pri["lambdaV"])
        E = np.ascontiguousarray(Et.T)
        tau = (pri["alpha"] + 0.5 * M.sum()) / (pri["beta"] + 0.5 * (E ** 2).sum())
        Us.append(U.copy()); Vs.append(V.copy()); taus.append(tau)
    return Us, Vs, taus


def vb_set_state(b, U0, V0, exptau):
    """q(U), q(V) with means near (U0, V0): mu = the set state, precision 4 / mu^2 (a standard deviation of half the mean)"""
    from oracle import bnmtf_oracle as O
    b.muU, b.muV = U0.copy(), V0.copy()
    b.tauU, b.tauV = 4.0 / np.maximum(U0, 1e-3) ** 2, 4.0 / np.maximum(V0, 1e-3) ** 2
    b.expU, b.varU = O.tn_expectation(b.muU, b.tauU), O.tn_variance(b.muU, b.tauU)
    b.expV, b.varV = O.tn_expectation(b.muV, b.tauV), O.tn_variance(b.muV, b.tauV)
    b.exptau = exptau


# the reader side's tolerance (tests/test_handover_exact_gpu.py): 8 x the largest deviation of the pre-pass run (BNMTF_HANDOVER=0)
# from the fp64 oracle over all cases, per element of U, V and tau scaled by the row's largest value -- measured on an MI355X
READER_TOL = 8 * 9.88e-6
