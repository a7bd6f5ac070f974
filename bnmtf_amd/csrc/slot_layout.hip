// The slot layout of the on-chip sweeps (slot_layout.h): from every unit's missing inner indices to the tables the sweep
// kernels gather through, and the choice of the sweep's block shape.  Host code only: nothing here calls the HIP runtime.
#include <cstring>

#include "kernels.h"
#include "slot_layout.h"

namespace bnmtf {

LayoutSwitches LayoutSwitches::from_env() {
  LayoutSwitches s;
  auto num = [](const char* name) -> std::optional<int> {
    const char* e = getenv(name);
    return e ? std::optional<int>(atoi(e)) : std::nullopt;
  };
  s.wide = num("BNMTF_WIDE");
  s.fast_nw = num("BNMTF_FAST_NW");
  s.unit = num("BNMTF_UNIT");
  s.unit_nw = num("BNMTF_UNIT_NW");
  s.no_chunks = getenv("BNMTF_NO_CHUNKS") != nullptr;
  if (const char* e = getenv("BNMTF_VB_PATH")) s.vb_path = !strcmp(e, "masked") ? 1 : !strcmp(e, "pairs") ? 2 : 0;
#ifdef BNMTF_EXPERIMENTS       // (A/B switches of decisions that are made: make EXPERIMENTS=1)
  s.balance = num("BNMTF_BALANCE").value_or(1) != 0;
  s.turns = num("BNMTF_TURNS");
  s.twin = num("BNMTF_TWIN");
#endif
  return s;
}

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // an empty slot of a lane list
using LaneList = std::vector<uint32_t>;      // one lane's slot contents, in slot order

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// fast layout: a unit owns a 32-lane half wave.  Lane r prefers the entries with j mod 32 == r (bank-conflict-free
// LDS gathers).  Residue classes are binomially unbalanced, so instead of padding every lane to the fullest class
// a unit gets E = ceil(cnt / 32) slots per lane (rounded up to even) and the entries of over-full classes are
// parked in lanes with room.  A parked entry shares its row's LDS read with the entry of its own residue lane (a
// 2-way bank conflict: one extra LDS cycle for that row); parked entries are packed into the last rows, distinct
// residues per row, so that few rows pay it.  BNMTF_BALANCE=0 restores the padded conflict-free layout.
//
// E slots per lane for the 32 lane lists of one half wave (L[r]: the entries of residue class r, `cnt` in all), balanced:
// E = ceil(cnt / 32) rounded up to even, the entries of over-full classes parked in lanes with room (see above).  over: scratch
int balance_lanes(LaneList* L, size_t cnt, bool balance, std::vector<LaneList>& over) {
  int emax = 0;
  for (int r = 0; r < 32; ++r) emax = std::max(emax, (int)L[r].size());
  int E = std::max(2, (emax + 1) & ~1);
  const int Eb = std::max(2, ((int)((cnt + 31) / 32) + 1) & ~1);
  if (balance && Eb < E) {
    E = Eb;
    size_t nover = 0;
    for (int r = 0; r < 32; ++r) {
      over[r].clear();
      while ((int)L[r].size() > E) { over[r].push_back(L[r].back()); L[r].pop_back(); ++nover; }
    }
    std::vector<int> own(32);
    for (int r = 0; r < 32; ++r) { own[r] = (int)L[r].size(); L[r].resize(E, kNone); }
    // last rows first; in a row every free lane takes a parked entry of a residue not yet parked in that row
    int rr = 0;
    for (int row = E - 1; row >= 0 && nover > 0; --row) {
      uint32_t used = 0;
      for (int lane = 0; lane < 32 && nover > 0; ++lane) {
        if (own[lane] > row) continue;
        int pick = -1;
        for (int t = 0; t < 32; ++t) { const int r = (rr + t) & 31; if (!over[r].empty() && !((used >> r) & 1u)) { pick = r; break; } }
        if (pick < 0) break;
        L[lane][row] = over[pick].back(); over[pick].pop_back(); --nover;
        used |= 1u << pick; rr = (pick + 1) & 31;
      }
    }
    for (int row = E - 1; row >= 0 && nover > 0; --row)      // leftovers (same residue twice in a row): any free slot
      for (int lane = 0; lane < 32 && nover > 0; ++lane) {
        if (L[lane][row] != kNone) continue;
        for (int r = 0; r < 32; ++r) if (!over[r].empty()) { L[lane][row] = over[r].back(); over[r].pop_back(); --nover; break; }
      }
  }
  return E;
}

// Rows [row0, row0 + nrows) of a [.][64] slot table, lanes [lane0, lane0 + 32): slot s of the lane list L[r], and where the list
// has ended or the slot is empty -- L null: no unit at all -- the sentinel sent0 + r (a zero word behind the panel)
void fill_half_rows(uint32_t* table, size_t row0, uint32_t nrows, int lane0, const LaneList* L, uint32_t sent0) {
  for (uint32_t s = 0; s < nrows; ++s)
    for (int r = 0; r < 32; ++r) {
      uint32_t v = sent0 + (uint32_t)r;
      if (L && s < L[r].size() && L[r][s] != kNone) v = L[r][s];
      table[(row0 + s) * 64 + lane0 + r] = v;
    }
}

// 16-bit packed slot pairs (two inner indices per word): the slot table the on-chip kernels load
void pack_off16(const std::vector<uint32_t>& off, size_t rows, std::vector<uint32_t>& off16) {
  parallel_chunks((int)(rows / 2), 4096, [&](int ra, int rb) {
    for (size_t r2 = (size_t)ra; r2 < (size_t)rb; ++r2)
      for (int l = 0; l < 64; ++l) off16[r2 * 64 + l] = (off[(2 * r2) * 64 + l] & 0xFFFFu) | (off[(2 * r2 + 1) * 64 + l] << 16);
  });
}

// The pair layout's lane lists -- per unit, per chunk, per lane: slot contents, chunk-local inner indices -- and every unit's
// slot rows Eu (two chunks: each gets half of them)
void fill_pair_lanes(const SlotLayoutInput& in, const SlotLayout& g, std::vector<LaneList>& lanes, std::vector<int>& Eu) {
  const int nch = g.nch;
  parallel_chunks(in.n, 64, [&](int ua, int ub) {
    std::vector<LaneList> over(32);
    for (int ul = ua; ul < ub; ++ul) {
      const MissingView& mv = in.miss[ul];
      int ehalf = 0;
      for (int ch = 0; ch < nch; ++ch) {
        LaneList* L = &lanes[((size_t)ul * nch + ch) * 32];
        const uint32_t lo = ch == 0 ? 0u : (uint32_t)g.mh, hi = (nch == 2 && ch == 0) ? (uint32_t)g.mh : 0xFFFFFFFFu;
        size_t cnt = 0;
        {   // one allocation per lane instead of a doubling chain (32 lanes x 8192 units: the layout pass was mostly malloc)
          const size_t guess = (size_t)mv.count / (32 * (size_t)nch) + 8;
          for (int r = 0; r < 32; ++r) L[r].reserve(guess);
        }
        for (const uint32_t* pj = mv.idx; pj != mv.idx + mv.count; ++pj) { const uint32_t j = *pj; if (j >= lo && j < hi) { L[(j - lo) & 31].push_back(j - lo); ++cnt; } }
        ehalf = std::max(ehalf, balance_lanes(L, cnt, in.sw.balance, over));
      }
      Eu[ul] = nch * ehalf;                  // two chunks: each gets half of the unit's slot rows (a multiple of 4 in all)
    }
  });
}

// Where the pair of descending rank pi sits.  The 2/4/8-wave blocks take the pairs in that order.  The on-chip kernel picks the
// slot class per WAVE, so for the 16-wave shape the pairs are dealt to the blocks boustrophedon (and to the four SIMDs of a
// block likewise): every block, and every SIMD, gets the same mix of full and light units, and one round of blocks ends together.
int slot_of(int pi, bool use_wide, int wide_blocks) {
  if (!use_wide) return pi;
  const int r = pi / wide_blocks, c = pi % wide_blocks;
  const int blk = (r & 1) ? wide_blocks - 1 - c : c;
  // rank 0 = the pairs with the most slots.  The lightest quarter goes to waves 0-3, the waves of the sampler window (sampler
  // and table filler: sweep_chip.inc, RL) -- their role needs registers the heaviest slot class does not have, and a light
  // wave reaches the column's first barrier early, with the word-only half of its candidate done by the time the others arrive
  const int t = r >> 2, sx = r & 3;
  return blk * 16 + 4 * (3 - t) + ((t & 1) ? 3 - sx : sx);
}

// Units pair up in descending slot-count order (`order`); the pairs' places, slot rows and first rows
void order_pairs(const SlotLayoutInput& in, const std::vector<int>& order, const std::vector<int>& Eu, int wide_blocks, SlotLayout& out) {
  const int npairs_real = (in.n + 1) / 2;
  out.npairs = out.use_wide ? wide_blocks * 16 : npairs_real;
  out.unit_map.assign((size_t)out.npairs * 2, -1);
  out.pair_E.assign(out.npairs, 0u);
  out.pair_base.assign(out.npairs, 0u);
  out.emax = 0;
  for (int pi = 0; pi < npairs_real; ++pi) {
    int e = 0;
    const int sl = slot_of(pi, out.use_wide, wide_blocks);
    for (int hh = 0; hh < 2; ++hh) {
      const int pos = 2 * pi + hh;
      if (pos < in.n) { out.unit_map[2 * sl + hh] = order[pos]; e = std::max(e, Eu[order[pos]]); }
    }
    out.pair_E[sl] = (uint32_t)e;
    out.emax = std::max(out.emax, e);
  }
  size_t rows_total = 0;
  for (int sl = 0; sl < out.npairs; ++sl) { out.pair_base[sl] = (uint32_t)rows_total; rows_total += out.pair_E[sl]; }
  out.slots = rows_total;
}

// The pair layout's slot table from the lane lists
void fill_pair_table(const std::vector<LaneList>& lanes, SlotLayout& out) {
  const int nch = out.nch;
  out.off.resize(std::max<size_t>(out.slots, 1) * 64);
  parallel_chunks(out.npairs, 64, [&](int pa, int pb) {
    for (int pi = pa; pi < pb; ++pi)
      for (int hh = 0; hh < 2; ++hh) {
        const int ul = out.unit_map[2 * pi + hh];
        const LaneList* L = ul >= 0 ? &lanes[(size_t)ul * nch * 32] : nullptr;
        const uint32_t E = out.pair_E[pi];
        if (nch == 1) { fill_half_rows(out.off.data(), out.pair_base[pi], E, hh * 32, L, (uint32_t)out.mz); continue; }
        // two chunks: the pair's first E / 2 rows are chunk 0 (zero words behind index mh), the rest chunk 1 (behind mz - mh)
        fill_half_rows(out.off.data(), out.pair_base[pi], E / 2, hh * 32, L, (uint32_t)out.mh);
        fill_half_rows(out.off.data(), (size_t)out.pair_base[pi] + E / 2, E - E / 2, hh * 32, L ? L + 32 : nullptr, (uint32_t)(out.mz - out.mh));
      }
  });
}

// ---- the unit-per-wave layout (kernel_sweep_unit.hip): few units per CU -- a shard of a multi-GPU run, a small
// problem.  A pair's two halves belong to the SAME unit: residue class r of the unit's missing entries is dealt in turn to
// lanes r and r + 32 (each half of a 64-lane LDS read touches 32 distinct banks), each half balanced like a 32-lane unit.
// Pair p = local unit p (no sorting: a block's waves do not share slot work).  Beside the layout above (the variational
// sweeps keep it), a few MB at these sizes.  Leaves `out` without the tables when a unit needs more than kUnitMaxSlots slots.
void build_unit_layout(const SlotLayoutInput& in, SlotLayout& out) {
  const int n = in.n;
  std::vector<LaneList> ul((size_t)n * 64);
  std::vector<uint32_t> uE(n, 0u), uB(n, 0u);
  parallel_chunks(n, 64, [&](int ua, int ub) {
    std::vector<LaneList> over(32);
    for (int u = ua; u < ub; ++u) {
      LaneList* L = &ul[(size_t)u * 64];
      size_t cnt[2] = {0, 0};
      uint8_t turn[32] = {};
      for (const uint32_t* pj = in.miss[u].idx; pj != in.miss[u].idx + in.miss[u].count; ++pj) {
        const int r = (int)(*pj & 31u), hh = turn[r]; turn[r] ^= 1;
        L[hh * 32 + r].push_back(*pj); ++cnt[hh];
      }
      const int e0 = balance_lanes(L, cnt[0], in.sw.balance, over), e1 = balance_lanes(L + 32, cnt[1], in.sw.balance, over);
      uE[u] = (uint32_t)std::max(e0, e1);
    }
  });
  size_t rows = 0; uint32_t emax = 0;
  for (int u = 0; u < n; ++u) { uB[u] = (uint32_t)rows; rows += uE[u]; emax = std::max(emax, uE[u]); }
  if ((int)emax > kUnitMaxSlots) return;
  std::vector<uint32_t> uoff(rows * 64);                 // (every uE is even and at least 2: rows / 2 words, both halves written)
  parallel_chunks(n, 64, [&](int ua, int ub) {
    for (int u = ua; u < ub; ++u)
      for (int hh = 0; hh < 2; ++hh) fill_half_rows(uoff.data(), uB[u], uE[u], hh * 32, &ul[(size_t)u * 64 + hh * 32], (uint32_t)out.mz);
  });
  out.u_off16.assign(rows / 2 * 64, 0);
  pack_off16(uoff, rows, out.u_off16);
  out.u_unit_map.resize((size_t)n * 2);
  for (int u = 0; u < n; ++u) out.u_unit_map[2 * u] = out.u_unit_map[2 * u + 1] = u;
  out.u_pair_E = std::move(uE);
  out.u_pair_base = std::move(uB);
  out.u_nw = n <= 4 * 256 ? 4 : 8;
  if (in.sw.unit_nw) out.u_nw = *in.sw.unit_nw == 8 ? 8 : 4;
  out.u_emax = (int)emax;
  out.uw_ok = true;
  out.stats_blocks = std::max(out.stats_blocks, (n + out.u_nw - 1) / out.u_nw + 2);
}

}  // namespace

void build_slot_layout(const SlotLayoutInput& in, SlotLayout& out, CreateLaps* laps) {
  const LayoutSwitches& sw = in.sw;
  const int n = in.n, m = in.m, KP = in.KP;
  auto lap = [&](const char* what) { if (laps) laps->lap(what); };
  out = SlotLayout();
  out.mz = round_up(m, 32);
  out.pw = round_up(out.mz + 32, 256);
  out.pair_ok = out.mz + 32 < 65536;
  out.vb_path = sw.vb_path;
  // an inner extent that does not fit one LDS panel is cut in two chunks (kernel_sweep_fast.hip: sweep_two_chunks_plan); a
  // unit's entries are then laid out chunk by chunk, with inner indices local to the chunk
  out.pw_chunk = out.pw;
  if (!sweep_fast_supported(KP, out.pw) && !sw.no_chunks && sweep_two_chunks_plan(KP, m, &out.mh, &out.pw_chunk, &out.pw1)) out.nch = 2;
  const int nch = out.nch;

  std::vector<int> Eu(n, 0);
  std::vector<LaneList> lanes((size_t)n * 32 * nch);
  fill_pair_lanes(in, out, lanes, Eu);
  lap("    layout: lanes filled and balanced");

  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return Eu[x] > Eu[y]; });
  // the 16-wave shape: from 192 blocks of 16 pairs, when every pair fits its slot classes (BNMTF_WIDE=0: never, 1: whenever it can run)
  const int emax_all = n > 0 ? Eu[order[0]] : 0;
  const int wide_blocks = ((n + 1) / 2 + 15) / 16;
  out.wide_can = nch == 1 && sweep_wide_supported(KP, out.pw) && emax_all <= kWideMaxSlots && n > 0;
  out.use_wide = out.wide_can && wide_blocks >= 192;
  if (sw.wide) out.use_wide = out.wide_can && *sw.wide != 0;
#ifdef BNMTF_EXPERIMENTS       // (kernel_sweep_turns.hip is part of that build only)
  if (sw.turns) out.use_turns = out.use_wide && sweep_turns_supported(KP, out.pw) && *sw.turns != 0;
#endif
  order_pairs(in, order, Eu, wide_blocks, out);
  fill_pair_table(lanes, out);
  lap("    layout: slot table filled");
  out.off16.assign(std::max<size_t>(out.slots / 2, 1) * 64, 0);
  if (out.pair_ok) pack_off16(out.off, out.slots, out.off16);

  // waves per block: 8 when there are enough units for >= 256 blocks, else 4 or 2 (multi-GPU shards, small problems)
  out.f_nw = out.npairs >= 8 * 256 ? 8 : (out.npairs >= 4 * 256 ? 4 : (out.npairs >= 2 * 64 ? 2 : 8));
  if (sw.fast_nw) out.f_nw = *sw.fast_nw == 2 ? 2 : (*sw.fast_nw == 4 ? 4 : 8);
  if (out.use_wide) out.f_nw = 16;
  // the twin shape (BNMTF_TWIN=1): the 16-wave layout run by 8-wave blocks, two to a CU (sweep_chip.inc, TW = 1)
  if (sw.twin) out.use_twin = out.use_wide && !out.use_turns && in.world == 1 && out.pw <= kTwinPanelStride && *sw.twin != 0;
  if (out.use_twin) out.f_nw = 8;
  if (nch == 2) out.f_nw = 8;                       // the two-chunk variant is an 8-wave kernel
  // pairs with more slots per lane than the block shape holds (kFastMaxSlots; the 16-wave shape is only chosen when
  // every pair fits) are left to the generic kernel: their waves idle in the on-chip kernel
  for (int pi = 0; pi < out.npairs && !out.use_wide; ++pi)
    if ((int)out.pair_E[pi] > kFastMaxSlots)
      for (int t = 2 * pi; t < 2 * pi + 2; ++t) if (out.unit_map[t] >= 0) out.gen_units.push_back(out.unit_map[t]);
  out.stats_blocks = std::max((out.npairs + out.f_nw - 1) / out.f_nw, sweep_vb_blocks(out.npairs)) + 2;   // the VB sweep writes its own block count of rows
  // the block of every slot row: what build_handover needs beside the layout itself (one GPU, the 16-wave shape or the
  // plain 8-wave shape, every unit on the on-chip kernel)
  if (in.world == 1 && !out.use_turns && out.pair_ok && out.gen_units.empty() && nch == 1 && (out.f_nw == 16 || out.f_nw == 8) && out.npairs / out.f_nw < 65535) {
    out.ho_ppb = out.f_nw;
    out.row_blk.assign(std::max<size_t>(out.slots, 1), 0);
    for (int pi = 0; pi < out.npairs; ++pi)
      for (uint32_t sidx = 0; sidx < out.pair_E[pi]; ++sidx) out.row_blk[out.pair_base[pi] + sidx] = (uint16_t)(pi / out.ho_ppb);
  }

  // (a test that forces another block shape -- BNMTF_WIDE, BNMTF_FAST_NW -- gets that shape; BNMTF_UNIT=0 switches this one off)
  if (n > 0 && n <= kUnitMaxUnits && nch == 1 && out.pair_ok && sweep_unit_supported(KP, out.pw) && !sw.wide && !sw.fast_nw && !(sw.unit && *sw.unit == 0)) {
    build_unit_layout(in, out);
    lap("    layout: unit-per-wave tables");
  }
}

}  // namespace bnmtf
