// The slot layout of the on-chip sweeps (slot_layout.hip): host arithmetic on every unit's missing inner indices -- no device
// call, no Dir.  build_dir (api.hip) runs it on the lists it downloads and uploads the tables; bnmtf_slot_layout hands the same
// tables to a caller without a GPU (tests/test_slot_layout_cpu.py).  Also the host helpers the layout passes share with api.hip.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <system_error>
#include <thread>
#include <vector>

namespace bnmtf {

// Host threads for the O(I*J) layout passes of bnmtf_create (a cross-validation driver pays them once per model):
// fn(begin, end) over fixed-size chunks of [0, n), so results never depend on the thread count.
template <typename Fn>
void parallel_chunks(int n, int chunk, Fn fn) {
  const int nchunks = (n + chunk - 1) / chunk;
  int nt = (int)std::thread::hardware_concurrency();
  if (const char* e = getenv("BNMTF_HOST_THREADS")) nt = atoi(e);
  nt = std::max(1, std::min({nt, 32, nchunks}));
  if ((size_t)n * (size_t)chunk < 4096) nt = 1;           // (a few thousand rows: starting the threads costs more than the pass)
  std::atomic<int> next{0};
  auto work = [&]() {
    for (int c = next.fetch_add(1); c < nchunks; c = next.fetch_add(1)) fn(c * chunk, std::min(n, (c + 1) * chunk));
  };
  if (nt == 1) { work(); return; }
  // nt - 1 helpers and the calling thread.  A thread that cannot be had (EAGAIN: the user's process / thread limit -- a long test
  // session with worker pools, three ranks building their layouts at once) must not leave this function as an exception: it
  // would cross the C ABI and end the process (std::terminate).  The chunks are claimed one by one, so whoever is there does them.
  std::vector<std::thread> ts;
  ts.reserve(nt);
  for (int t = 0; t + 1 < nt; ++t) {
    try { ts.emplace_back(work); } catch (const std::system_error&) { break; }
  }
  work();
  for (auto& t : ts) t.join();
}

// BNMTF_CREATE_TIMING=1: wall-clock laps of bnmtf_create's phases on stderr
struct CreateLaps {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  bool on = getenv("BNMTF_CREATE_TIMING") != nullptr;
  void lap(const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (on) fprintf(stderr, "bnmtf_create: %-44s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// The environment's say in the layout, read in ONE place (from_env) when a layout is built: a switch flipped later does not
// change a model that exists.  An empty optional: the variable is not set (the unit-per-wave tables are skipped when BNMTF_WIDE
// or BNMTF_FAST_NW is merely present); otherwise its atoi.
struct LayoutSwitches {
  std::optional<int> wide;        // BNMTF_WIDE: 0 never the 16-wave shape, else whenever it can run
  std::optional<int> fast_nw;     // BNMTF_FAST_NW: 2 / 4 waves per block of the pair layout, anything else 8
  std::optional<int> unit;        // BNMTF_UNIT: 0 no unit-per-wave tables
  std::optional<int> unit_nw;     // BNMTF_UNIT_NW: 8 unit waves per block, anything else 4
  bool no_chunks = false;         // BNMTF_NO_CHUNKS: never cut the inner extent in two chunks
  int vb_path = 0;                // BNMTF_VB_PATH: 1 masked, 2 pairs, 0 by policy (unset or anything else)
  // make EXPERIMENTS=1 only (A/B switches of decisions that are made); otherwise as below, whatever the environment holds
  bool balance = true;            // BNMTF_BALANCE=0: the padded conflict-free layout
  std::optional<int> turns;       // BNMTF_TURNS
  std::optional<int> twin;        // BNMTF_TWIN
  static LayoutSwitches from_env();
};

struct MissingView { const uint32_t* idx; uint32_t count; };     // a unit's missing inner indices, ascending

struct SlotLayoutInput {
  int n = 0, m = 0, KP = 32, world = 1;    // local units, inner extent, padded factor width (32 / 64), ranks of the run
  const MissingView* miss = nullptr;       // [n]
  LayoutSwitches sw;
};

// What the sweep kernels are given (kernels.h FastArgs; model.h Dir keeps the scalars and the uploaded tables)
struct SlotLayout {
  // geometry: inner extent rounded up to 32, panel floats, chunks (1 or 2), first inner index of chunk 1, panel floats of the
  // longer chunk / of chunk 1, every inner index and sentinel fits 16 bits
  int mz = 0, pw = 0, nch = 1, mh = 0, pw_chunk = 0, pw1 = 0;
  bool pair_ok = false;
  // the chosen shapes
  bool wide_can = false, use_wide = false, use_turns = false, use_twin = false;
  int f_nw = 8, vb_path = 0;
  bool uw_ok = false;
  int u_nw = 4, ho_ppb = 0, stats_blocks = 0;
  // the pair layout: a unit per 32-lane half wave
  std::vector<int> unit_map;               // [2 npairs] local unit of each half wave, or -1
  std::vector<uint32_t> pair_E, pair_base; // [npairs] slot rows of the pair, its first row
  std::vector<uint32_t> off;               // [max(slots, 1)][64] inner index, or the sentinel mz + lane % 32
  std::vector<uint32_t> off16;             // [max(slots / 2, 1)][64] rows 2h (low half) and 2h + 1 packed; zeros unless pair_ok
  int npairs = 0, emax = 0;
  size_t slots = 0;
  std::vector<int> gen_units;              // units left to the generic kernel
  std::vector<uint16_t> row_blk;           // [max(slots, 1)] block of every slot row when ho_ppb > 0, else empty
  // the unit-per-wave layout (uw_ok; empty otherwise): pair p = unit p, both halves
  std::vector<int> u_unit_map;
  std::vector<uint32_t> u_pair_E, u_pair_base, u_off16;
  int u_emax = 0;
};

// laps: bnmtf_create's timing laps (null: none)
void build_slot_layout(const SlotLayoutInput& in, SlotLayout& out, CreateLaps* laps = nullptr);

}  // namespace bnmtf
