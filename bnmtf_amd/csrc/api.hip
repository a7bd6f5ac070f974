// C ABI of libbnmtf_hip.so (include/bnmtf_hip.h): model construction (host-side
// layout of the masked matrix for the two sweep directions), state hand-off, the
// Gibbs / VB drivers that enqueue the kernels on the handle's stream.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <exception>
#include <map>
#include <new>
#include <system_error>
#include <thread>
#include <tuple>
#include <vector>

#include "model.h"
#include "slot_layout.h"
#include "comm.h"
#include "many.h"
#include "device_rng.h"

namespace bnmtf {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
}  // namespace bnmtf
// (BNMTF_ABI_GUARD, the handler every entry point that returns a status ends in: model.h)
extern "C" int bnmtf_shard_range(int64_t n, int rank, int world, int64_t* first, int64_t* count);
namespace bnmtf {
static void np_free(bnmtf_model* h);   // api_np.inc
static void obs_free(bnmtf_model* h);  // api_obs.inc
static bool obs_is_np(const bnmtf_model* h);   // api_obs.inc: a handle of bnmtf_onp_create

template <typename T>
static int dalloc(T** p, size_t count, bool zero = true) {
  if (count == 0) count = 1;
  HIPCHK(hipMalloc((void**)p, count * sizeof(T)));
  if (zero) { HIPCHK(hipMemset(*p, 0, count * sizeof(T))); HIPCHK(hipDeviceSynchronize()); }
  return BNMTF_OK;
}
template <typename T>
static void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}
// a host table onto the device, in an allocation of its own (at least one element); returns with the copy done
template <typename T>
static int upload(T** dst, const std::vector<T>& src, hipStream_t st) {
  CHK(dalloc(dst, src.size(), false));
  if (!src.empty()) HIPCHK(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));            // (src is the caller's local)
  return BNMTF_OK;
}

// a handle of bnmtf_obs_create, -- the tri-factorisation, L > 0 -- bnmtf_otri_create or -- NMF / NMTF -- bnmtf_onp_create (the
// observed-entry layout, api_obs.inc) holds none of what the other entry points work on
static int refuse_obs(const bnmtf_model* h, const char* fn) {
  if (h && h->obs) {      // (fn null: reached through ensure_std, from any of the sampler and variational calls)
    set_error("%s%sa handle of %s calls (layout='observed')", fn ? fn : "", fn ? ": " : "",
              obs_is_np(h) ? "bnmtf_onp_create runs only the bnmtf_onp_*"
                           : h->L > 0 ? "bnmtf_otri_create runs only the bnmtf_otri_*" : "bnmtf_obs_create runs only the bnmf_obs_*");
    return BNMTF_EINVAL;
  }
  return BNMTF_OK;
}

// A model search builds and destroys a model per candidate (fold x rank x restart), all of the same few sizes: the one device
// allocation of a small model and its stream are handed back to a per-process pool instead of to the driver (hipMalloc / hipFree /
// stream creation are 0.3-1.5 ms each, a 1 000-iteration run of a toy model 15 ms).  Bounded: 256 MB of buffers, 64 streams.
struct DevicePool {
  std::mutex mu;
  std::vector<std::tuple<int, size_t, void*>> bufs;     // (device, bytes, pointer)
  std::vector<std::pair<int, hipStream_t>> streams;
  size_t held = 0;
  void* take(int dev, size_t bytes) {
    std::lock_guard<std::mutex> g(mu);
    for (size_t i = 0; i < bufs.size(); ++i)
      if (std::get<0>(bufs[i]) == dev && std::get<1>(bufs[i]) == bytes) { void* p = std::get<2>(bufs[i]); held -= bytes; bufs.erase(bufs.begin() + i); return p; }
    return nullptr;
  }
  bool give(int dev, size_t bytes, void* p) {
    std::lock_guard<std::mutex> g(mu);
    if (held + bytes > ((size_t)256 << 20) || bufs.size() >= 512) return false;
    bufs.emplace_back(dev, bytes, p); held += bytes;
    return true;
  }
  hipStream_t take_stream(int dev) {
    std::lock_guard<std::mutex> g(mu);
    for (size_t i = 0; i < streams.size(); ++i)
      if (streams[i].first == dev) { hipStream_t s = streams[i].second; streams.erase(streams.begin() + i); return s; }
    return nullptr;
  }
  bool give_stream(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> g(mu);
    if (streams.size() >= 64) return false;
    streams.emplace_back(dev, s);
    return true;
  }
};
static DevicePool& device_pool() { static DevicePool* p = new DevicePool(); return *p; }      // (never destroyed: the driver may be gone at exit)

// events / scratch buffers of one call: released on every return path
struct EventList {
  std::vector<hipEvent_t> ev;
  int create(size_t n) {
    ev.reserve(n);
    for (size_t i = 0; i < n; ++i) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); }
    return BNMTF_OK;
  }
  hipEvent_t operator[](size_t i) const { return ev[i]; }
  // out[it] = seconds from ev[0] to ev[it + 1], the stamp behind iteration `it` (the stream is drained); out may be null
  void seconds(int n_iter, double* out) const {
    for (int it = 0; out && it < n_iter; ++it) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[it + 1]); out[it] = (double)ms * 1e-3; }
  }
  ~EventList() { for (auto e : ev) (void)hipEventDestroy(e); }
};
// the variational models' record of n_iter iterations of 16 doubles each: [0] exptau, [1..3] MSE / R^2 / Rp, [4..13] the ELBO's
// terms; any output may be null
static void unpack_vb_rec(const double* rec, int n_iter, double* exptau, double* perf, double* terms) {
  for (int it = 0; it < n_iter; ++it) {
    const double* q = rec + (size_t)it * 16;
    if (exptau) exptau[it] = q[0];
    if (perf) for (int m = 0; m < 3; ++m) perf[(size_t)it * 3 + m] = q[1 + m];
    if (terms) for (int m = 0; m < 10; ++m) terms[(size_t)it * 10 + m] = q[4 + m];
  }
}
static int vb_reserve_rec(bnmtf_model* h, int n_iter) {      // room on the device for that record
  if (h->vb_rec_cap >= (size_t)n_iter) return BNMTF_OK;
  dfree(h->vb_rec); h->vb_rec_cap = 0;
  CHK(dalloc(&h->vb_rec, (size_t)n_iter * 16));
  h->vb_rec_cap = n_iter;
  return BNMTF_OK;
}
template <typename T>
struct DevBuf {
  T* p = nullptr;
  int alloc(size_t count, bool zero = false) { return dalloc(&p, count, zero); }
  ~DevBuf() { dfree(p); }
};
// the stream and the three events of one call that takes no handle (api_predictive.inc, api_log_predictive.inc, api_top.inc, api_foldin.inc, api_predictive_q.inc): event 0
// before an upload, 1 behind it, 2 behind the kernel; released on every return path
struct CallScope {
  hipStream_t s = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int open(int device) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    return BNMTF_OK;
  }
  int mark(int i) { HIPCHK(hipEventRecord(ev[i], s)); return BNMTF_OK; }
  int elapsed(double* upload_ms, double* kernel_ms) const {      // (events 0 - 1 and 1 - 2, which the caller has waited for)
    float up = 0.f, kn = 0.f;
    HIPCHK(hipEventElapsedTime(&up, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&kn, ev[1], ev[2]));
    *upload_ms = up; *kernel_ms = kn;
    return BNMTF_OK;
  }
  ~CallScope() {
    for (int i = 2; i >= 0; --i) if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (s) (void)hipStreamDestroy(s);
  }
};
// upload and kernel time of this host thread's last call of each of the five, from the events (bnmtf_*_times)
enum CallKind { kCallPredictive, kCallTop, kCallFoldIn, kCallPredictiveQ, kCallLogPredictive, kCallKinds };
static thread_local double g_call_ms[kCallKinds][2] = {};
static int call_times(const char* who, CallKind kind, double* upload_ms, double* kernel_ms) {
  if (!upload_ms || !kernel_ms) { set_error("%s: null argument", who); return BNMTF_EINVAL; }
  *upload_ms = g_call_ms[kind][0]; *kernel_ms = g_call_ms[kind][1];
  return BNMTF_OK;
}

// What the calls over an entry list and the host's stored samples share (api_predictive.inc, api_log_predictive.inc; the sort also
// api_predictive_q.inc).
// The list by row, in the given order within a row: a stable counting sort.  rowptr [I + 1], col [n] the columns in list order,
// perm [n] the given position of list position q: the outputs are scattered back through it.
static void sort_entries_by_row(int I, uint64_t n, const int32_t* rows, const int32_t* cols, std::vector<uint32_t>& rowptr,
                                std::vector<uint32_t>& col, std::vector<uint32_t>& perm) {
  rowptr.assign((size_t)I + 1, 0u); col.resize(n); perm.resize(n);
  for (uint64_t e = 0; e < n; ++e) rowptr[(size_t)rows[e] + 1]++;
  for (int i = 0; i < I; ++i) rowptr[(size_t)i + 1] += rowptr[i];
  std::vector<uint32_t> at(rowptr.begin(), rowptr.end() - 1);
  for (uint64_t e = 0; e < n; ++e) { const uint32_t q = at[rows[e]]++; col[q] = (uint32_t)cols[e]; perm[q] = (uint32_t)e; }
}
constexpr size_t kSampleStageBytes = (size_t)256 << 20;          // chunk_samples = 0: as many samples as fit this, at least one
// samples per upload and launch: chunk_samples, or with 0 what fits the staging size; at most T
static int sample_chunk(int chunk_samples, int T, size_t floats_per_sample) {
  int chunk = chunk_samples;
  if (chunk == 0) {
    const size_t fit = kSampleStageBytes / (floats_per_sample * sizeof(float));
    chunk = fit < 1 ? 1 : fit > (size_t)T ? T : (int)fit;
  }
  return chunk > T ? T : chunk;
}
// samples [t0, t0 + c) of the call, array indices first + t * step, `per` floats each, onto dst
static int upload_samples(float* dst, const float* src, size_t per, uint64_t first, uint64_t step, int t0, int c, hipStream_t st) {
  if (step == 1) {
    HIPCHK(hipMemcpyAsync(dst, src + (first + (uint64_t)t0) * per, (size_t)c * per * sizeof(float), hipMemcpyHostToDevice, st));
    return BNMTF_OK;
  }
  for (int s = 0; s < c; ++s)
    HIPCHK(hipMemcpyAsync(dst + (size_t)s * per, src + (first + (uint64_t)(t0 + s) * step) * per, per * sizeof(float), hipMemcpyHostToDevice, st));
  return BNMTF_OK;
}

// ------------------------------------------------------------------ layout
// Fill one direction: the contraction's split geometry, the I x J passes on the device (kernel_layout.hip: masked / transposed
// contraction operand, missing lists) and their download, the slot layout from the downloaded lists (one call into
// slot_layout.hip: host code), the uploads and the remaining allocations.
// dR / dM: the data and the mask on the device ([I][J] row major); by_rows: a unit is a row of R (else a column); obs: observed
// entries per unit (global).
static int build_dir(Dir& d, int nglob, int m, int W, int rank, int world, const double* lambda,
                     const float* dR, const uint8_t* dM, int I, int J, bool by_rows, const std::vector<uint32_t>& obs, hipStream_t st) {
  d.nglob = nglob; d.m = m; d.W = W; d.KP = W <= 32 ? 32 : 64;
  {
    int64_t first = 0, count = 0;
    (void)bnmtf_shard_range(nglob, rank, world, &first, &count);
    d.n0 = (int)first; d.n = (int)count;
  }
  d.n_pad = round_up(std::max(d.n, 1), 128);
  // split of the inner dimension: aim at >= 2 blocks per CU, >= 64 inner rows per wave
  // a wave covers 128 output columns (four 32-column tiles); when the output side is short (a shard of a multi-GPU run)
  // 64 columns, so that the chip is filled with half as many inner slices, each twice as long (BNMTF_GEMM_TW=2/4 forces)
  d.gemm_tw = (d.KP == 64 && d.n_pad <= 2048) ? 2 : 4;
#ifdef BNMTF_EXPERIMENTS       // (A/B switches of decisions that are made: make EXPERIMENTS=1)
  if (const char* e = getenv("BNMTF_GEMM_TW")) d.gemm_tw = atoi(e) == 2 && d.KP == 64 ? 2 : 4;
#endif
  const int tiles = d.n_pad / (32 * d.gemm_tw);
  // one block per CU: at KP = 64 the GEMM holds 332 registers per lane (one resident block), and at KP = 32 -- where two
  // would fit -- 256 blocks with twice the inner slice per wave beat 512 (4096^2, K = 32: 20.3 us against 23.2; round 3)
  int split = std::max(1, 256 / tiles);
#ifdef BNMTF_EXPERIMENTS
  if (const char* e = getenv("BNMTF_GEMM_SPLIT")) split = std::max(1, atoi(e));
#endif
  const int max_split = std::max(1, m / (4 * 64));
  d.split = std::min(split, max_split);
  d.ipw = round_up((m + d.split * 4 - 1) / (d.split * 4), 32);   // multiple of the GEMM's 2*U register-pipeline group
  d.inner_pad = d.split * 4 * d.ipw;

  CreateLaps laps;
  std::vector<uint32_t> ptr(d.n + 1, 0), idx;
  d.obs_count.assign(nglob, 0);
  d.nmiss = 0;
  for (int ul = 0; ul < d.n; ++ul) {
    const uint32_t cnt = (uint32_t)m - obs[d.n0 + ul];
    d.nmiss += cnt;
    ptr[ul + 1] = ptr[ul] + (cnt + 63u) / 64u * 64u;                 // 64-wide slots, padded with the zero sentinel m
  }
  d.nslots = ptr[d.n];
  CHK(dalloc(&d.big, (size_t)d.inner_pad * d.n_pad));               // zero-filled: the pads stay zero
  CHK(dalloc(&d.slot_ptr, ptr.size(), false));
  HIPCHK(hipMemcpyAsync(d.slot_ptr, ptr.data(), ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CHK(dalloc(&d.idx, std::max<size_t>(d.nslots, 1), false));
  launch_masked_operand(dR, dM, I, J, by_rows ? 1 : 0, d.n0, d.n, m, d.big, d.n_pad, st);
  launch_missing_lists(dM, I, J, by_rows ? 1 : 0, d.n0, d.n, m, d.slot_ptr, d.idx, st);
  idx.resize(d.nslots);
  if (d.nslots) HIPCHK(hipMemcpyAsync(idx.data(), d.idx, d.nslots * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  laps.lap("  build_dir: R~ operand + missing lists (device)");
  // the slot layout of the on-chip sweeps and the choice of their block shape: host arithmetic on the downloaded lists
  // (slot_layout.hip; the environment's switches are read there, once, now)
  SlotLayout lay;
  {
    std::vector<MissingView> miss(d.n);
    for (int ul = 0; ul < d.n; ++ul) miss[ul] = {idx.data() + ptr[ul], (uint32_t)m - obs[d.n0 + ul]};
    SlotLayoutInput in;
    in.n = d.n; in.m = m; in.KP = d.KP; in.world = world; in.miss = miss.data(); in.sw = LayoutSwitches::from_env();
    build_slot_layout(in, lay, &laps);
  }
  d.mz = lay.mz; d.pw = lay.pw; d.nch = lay.nch; d.mh = lay.mh; d.pw_chunk = lay.pw_chunk; d.pw1 = lay.pw1; d.pair_ok = lay.pair_ok;
  d.wide_can = lay.wide_can; d.use_wide = lay.use_wide; d.use_turns = lay.use_turns; d.use_twin = lay.use_twin;
  d.f_nw = lay.f_nw; d.vb_path = lay.vb_path; d.ho_ppb = lay.ho_ppb; d.stats_blocks = lay.stats_blocks;
  d.f_npairs = lay.npairs; d.f_emax = lay.emax; d.f_slots = lay.slots; d.f_gen_count = (int)lay.gen_units.size();
  d.uw_ok = lay.uw_ok; d.u_nw = lay.u_nw; d.u_emax = lay.u_emax;
  d.fast_ok = true;
  CHK(upload(&d.f_unit_map, lay.unit_map, st));
  CHK(upload(&d.f_pair_E, lay.pair_E, st));
  CHK(upload(&d.f_pair_base, lay.pair_base, st));
  CHK(upload(&d.f_off, lay.off, st));
  CHK(upload(&d.f_off16, lay.off16, st));
  CHK(upload(&d.f_gen_units, lay.gen_units, st));
  if (d.ho_ppb > 0) CHK(upload(&d.f_row_blk, lay.row_blk, st));       // (what build_handover needs beside the layout itself)
  if (d.uw_ok) {
    CHK(upload(&d.u_unit_map, lay.u_unit_map, st));
    CHK(upload(&d.u_pair_E, lay.u_pair_E, st));
    CHK(upload(&d.u_pair_base, lay.u_pair_base, st));
    CHK(upload(&d.u_off16, lay.u_off16, st));
  }
  CHK(dalloc(&d.stats, (size_t)d.stats_blocks * 4));
  laps.lap("    layout: tables uploaded");
  laps.lap("  build_dir: slot layout + its uploads");
  CHK(dalloc(&d.slabs, (size_t)d.split * d.n_pad * d.KP));
  CHK(dalloc(&d.q, idx.size()));
  std::vector<float> lam((size_t)std::max(d.n, 1) * d.KP, 0.0f);
  for (int ul = 0; ul < d.n; ++ul)
    for (int k = 0; k < W; ++k) lam[(size_t)ul * d.KP + k] = (float)lambda[(size_t)(d.n0 + ul) * W + k];
  CHK(upload(&d.lambda, lam, st));
  // C64 | colsum | colsum2 in one piece: what a multi-GPU run sums over the ranks with ONE all-reduce (exchange_factor)
  CHK(dalloc(&d.C64, (size_t)64 * 64 + 128));
  d.colsum = d.C64 + 64 * 64; d.colsum2 = d.colsum + 64; d.gram_packed = true;
  CHK(dalloc(&d.C32, (size_t)64 * 64));
  CHK(dalloc(&d.numer, (size_t)std::max(d.n, 1)));
  CHK(dalloc(&d.taup, (size_t)std::max(d.n, 1)));
  return BNMTF_OK;
}

// q hand-over tables for one writer / reader pair of directions (model.h Dir::ho_*), built on the device from the two slot
// layouts (kernel_handover.hip).  Returns false (and leaves the pair without hand-over) if a staging area or a region would
// not fit the block's LDS or its 16-bit offsets.
static bool build_handover(bnmtf_model* h, Dir& W, Dir& Rd) {
  if (!W.f_row_blk || !Rd.f_row_blk || W.f_npairs == 0 || Rd.f_npairs == 0) return false;
  const int nbW = (W.f_npairs + W.ho_ppb - 1) / W.ho_ppb, nbR = (Rd.f_npairs + Rd.ho_ppb - 1) / Rd.ho_ppb;
  if (nbR > 8192) return false;                         // (the destination kernel counts per reader block in LDS)
  const size_t rowsW = W.f_slots, rowsR = Rd.f_slots;
  DevBuf<uint32_t> inv, dst_slot, dst_rank, count, sbase, stotal, rbase, rdata, rsize, limits;
  if (inv.alloc(std::max<size_t>(Rd.nslots, 1)) || dst_slot.alloc(std::max<size_t>(rowsW, 1) * 64) || dst_rank.alloc(std::max<size_t>(rowsW, 1) * 64) ||
      count.alloc((size_t)nbW * nbR) || sbase.alloc((size_t)nbW * nbR) || stotal.alloc(nbW) || rbase.alloc((size_t)nbW * nbR) || rdata.alloc(nbR) ||
      rsize.alloc(nbR) || limits.alloc(4, true)) return false;
  uint16_t *t_out = nullptr, *t_in = nullptr;
  // (two 16-bit places per word; an odd row count leaves the last word's upper half unused)
  if (dalloc(&t_out, ((rowsW + 1) / 2) * 128, true) || dalloc(&t_in, ((rowsR + 1) / 2) * 128, true)) return false;
  W.ho_out = reinterpret_cast<uint32_t*>(t_out); Rd.ho_in = reinterpret_cast<uint32_t*>(t_in);
  if (dalloc(&W.ho_pk, (size_t)nbW * nbR * 3, false) || dalloc(&Rd.ho_region_ofs, (size_t)nbR + 1, false)) return false;
  HandoverArgs a;
  a.w_off = W.f_off; a.w_pB = W.f_pair_base; a.w_pE = W.f_pair_E; a.w_umap = W.f_unit_map; a.w_npairs = W.f_npairs; a.w_ppb = W.ho_ppb; a.w_nb = nbW; a.w_inner = (uint32_t)Rd.nglob;
  a.r_off = Rd.f_off; a.r_pB = Rd.f_pair_base; a.r_pE = Rd.f_pair_E; a.r_umap = Rd.f_unit_map; a.r_npairs = Rd.f_npairs; a.r_ppb = Rd.ho_ppb; a.r_nb = nbR; a.r_inner = (uint32_t)W.nglob;
  a.r_row_blk = Rd.f_row_blk; a.r_ptr = Rd.slot_ptr; a.r_idx = Rd.idx;
  a.inv = inv.p; a.dst_slot = dst_slot.p; a.dst_rank = dst_rank.p; a.count = count.p;
  a.sbase = sbase.p; a.stotal = stotal.p; a.rbase = rbase.p; a.rdata = rdata.p; a.rsize = rsize.p;
  a.rofs = Rd.ho_region_ofs; a.t_out = t_out; a.t_in = t_in; a.pk = W.ho_pk; a.limits = limits.p;
  launch_handover_build(a, h->stream);
  uint32_t lim[4];
  if (hipMemcpyAsync(lim, limits.p, sizeof(lim), hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return false;
  // staging area and region live behind the Gram in the block's LDS (160 KiB in all; the launch asks for what they need)
  // (8-wave blocks run two to a CU: half the LDS each.  256: the VB kernel's small arrays ahead of the panels)
  const uint32_t lds_w = (W.ho_ppb == 8 ? 80u : 160u) * 1024u / 4u - (uint32_t)(W.KP * W.KP) - 256u;
  const uint32_t lds_r = (Rd.ho_ppb == 8 ? 80u : 160u) * 1024u / 4u - (uint32_t)(W.KP * W.KP) - 256u;
  if (lim[2] != 0 || lim[0] + 256u + 32u > lds_w || lim[0] + 32u > 65536u || lim[1] > lds_r || lim[1] > 65536u) return false;
  W.ho_lds_floats = std::max(W.ho_lds_floats, (int)lim[0] + 256 + 32);
  Rd.ho_lds_floats = std::max(Rd.ho_lds_floats, (int)lim[1]);
  if (dalloc(&Rd.ho_region, (size_t)lim[3] + 256) != BNMTF_OK) return false;      // zero-filled: the zeros behind the runs are never written
  Rd.ho_blocks = nbR;
  return true;
}

static int alloc_factor(Dir& d, int other_inner_pad) {
  d.xrows = std::max(d.nglob + 1, other_inner_pad);
  d.ldT = round_up(round_up(d.nglob, 32) + 32, 256);   // = the other direction's panel size pw; zero beyond nglob
  CHK(dalloc(&d.X, (size_t)d.xrows * d.KP));
  CHK(dalloc(&d.XT, (size_t)d.KP * d.ldT));
  CHK(dalloc(&d.XT2, (size_t)d.KP * d.ldT));
  const int nb = post_blocks(d.nglob);
  CHK(dalloc(&d.Cpart, (size_t)nb * d.KP * d.KP));
  CHK(dalloc(&d.spart, (size_t)nb * d.KP));
  CHK(dalloc(&d.s2part, (size_t)nb * d.KP));
  return BNMTF_OK;
}

static void free_dir(Dir& d) {
  dfree(d.big); dfree(d.slabs); dfree(d.lambda); dfree(d.slot_ptr); dfree(d.idx); dfree(d.q);
  dfree(d.X); dfree(d.XT); dfree(d.C64); dfree(d.C32);
  if (!d.gram_packed) { dfree(d.colsum); dfree(d.colsum2); }
  if (d.ev_sweep) (void)hipEventDestroy(d.ev_sweep);
  if (d.ev_gram) (void)hipEventDestroy(d.ev_gram);
  if (d.ev_gathered) (void)hipEventDestroy(d.ev_gathered);
  if (d.ev_gram_all) (void)hipEventDestroy(d.ev_gram_all);
  dfree(d.XT2); dfree(d.Cpart); dfree(d.spart); dfree(d.s2part); dfree(d.f_unit_map); dfree(d.f_pair_E);
  dfree(d.f_pair_base); dfree(d.f_off); dfree(d.f_off16); dfree(d.stats); dfree(d.f_gen_units);
  dfree(d.u_unit_map); dfree(d.u_pair_E); dfree(d.u_pair_base); dfree(d.u_off16);
  dfree(d.vb_stats);
  dfree(d.ho_in); dfree(d.ho_out); dfree(d.ho_pk); dfree(d.ho_region_ofs); dfree(d.ho_region); dfree(d.f_row_blk);
  dfree(d.mu); dfree(d.tauq); dfree(d.var); dfree(d.S2); dfree(d.S2T); dfree(d.XS); dfree(d.vb_asq); dfree(d.vb_vsq); dfree(d.mbits); dfree(d.XB); dfree(d.mslabs); dfree(d.xb_umax); dfree(d.xb_cexp); dfree(d.xb_mpart); dfree(d.numer); dfree(d.taup);
}

// ---------------------------------------------------------------- profiling
struct ScopedKernelTimer {
  bnmtf_model* h; int id; hipEvent_t a = nullptr, b = nullptr;
  bool on;
  ScopedKernelTimer(bnmtf_model* h_, int id_) : h(h_), id(id_), on(((h_->profiling >> id_) & 1u) && h_->iteration % h_->profile_stride == 0) {
    if (!on) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!h->event_pool.empty()) { e = h->event_pool.back(); h->event_pool.pop_back(); }
      else (void)hipEventCreate(&e);
      return e;
    };
    a = get(); b = get();
    (void)hipEventRecord(a, h->stream);
  }
  ~ScopedKernelTimer() {
    if (!on) return;
    (void)hipEventRecord(b, h->stream);
    h->pending_events.push_back({id, {a, b}});
  }
};
static void drain_events(bnmtf_model* h) {
  for (auto& pe : h->pending_events) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pe.second.first, pe.second.second) == hipSuccess) {
      h->kernel_ms[pe.first] += ms;
      h->kernel_launches[pe.first] += 1;
    }
    h->event_pool.push_back(pe.second.first);
    h->event_pool.push_back(pe.second.second);
  }
  h->pending_events.clear();
}

// q hand-over between the half sweeps, for the duration of one run call: from its first rows sweep (a pre-pass) on
struct HandoverScope {
  bnmtf_model* h;
  // (a call that follows another one of the same handle with the state untouched in between picks the regions up where that
  // call left them: run(50) + run(50) is the chain of run(100), bit for bit)
  explicit HandoverScope(bnmtf_model* h_) : h(h_) {
    h->ho_active = h->ho_enabled && !h->comm && h->use_fast && !h->block_mode;
    if (!h->ho_active || !h->ho_regions_current) h->rows.ho_filled = h->cols.ho_filled = false;
    h->ho_regions_current = false;            // (an error return out of the loop leaves them unknown)
  }
  // the run loop has finished and its stream is drained: the regions hold q of the state the call leaves behind
  void commit() { h->ho_regions_current = h->ho_active && h->rows.ho_filled; }
  ~HandoverScope() { h->ho_active = false; }        // (an error return never got to commit(): the regions stay "unknown")
};
// ------------------------------------------------------------- step pieces
static void enqueue_gemm(bnmtf_model* h, Dir& d, const Dir& other, int kid, int part = 0);
// part: 0 the whole contraction; 1 only the inner slices that lie inside the rank's OWN block of the other factor (rows
// [other.n0, other.n0 + other.n): final the moment the rank's sweep ends, before any exchange); 2 the remaining slices
static void enqueue_gemm(bnmtf_model* h, Dir& d, const Dir& other, int kid, int part) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));                              // (padding too: a recorded list compares argument bytes)
  g.big = d.big; g.ld = d.n_pad; g.X = other.X; g.slabs = d.slabs;
  g.n_pad = d.n_pad; g.split = d.split; g.inner_per_wave = d.ipw; g.tw = d.gemm_tw;
  const int rows_per_slice = 4 * d.ipw;
  const int s0 = (other.n0 + rows_per_slice - 1) / rows_per_slice, s1 = std::min(d.split, (other.n0 + other.n) / rows_per_slice);
  const bool have_local = h->comm && s1 > s0;
  if (part == 1) {
    if (!have_local) return;
    ScopedKernelTimer t(h, kid);
    g.split0 = s0; g.nsplit = s1 - s0;
    launch_gemm(g, d.KP, h->stream);
    return;
  }
  ScopedKernelTimer t(h, kid);
  if (part == 2 && have_local) {
    if (s0 > 0) { g.split0 = 0; g.nsplit = s0; launch_gemm(g, d.KP, h->stream); }
    if (s1 < d.split) { g.split0 = s1; g.nsplit = d.split - s1; launch_gemm(g, d.KP, h->stream); }
    return;
  }
  launch_gemm(g, d.KP, h->stream);
}
// relayout (XT, XT2) + Gram of a factor that was just written
// the variational half sweep of direction d (other factor o) runs on the on-chip kernels (api_models.inc: enqueue_vb_sweep)
// Policy (same-box A/Bs): the product's fixed cost (bits x digit planes, column maxima, planes, slab reads) pays when
// a column loop is 64 columns of a 16-wave block -- 8192^2, K = 64: +7 % -- and does not at K <= 32 (4096^2: -15 %, 8192^2: -5 %),
// where the pair-panel kernel (kernel_sweep_vb.hip) stays.  BNMTF_VB_PATH=masked / pairs forces one of them -- read ONCE, when the
// model's layout is built: the relayout of one half sweep builds what the next one's kernel reads (the pair panels or not), so a
// switch flipped between two calls must not change the path of a model that exists (round 4's advice).
static bool vb_chip_ok(const Dir& d, const Dir& o) {
  if (!(d.mbits && o.XB && d.mslabs && d.nch == 1 && sweep_fast_supported(d.KP, d.pw))) return false;
  if (d.vb_path != 0) return d.vb_path == 1;
  return d.KP == 64 && d.use_wide;
}
static void enqueue_post(bnmtf_model* h, Dir& d, bool vb = false, hipStream_t st = nullptr) {      // st: null = the compute stream
  PostArgs g;
  memset(&g, 0, sizeof(g));
  g.X = d.X; g.rows = d.nglob; g.KP = d.KP; g.XT = d.XT; g.ldT = d.ldT; g.XT2 = d.XT2; g.ld2 = d.ldT;
  g.Cpart = d.Cpart; g.spart = d.spart; g.C64 = d.C64; g.C32 = d.C32; g.colsum = d.colsum;
  if (vb) { g.S2 = d.S2; g.S2T = d.S2T; g.s2part = d.s2part; g.colsum2 = d.colsum2; g.XS = d.XS; }
  // (the (E, S2) pair panels are read by the pair-panel VB kernel only: the on-chip path takes its masked sums from kernel_maskgemm.hip)
  if (vb && vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows)) {
    g.XS = nullptr;
    // ... and needs the column maxima of [S2 | E^2] (the fixed-point grid of its digit planes): the Gram blocks see every row anyway
    g.mpart = d.xb_mpart; g.umax = d.xb_umax;
    d.xb_umax_posted = d.xb_mpart != nullptr;
  } else d.xb_umax_posted = false;
  g.snap = d.snap_dst; g.snapW = d.W; d.snap_dst = nullptr;
  launch_post(g, st ? st : h->stream);
}
// Several GPUs, after a half sweep: the block of X this rank has just drawn goes to the other ranks (all-gather on the
// exchange stream) WHILE the rank forms the Gram partial and the column sums of its own rows; the partials -- one buffer,
// C64 | colsum -- are then summed over the ranks by one all-reduce (north_star's "all-reduce on the K x K Gram matrices";
// every rank used to form the whole Gram from the gathered factor), which runs beside the relayout of the gathered factor
// and the next contraction.  The compute stream waits for the gathered factor here and for the summed Gram in await_gram(),
// just ahead of its first reader.  Every collective is issued on the ONE exchange stream, in the same order on all ranks.
// next / next_kid: the direction whose contraction reads d's factor next.  Its inner slices over this rank's OWN rows of the
// factor are launched here, ahead of the wait for the other ranks' blocks (they are final, whatever the others send); the
// remaining slices behind the relayout of the gathered factor.  Every slice writes its own slab and the sweep adds the slabs
// in slab order, so the chain is the same bits as with one launch.
static int exchange_factor(bnmtf_model* h, Dir& d, Dir* next = nullptr, int next_kid = 0) {
  if (!h->comm) { enqueue_post(h, d); return BNMTF_OK; }
  // BNMTF_EXCHANGE=serial: every collective on the compute stream, in program order, nothing overlapped -- the fall-back
  // while the two-stream ordering below has not run on a node with several GPUs (round 3's advice; tests/test_rccl_two_process_gpu.py)
  const char* xe = getenv("BNMTF_EXCHANGE");            // (read per call: the sharded tests run both orderings in one process)
  if (xe && !strcmp(xe, "serial")) {
    PostArgs g;
    memset(&g, 0, sizeof(g));
    g.X = d.X; g.rows = d.nglob; g.KP = d.KP; g.XT = d.XT; g.ldT = d.ldT; g.XT2 = d.XT2; g.ld2 = d.ldT;
    g.Cpart = d.Cpart; g.spart = d.spart; g.C64 = d.C64; g.C32 = d.C32; g.colsum = d.colsum;
    launch_post_gram_rows(g, d.n0, d.n0 + d.n, h->stream);
    CHK(comm_allgather_factor(h->comm, d.X, d.KP, d.nglob, h->world, h->stream));
    CHK(comm_allreduce_sum(h->comm, d.C64, 64 * 64 + 64, h->stream));
    launch_gram_cast(d.C64, d.C32, d.KP * d.KP, h->stream);
    g.snap = d.snap_dst; g.snapW = d.W; d.snap_dst = nullptr;
    launch_post_layout(g, h->stream);
    d.gram_pending = false;
    return BNMTF_OK;
  }
  if (!h->xchg_stream) HIPCHK(hipStreamCreateWithFlags(&h->xchg_stream, hipStreamNonBlocking));
  for (hipEvent_t* e : {&d.ev_sweep, &d.ev_gram, &d.ev_gathered, &d.ev_gram_all})
    if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  PostArgs g;
  memset(&g, 0, sizeof(g));
  g.X = d.X; g.rows = d.nglob; g.KP = d.KP; g.XT = d.XT; g.ldT = d.ldT; g.XT2 = d.XT2; g.ld2 = d.ldT;
  g.Cpart = d.Cpart; g.spart = d.spart; g.C64 = d.C64; g.C32 = d.C32; g.colsum = d.colsum;
  HIPCHK(hipEventRecord(d.ev_sweep, h->stream));
  launch_post_gram_rows(g, d.n0, d.n0 + d.n, h->stream);             // own rows only: they are final, whatever the others send
  HIPCHK(hipEventRecord(d.ev_gram, h->stream));
  if (next) enqueue_gemm(h, *next, d, next_kid, 1);
  HIPCHK(hipStreamWaitEvent(h->xchg_stream, d.ev_sweep, 0));
  CHK(comm_allgather_factor(h->comm, d.X, d.KP, d.nglob, h->world, h->xchg_stream));
  HIPCHK(hipEventRecord(d.ev_gathered, h->xchg_stream));
  HIPCHK(hipStreamWaitEvent(h->xchg_stream, d.ev_gram, 0));
  CHK(comm_allreduce_sum(h->comm, d.C64, 64 * 64 + 64, h->xchg_stream));          // C64 | colsum
  launch_gram_cast(d.C64, d.C32, d.KP * d.KP, h->xchg_stream);
  HIPCHK(hipEventRecord(d.ev_gram_all, h->xchg_stream));
  d.gram_pending = true;
  HIPCHK(hipStreamWaitEvent(h->stream, d.ev_gathered, 0));
  g.snap = d.snap_dst; g.snapW = d.W; d.snap_dst = nullptr;
  launch_post_layout(g, h->stream);
  if (next) { enqueue_gemm(h, *next, d, next_kid, 2); next->gemm_ahead = true; }
  return BNMTF_OK;
}
// One GPU, bnmf_gibbs_run: what follows a half sweep -- the relayout and the Gram of the factor it wrote (post_kernel,
// gram_reduce_kernel) and, behind the V sweep, the end of the iteration (finish_kernel, the posterior sums, the sample slot's
// event) -- is read by nothing on the compute stream before the NEXT sweep: the contraction in between reads the factor's X
// alone.  So it goes to a second stream, beside that contraction, which is HBM-bound with one wave per SIMD and leaves the
// tail kernels the registers and the LDS they need (launch_post's note):
//   main:  gemm_rows | sweep_rows | fork(0) | gemm_cols ............ | join(0) | sweep_cols | fork(1) | gemm_rows(it+1) ........ | join(1) | sweep_rows
//   tail:                           wait    | post(U) | gram(U) | done(0)                     wait    | post(V) | gram(V) | finish | done(1)
// Every reader is behind its join: sweep_cols reads U's XT / XT2 / C32, finish (on the tail stream, in order behind both
// relayouts) both Grams, the V sweep's statistics and acc; the next sweep_rows reads V's layouts and the tau that finish wrote.
// Write after read: sweep_rows(it+1) overwrites the U.X that post(U)(it) and the posterior sums of iteration it read -- both
// joined before it, at join(0) and join(1) of iteration it; sweep_cols(it) overwrites the V.X that post(V)(it-1) read, joined
// at join(1) of it-1; the memset of acc ahead of sweep_cols(it) follows join(1) of it-1, behind the finish that read it.  The
// sample slots are written, and their events recorded and waited for, on the tail stream (SampleSink::writer).
// BNMTF_TAIL=serial (read at bnmtf_create), a communicator, a small problem (tail_overlap_wanted) or any other loop: everything
// on the compute stream, as before.
// By default only where the contraction is long enough to hide the tail and to pay for the four cross-stream edges of an
// iteration (a few microseconds each on the compute stream): measured, same box, against the parent -- 8192 x 8192: K = 64
// +5.6 %, K = 32 +2.9 %; 4096 x 4096, K = 32, where the contraction is 16-21 us: -5.4 %.  Sizes in between
// have not been measured and keep the one-stream order.  BNMTF_TAIL=overlap / serial forces either.
static bool tail_overlap_wanted(const bnmtf_model* h) {
  if (h->comm || h->world > 1 || h->L != 0) return false;
  if (h->tail_mode != 0) return h->tail_mode == 1;
  return (int64_t)h->I * h->J >= (int64_t)8192 * 8192;
}
struct TailOverlap {
  bnmtf_model* h = nullptr;
  bool on = false, pending[2] = {false, false};
  int begin(bnmtf_model* h_) {
    h = h_; on = tail_overlap_wanted(h);
    if (!on) return BNMTF_OK;
    // The four events order kernels of this one device against each other and nothing else (the sample copies and the host
    // have events of their own), so they are recorded without the system-scope fence: with it every record wrote back and
    // invalidated the L2 in the middle of the loop -- 7-8 us between a sweep's end and the contraction's start in the trace,
    // and the whole gain of the second stream (measured: DESIGN.md section 7).
    if (!h->tail_stream) HIPCHK(hipStreamCreateWithFlags(&h->tail_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : h->ev_tail)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    return BNMTF_OK;
  }
  hipStream_t stream() const { return on ? h->tail_stream : h->stream; }
  // the sweep of direction dir (0 rows, 1 cols) has been enqueued: what follows on the tail stream starts behind it
  int fork(int dir) {
    HIPCHK(hipEventRecord(h->ev_tail[2 * dir], h->stream));
    HIPCHK(hipStreamWaitEvent(h->tail_stream, h->ev_tail[2 * dir], 0));
    return BNMTF_OK;
  }
  int done(int dir) {
    HIPCHK(hipEventRecord(h->ev_tail[2 * dir + 1], h->tail_stream));
    pending[dir] = true;
    return BNMTF_OK;
  }
  // the compute stream is about to enqueue the first reader of what the tail of direction dir made
  int join(int dir) {
    if (pending[dir]) { HIPCHK(hipStreamWaitEvent(h->stream, h->ev_tail[2 * dir + 1], 0)); pending[dir] = false; }
    return BNMTF_OK;
  }
  // an error return out of the loop leaves nothing running on the tail stream behind the caller's back
  ~TailOverlap() { if (on && (pending[0] || pending[1])) (void)hipStreamSynchronize(h->tail_stream); }
};
// the summed Gram of d (C32, C64, colsum) is about to be read on the compute stream
static int await_gram(bnmtf_model* h, Dir& d) {
  if (d.gram_pending) { HIPCHK(hipStreamWaitEvent(h->stream, d.ev_gram_all, 0)); d.gram_pending = false; }
  return BNMTF_OK;
}
// q hand-over between the half sweeps (the run loops switch it on: bnmf_gibbs_run, bnmf_vb_run): read this direction's region
// if the other direction's last sweep filled it, fill the other's.  Every ho_refresh-th iteration the rows sweep runs its
// pre-pass all the same: q handed back and forth collects one fp32 rounding per column update, the pre-pass starts from X
// again (tools/handover_drift.py: no drift to see at 64).
static void set_handover(bnmtf_model* h, Dir& d, const Dir& other, FastArgs& f, bool kernel_can) {
  f.ho_read = f.ho_write = 0; f.ho_nb_other = 0; f.ho_lds_floats = 0; f.ho_rows_total = (int)d.f_slots;
  f.ho_in = f.ho_out = f.ho_pk = f.ho_region_ofs = nullptr; f.ho_region = nullptr; f.ho_dst = nullptr;
  if (!(h->ho_active && d.ho_ready && other.ho_ready && kernel_can)) return;
  const bool refresh = &d == &h->rows && h->iteration % h->ho_refresh == 0;
  f.ho_read = d.ho_filled && !refresh;
  f.ho_in = d.ho_in; f.ho_region = d.ho_region; f.ho_region_ofs = d.ho_region_ofs;
  f.ho_write = 1; f.ho_nb_other = other.ho_blocks; f.ho_lds_floats = d.ho_lds_floats;
  f.ho_out = d.ho_out; f.ho_pk = d.ho_pk; f.ho_dst = other.ho_region;
  other.ho_filled = true; d.ho_filled = false;
}
static void enqueue_sweep(bnmtf_model* h, Dir& d, const Dir& other, SweepArgs& s, bool want_stats) {
  s.unit_list = nullptr;
  h->last_sweep_fast = false;
  if (h->use_fast && d.uw_ok && other.X && s.cond_k < 0 && s.mode != kSweepVB && !s.cov_S && !s.order && (!h->ho_enabled || h->uw_force)) {
    // few units per CU: one unit per wave (kernel_sweep_unit.hip); every unit of the direction (a layout with a unit beyond
    // kFastMaxSlots slots per lane is not built)
    FastArgs f;
    memset(&f, 0, sizeof(f));
    f.unit_map = d.u_unit_map; f.pair_E = d.u_pair_E; f.pair_base = d.u_pair_base; f.off16 = d.u_off16;
    f.npairs = d.n; f.mz = d.mz; f.pw = d.pw; f.nw = d.u_nw; f.nch = 1;
    f.XoT = other.XT; f.ldT_o = other.ldT; f.Xo = other.X; f.Xo_rows = other.nglob;
    f.stats = want_stats ? d.stats : nullptr;
    SweepArgs s2 = s;
    s2.acc = nullptr;
    if (h->ho_active) { d.ho_filled = false; }        // (q is not handed over by this shape: the next reader of a region rebuilds)
    launch_sweep_unit(s2, f, h->stream);
    h->last_sweep_fast = true;
    return;
  }
  if (h->use_fast && d.fast_ok && s.cond_k < 0 && s.mode != kSweepVB && (d.nch == 2 || sweep_fast_supported(d.KP, d.pw))) {
    FastArgs f;
    f.unit_map = d.f_unit_map; f.pair_E = d.f_pair_E; f.pair_base = d.f_pair_base; f.off = d.f_off;
    f.npairs = d.f_npairs; f.mz = d.mz; f.pw = d.nch == 2 ? d.pw_chunk : d.pw; f.nw = d.f_nw;
    f.nch = d.nch; f.mh = d.mh; f.pw1 = d.pw1; f.twin = d.use_twin ? 1 : 0;
    f.XoT = other.XT; f.ldT_o = other.ldT; f.XoT2 = other.XT2; f.ld2_o = other.ldT; f.Xo = other.X; f.Xo_rows = other.nglob;
    f.stats = want_stats ? d.stats : nullptr;
    SweepArgs s2 = s;
    s2.acc = nullptr;
    f.off16 = d.pair_ok ? d.f_off16 : nullptr;
    set_handover(h, d, other, f, !d.use_turns && d.nch == 1 && d.f_nw == d.ho_ppb && s.mode != kSweepVB);
#ifdef BNMTF_EXPERIMENTS
    if (d.use_wide && d.use_turns) launch_sweep_turns(s2, f, h->stream);
    else
#endif
    if (d.use_wide && !d.use_twin) launch_sweep_wide(s2, f, h->stream);
    else launch_sweep_fast(s2, f, h->stream);
    h->last_sweep_fast = true;
    if (d.f_gen_count == 0) return;
    s.unit_list = d.f_gen_units;           // the few units with more than kFastMaxSlots slots per lane
    s.n = d.f_gen_count;
  }
  launch_sweep(s, h->stream);
}
static SweepArgs sweep_args(bnmtf_model* h, Dir& d, const Dir& other, int mode, uint32_t stream_id) {
  SweepArgs s;
  memset(&s, 0, sizeof(s));
  s.min_x = mode == kSweepMode ? h->cur_min_x : 0.f;
  s.n = d.n; s.n0 = d.n0; s.K = d.W; s.KP = d.KP; s.mode = mode; s.cond_k = -1; s.qinit_only = 0; s.only_k = -1; s.vb_moments = 1; s.vb_stats = nullptr;
  s.col0 = h->col0;
  s.slabs = d.slabs; s.split = d.split; s.n_pad = d.n_pad; s.lambda = d.lambda;
  s.Xself = d.X; s.XselfT = nullptr; s.ldT_self = d.ldT;
  s.XoT = other.XT; s.ldT_o = other.ldT; s.C32 = other.C32;
  s.slot_ptr = d.slot_ptr; s.idx = d.idx; s.q = d.q;
  s.tau = h->tau_f;
  s.key0 = (uint32_t)h->seed; s.key1 = (uint32_t)(h->seed >> 32); s.it = (uint32_t)h->iteration; s.stream = stream_id;
  s.acc = nullptr;
  s.numer_out = d.numer; s.tau_out = d.taup;
  s.mu_self = d.mu; s.tau_self = d.tauq; s.var_self = d.var; s.S2self = d.S2; s.S2selfT = d.S2T;
  s.S2oT = other.S2T; s.colsum2_o = other.colsum2;
  return s;
}

static int upload_factor(bnmtf_model* h, Dir& d, const double* src) {
  std::vector<float> tmp((size_t)d.nglob * d.KP, 0.0f);
  for (int r = 0; r < d.nglob; ++r)
    for (int k = 0; k < d.W; ++k) tmp[(size_t)r * d.KP + k] = (float)src[(size_t)r * d.W + k];
  HIPCHK(hipMemcpyAsync(d.X, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  enqueue_post(h, d);
  return BNMTF_OK;
}
static int download_matrix(bnmtf_model* h, const float* dev, int rows, int W, int KP, double* dst) {
  std::vector<float> tmp((size_t)rows * KP);
  HIPCHK(hipMemcpyAsync(tmp.data(), dev, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int r = 0; r < rows; ++r)
    for (int k = 0; k < W; ++k) dst[(size_t)r * W + k] = (double)tmp[(size_t)r * KP + k];
  return BNMTF_OK;
}
static int set_tau(bnmtf_model* h, double tau) {
  const float tf = (float)tau;
  HIPCHK(hipMemcpyAsync(h->tau_d, &tau, sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tau_f, &tf, sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

static int bnmtf_alloc_extras(bnmtf_model* h, const double* lambdaS);
static int build_standard(bnmtf_model* h, const double* lambda_S, const uint8_t* comm_id);
static void describe_model(bnmtf_model* h);
static int small_build(bnmtf_model* h, const float* R, const uint8_t* M);
static void small_free(bnmtf_model* h);
static int ensure_std(bnmtf_model* h);

// ------------------------------------------------------------ sample hand-off
// run() hands every sample to the host (all_U[it], all_V[it]; bnmf_gibbs_optimised.py:146-148).  The factor is packed
// ([rows][KP] -> [rows][W]) into a device snapshot slot on the compute stream -- a few microseconds -- and the compute
// stream moves on to the next iteration; a copy stream takes the slot to the host behind it.  Caller buffers that are
// pinned (bnmtf_host_alloc, or registered by the caller) receive the copy directly, at PCIe rate and with no host work;
// pageable ones go through a pinned ring that the calling thread empties kDepth iterations behind the enqueue front.
struct SampleSink {
  // Slots are handed over in GROUPS of kGroup iterations: one event recorded on the compute stream and one stream wait per
  // group, not per iteration -- an event record drains the compute queue for a few microseconds each time (round 1: eight
  // records cost 30 us per iteration).  Two groups of slots: one being filled while the other goes to the host.
#ifndef BNMTF_SAMPLE_GROUP
#define BNMTF_SAMPLE_GROUP 8
#endif
  static constexpr int kGroup = BNMTF_SAMPLE_GROUP, kGroups = 2, kDepth = kGroup * kGroups;
  struct Mat { const float* src; int rows, W, KP; float* dst; size_t off; };
  bnmtf_model* h = nullptr;
  hipStream_t writer = nullptr;   // the stream whose kernels fill the slots: the compute stream, or the tail stream of bnmf_gibbs_run (TailOverlap)
  Mat m[3]; int nmat = 0;
  size_t per_it = 0;            // floats per iteration over all matrices
  bool active = false, direct = true;
  int n_iter = 0, group_first = 0, drained = 0;     // first iteration of the group being filled; ring path: iterations already in the caller's arrays
  int next_copy = 0;                                // first iteration whose slot has not been given to the copy stream yet
  int pending_last[kGroups] = {-1, -1};             // ring path: last iteration of the group whose copy is in flight in event slot g

  void add(const float* src, int rows, int W, int KP, float* dst) {
    if (!dst) return;
    m[nmat++] = Mat{src, rows, W, KP, dst, per_it};
    per_it += (size_t)rows * W;
  }
  static bool pinned(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
  }
  int begin(bnmtf_model* h_, int n_iter_, hipStream_t writer_ = nullptr) {
    h = h_; n_iter = n_iter_; next_copy = 0; writer = writer_ ? writer_ : h_->stream;
    if (nmat == 0) return BNMTF_OK;
    active = true;
    for (int i = 0; i < nmat; ++i) direct = direct && pinned(m[i].dst) && pinned(m[i].dst + (size_t)n_iter * m[i].rows * m[i].W - 1);
    if (getenv("BNMTF_SAMPLES_RING")) direct = false;       // test hook: force the pageable path
    if (!h->copy_stream) {
      HIPCHK(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
      for (int s = 0; s < kGroups; ++s) {
        HIPCHK(hipEventCreateWithFlags(&h->snap_ready[s], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->copy_done[s], hipEventDisableTiming));
      }
    }
    if (h->snap_dev_cap < per_it * kDepth) {
      dfree(h->snap_dev);
      CHK(dalloc(&h->snap_dev, per_it * kDepth, false));
      h->snap_dev_cap = per_it * kDepth;
    }
    if (!direct && h->snap_host_cap < per_it * kDepth) {
      if (h->snap_host) (void)hipHostFree(h->snap_host);
      h->snap_host = nullptr; h->snap_host_cap = 0;
      HIPCHK(hipHostMalloc((void**)&h->snap_host, per_it * kDepth * sizeof(float), hipHostMallocDefault));
      h->snap_host_cap = per_it * kDepth;
    }
    return BNMTF_OK;
  }
  // ring path: the group in event slot g has landed in the pinned ring -> the caller's arrays
  int drain_group(int g) {
    if (pending_last[g] < 0) return BNMTF_OK;
    HIPCHK(hipEventSynchronize(h->copy_done[g]));
    for (; drained <= pending_last[g]; ++drained) {
      const float* slot = h->snap_host + (size_t)(drained % kDepth) * per_it;
      for (int i = 0; i < nmat; ++i)
        memcpy(m[i].dst + (size_t)drained * m[i].rows * m[i].W, slot + m[i].off, (size_t)m[i].rows * m[i].W * sizeof(float));
    }
    pending_last[g] = -1;
    return BNMTF_OK;
  }
  // before iteration `it` is enqueued: at the start of a group its slots must have been taken to the host (the group two back)
  // (the wait goes to the stream that writes the slots)
  int open_slot(int it) {
    if (!active || it % kGroup != 0 || it < kDepth) return BNMTF_OK;
    const int g = (it / kGroup) % kGroups;
    if (!direct) CHK(drain_group(g));
    HIPCHK(hipStreamWaitEvent(writer, h->copy_done[g], 0));
    return BNMTF_OK;
  }
  // where matrix `src` goes in the slot of iteration `it` (the relayout kernel that follows its sweep writes it there), or null
  float* slot_for(int it, const float* src) const {
    if (!active) return nullptr;
    for (int i = 0; i < nmat; ++i)
      if (m[i].src == src) return h->snap_dev + (size_t)(it % kDepth) * per_it + m[i].off;
    return nullptr;
  }
  // matrix `src` is final for iteration `it`: pack it into the slot (writer stream)
  void snapshot(int it, const float* src) {
    if (!active) return;
    for (int i = 0; i < nmat; ++i)
      if (m[i].src == src) launch_compact_rows(src, m[i].rows, m[i].W, m[i].KP, h->snap_dev + (size_t)(it % kDepth) * per_it + m[i].off, writer);
  }
  // every matrix of iteration `it` is in its slot; at the end of a group the group goes to the copy stream -- and in the LAST group
  // of the run every iteration on its own: what is still to be copied when the last sweep has finished is then one iteration, not
  // four (16 MB at cfg3 = 0.6 ms behind the compute stream, 7 % of a 20-iteration call)
  int close_slot(int it) {
    if (!active) return BNMTF_OK;
    const bool last_group = it / kGroup == (n_iter - 1) / kGroup;
    if (it % kGroup != kGroup - 1 && it != n_iter - 1 && !last_group) return BNMTF_OK;
    const int first = next_copy, g = (it / kGroup) % kGroups;
    next_copy = it + 1;
    HIPCHK(hipEventRecord(h->snap_ready[g], writer));
    HIPCHK(hipStreamWaitEvent(h->copy_stream, h->snap_ready[g], 0));
#ifdef BNMTF_EXPERIMENT_SAMPLES_NOCOPY
    constexpr bool nocopy = true;      // measurement build only (wrong results): the hand-off without its copies
#else
    constexpr bool nocopy = false;
#endif
    for (int j = first; j <= it && !nocopy; ++j) {
      const float* slot = h->snap_dev + (size_t)(j % kDepth) * per_it;
      if (direct) {
        for (int i = 0; i < nmat; ++i)
          HIPCHK(hipMemcpyAsync(m[i].dst + (size_t)j * m[i].rows * m[i].W, slot + m[i].off, (size_t)m[i].rows * m[i].W * sizeof(float),
                                hipMemcpyDeviceToHost, h->copy_stream));
      } else {
        HIPCHK(hipMemcpyAsync(h->snap_host + (size_t)(j % kDepth) * per_it, slot, per_it * sizeof(float), hipMemcpyDeviceToHost, h->copy_stream));
      }
    }
    HIPCHK(hipEventRecord(h->copy_done[g], h->copy_stream));
    pending_last[g] = it;
    return BNMTF_OK;
  }
  int finish() {
    if (!active) return BNMTF_OK;
    HIPCHK(hipStreamSynchronize(h->copy_stream));
    if (!direct) {                                   // the groups still in the ring, oldest first
      const int g_last = ((n_iter - 1) / kGroup) % kGroups;
      CHK(drain_group((g_last + 1) % kGroups));
      CHK(drain_group(g_last));
    }
    active = false;
    return BNMTF_OK;
  }
  // an error return out of the iteration loop leaves copies in flight into the caller's arrays (or the ring): they are
  // waited for on EVERY way out, so nothing is written after run() has returned
  ~SampleSink() {
    if (active && h && h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  }
};

static int ensure_rec(bnmtf_model* h, size_t n) {
  if (h->rec_cap >= n) return BNMTF_OK;
  dfree(h->rec); dfree(h->gunit);
  CHK(dalloc(&h->rec, n * 5));
  CHK(dalloc(&h->gunit, n));
  h->rec_cap = n;
  return BNMTF_OK;
}
// Gamma(alpha_s, 1) variates of the next n iterations (tau = variate / beta_s): they depend on the seed and the iteration
// number only, so the fp64 Marsaglia-Tsang loop runs on the host, off the device's critical path.
static int stage_gamma_variates(bnmtf_model* h, int n) {
  h->gunit_host.resize((size_t)n);
  const double shape = h->alpha + 0.5 * h->n_obs;
  for (int it = 0; it < n; ++it)
    h->gunit_host[it] = gamma_unit_draw(shape, (uint32_t)(h->iteration + it), kStreamTau, (uint32_t)h->seed, (uint32_t)(h->seed >> 32));
  HIPCHK(hipMemcpyAsync(h->gunit, h->gunit_host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return BNMTF_OK;
}

// approx_expectation on the device: reset at the start of a run() call, add the sample of iteration `it` of that call
static int expectation_begin(bnmtf_model* h) {
  if (h->exp_burn < 0) return BNMTF_OK;
  if (!h->exp_rows) {
    CHK(dalloc(&h->exp_rows, (size_t)h->rows.xrows * h->rows.KP));
    CHK(dalloc(&h->exp_cols, (size_t)h->cols.xrows * h->cols.KP));
    CHK(dalloc(&h->exp_S, (size_t)std::max(h->K * h->L, 1)));
    CHK(dalloc(&h->exp_tau, 1));
  }
  HIPCHK(hipMemsetAsync(h->exp_rows, 0, sizeof(double) * h->rows.nglob * h->rows.KP, h->stream));
  HIPCHK(hipMemsetAsync(h->exp_cols, 0, sizeof(double) * h->cols.nglob * h->cols.KP, h->stream));
  HIPCHK(hipMemsetAsync(h->exp_S, 0, sizeof(double) * std::max(h->K * h->L, 1), h->stream));
  HIPCHK(hipMemsetAsync(h->exp_tau, 0, sizeof(double), h->stream));
  h->exp_count = 0;
  return BNMTF_OK;
}
static void expectation_add(bnmtf_model* h, int it, hipStream_t st = nullptr) {      // st: the stream of the iteration's finish kernel (null = the compute stream)
  if (h->exp_burn < 0 || it < h->exp_burn || (it - h->exp_burn) % h->exp_thin != 0) return;
  if (!st) st = h->stream;
  launch_accumulate(h->rows.X, (size_t)h->rows.nglob * h->rows.KP, h->exp_rows, h->tau_d, h->exp_tau, st);
  launch_accumulate(h->cols.X, (size_t)h->cols.nglob * h->cols.KP, h->exp_cols, nullptr, nullptr, st);
  if (h->L > 0) launch_accumulate(h->S, (size_t)h->K * h->L, h->exp_S, nullptr, nullptr, st);
  h->exp_count++;
}

}  // namespace bnmtf

#include "api_small.inc"

using namespace bnmtf;

#include "api_heldout.inc"

// ======================================================================= C ABI
extern "C" {

int bnmtf_version(void) { return 100; }
const char* bnmtf_last_error(void) { return g_err; }

int bnmtf_device_count(int* count) try {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { n = 0; (void)hipGetLastError(); }
  *count = n;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_comm_unique_id(uint8_t out[128]) { return comm_unique_id(out); }

int bnmtf_shard_range(int64_t n, int rank, int world, int64_t* first, int64_t* count) try {
  if (world < 1 || rank < 0 || rank >= world || n < 0) { set_error("bad shard request"); return BNMTF_EINVAL; }
  *first = n * rank / world;
  *count = n * (rank + 1) / world - *first;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_slot_layout(int n, int m, int KP, int world, const uint32_t* miss_ptr, const uint32_t* miss_idx, int64_t* info,
                      int32_t* unit_map, uint32_t* pair_E, uint32_t* pair_base, uint32_t* off, uint32_t* off16, int32_t* gen_units,
                      uint16_t* row_blk, int32_t* u_unit_map, uint32_t* u_pair_E, uint32_t* u_pair_base, uint32_t* u_off16) try {
  if (!miss_ptr || !info) { set_error("bnmtf_slot_layout: null argument"); return BNMTF_EINVAL; }
  if (n < 1 || m < 1 || (KP != 32 && KP != 64) || world < 1) { set_error("bnmtf_slot_layout: unsupported shape n=%d m=%d KP=%d world=%d (KP 32 or 64)", n, m, KP, world); return BNMTF_EINVAL; }
  if (miss_ptr[0] != 0) { set_error("bnmtf_slot_layout: miss_ptr[0] must be 0"); return BNMTF_EINVAL; }
  std::vector<MissingView> miss(n);
  for (int u = 0; u < n; ++u) {
    if (miss_ptr[u + 1] < miss_ptr[u] || miss_ptr[u + 1] - miss_ptr[u] > (uint32_t)m) { set_error("bnmtf_slot_layout: unit %d: bad list bounds", u); return BNMTF_EINVAL; }
    if (miss_ptr[u + 1] > miss_ptr[u] && !miss_idx) { set_error("bnmtf_slot_layout: null argument"); return BNMTF_EINVAL; }
    miss[u] = {miss_idx + miss_ptr[u], miss_ptr[u + 1] - miss_ptr[u]};
    for (uint32_t e = 0; e < miss[u].count; ++e)
      if (miss[u].idx[e] >= (uint32_t)m || (e && miss[u].idx[e] <= miss[u].idx[e - 1])) {
        set_error("bnmtf_slot_layout: unit %d: the missing indices must ascend and lie below m=%d (entry %u is %u)", u, m, e, miss[u].idx[e]);
        return BNMTF_EINVAL;
      }
  }
  SlotLayoutInput in;
  in.n = n; in.m = m; in.KP = KP; in.world = world; in.miss = miss.data(); in.sw = LayoutSwitches::from_env();
  SlotLayout L;
  build_slot_layout(in, L);
  const int64_t scalars[BNMTF_SLOT_INFO_LEN] = {
      L.mz, L.pw, L.nch, L.mh, L.pw_chunk, L.pw1, L.pair_ok, L.wide_can, L.use_wide, L.use_turns, L.use_twin, L.f_nw, L.vb_path, L.uw_ok, L.u_nw,
      L.ho_ppb, L.stats_blocks, L.npairs, L.emax, (int64_t)L.slots, L.u_emax,
      (int64_t)L.unit_map.size(), (int64_t)L.pair_E.size(), (int64_t)L.pair_base.size(), (int64_t)L.off.size(), (int64_t)L.off16.size(),
      (int64_t)L.gen_units.size(), (int64_t)L.row_blk.size(), (int64_t)L.u_unit_map.size(), (int64_t)L.u_pair_E.size(),
      (int64_t)L.u_pair_base.size(), (int64_t)L.u_off16.size()};
  memcpy(info, scalars, sizeof(scalars));
  auto put = [](auto* dst, const auto& src) { if (dst && !src.empty()) memcpy(dst, src.data(), src.size() * sizeof(src[0])); };
  put(unit_map, L.unit_map); put(pair_E, L.pair_E); put(pair_base, L.pair_base); put(off, L.off); put(off16, L.off16); put(gen_units, L.gen_units);
  put(row_blk, L.row_blk); put(u_unit_map, L.u_unit_map); put(u_pair_E, L.u_pair_E); put(u_pair_base, L.u_pair_base); put(u_off16, L.u_off16);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_create(const bnmtf_problem* p, bnmtf_handle* out) try {
  *out = nullptr;
  if (!p || !p->R || !p->M || !p->lambda_rows || !p->lambda_cols) { set_error("bnmtf_create: null argument"); return BNMTF_EINVAL; }
  if (p->I < 1 || p->J < 1 || p->K < 1 || p->K > BNMTF_MAX_RANK || p->L < 0 || p->L > BNMTF_MAX_RANK) {
    set_error("bnmtf_create: unsupported shape I=%d J=%d K=%d L=%d (1 <= K,L <= %d)", p->I, p->J, p->K, p->L, BNMTF_MAX_RANK);
    return BNMTF_EINVAL;
  }
  if (p->L > 0 && !p->lambda_S) { set_error("bnmtf_create: lambda_S required when L > 0"); return BNMTF_EINVAL; }
  if (p->world < 1 || p->rank < 0 || p->rank >= p->world) { set_error("bnmtf_create: bad rank/world %d/%d", p->rank, p->world); return BNMTF_EINVAL; }
  if (p->world > 1 && !p->comm_id) { set_error("bnmtf_create: comm_id required when world > 1"); return BNMTF_EINVAL; }
  if (p->world > p->I || p->world > p->J) { set_error("bnmtf_create: world %d larger than a matrix dimension", p->world); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(p->device));

  const auto t_create0 = std::chrono::steady_clock::now();
  bnmtf_model* h = new bnmtf_model();
  h->I = p->I; h->J = p->J; h->K = p->K; h->L = p->L;
  h->alpha = p->alpha; h->beta = p->beta; h->seed = p->seed;
  h->device = p->device; h->rank = p->rank; h->world = p->world;
  // BNMTF_TAIL=serial: bnmf_gibbs_run keeps every kernel on the compute stream, in program order (the A/B of TailOverlap, and what
  // tests/test_tail_overlap_gpu.py compares the two-stream order against, bit for bit); =overlap: the second stream whatever the
  // size.  Read once, here.
  if (const char* e = getenv("BNMTF_TAIL")) h->tail_mode = !strcmp(e, "serial") ? 2 : !strcmp(e, "overlap") ? 1 : 0;
  const int I = p->I, J = p->J;
  const float* R = p->R; const uint8_t* M = p->M;

  auto fail = [&](int rc) { bnmtf_destroy(h); return rc; };
  h->stream = device_pool().take_stream(p->device);
  if (!h->stream && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(BNMTF_EHIP); }

  // observed counts, training-mask constants (fp64) and the empty row/column check
  std::vector<uint32_t> rc(I, 0), cc(J, 0);
  double n_obs = 0, sR = 0, sR2 = 0;
  {
    constexpr int kRows = 64;                     // fixed chunks, combined in chunk order: the sums do not depend on the thread count
    const int nch = (I + kRows - 1) / kRows;
    std::vector<double> part((size_t)nch * 3, 0.0);
    std::vector<std::vector<uint32_t>> ccp(nch);
    parallel_chunks(I, kRows, [&](int a, int b) {
      const int ch = a / kRows;
      std::vector<uint32_t>& cl = ccp[ch];
      cl.assign(J, 0);
      double n = 0, s1 = 0, s2 = 0;
      for (int i = a; i < b; ++i) {
        uint32_t cnt = 0;
        for (int j = 0; j < J; ++j)
          if (M[(size_t)i * J + j]) {
            const double r = (double)R[(size_t)i * J + j];
            ++cnt; cl[j]++; s1 += r; s2 += r * r;
          }
        rc[i] = cnt; n += cnt;
      }
      part[(size_t)ch * 3] = n; part[(size_t)ch * 3 + 1] = s1; part[(size_t)ch * 3 + 2] = s2;
    });
    for (int ch = 0; ch < nch; ++ch) {
      n_obs += part[(size_t)ch * 3]; sR += part[(size_t)ch * 3 + 1]; sR2 += part[(size_t)ch * 3 + 2];
      for (int j = 0; j < J; ++j) cc[j] += ccp[ch][j];
    }
  }
  for (int i = 0; i < I; ++i) if (!rc[i]) { set_error("Fully unobserved row in R, row %d.", i); return fail(BNMTF_EINVAL); }
  for (int j = 0; j < J; ++j) if (!cc[j]) { set_error("Fully unobserved column in R, column %d.", j); return fail(BNMTF_EINVAL); }
  h->n_obs = n_obs; h->sumR = sR; h->sumR2 = sR2;

  CreateLaps laps;
  laps.t = t_create0;
  laps.lap("counts and sums over the mask");
  const int Wr = p->K, Wc = p->L > 0 ? p->L : p->K;
  int rcode;
  // the geometry every entry point may ask for, whichever path runs the model
  h->rows.nglob = I; h->rows.m = J; h->rows.W = Wr; h->rows.KP = Wr <= 32 ? 32 : 64;
  h->cols.nglob = J; h->cols.m = I; h->cols.W = Wc; h->cols.KP = Wc <= 32 ? 32 : 64;
  h->rows.obs_count = rc; h->cols.obs_count = cc;
  // Small models (kernel_small.hip: the whole run in one launch, one block per model) build only their own arena here -- ONE
  // allocation that also holds the full matrix, the mask and the scalars; the structures of the multi-launch path -- contraction
  // operands, slot layouts, Gram partials, ... -- are built the first time an entry point needs them (ensure_std).
  // BNMTF_SMALL=0: never.
  h->lam_rows.assign(p->lambda_rows, p->lambda_rows + (size_t)I * Wr);
  h->lam_cols.assign(p->lambda_cols, p->lambda_cols + (size_t)J * Wc);
  if (p->L > 0) h->lam_S.assign(p->lambda_S, p->lambda_S + (size_t)p->K * p->L);
  if (p->world == 1 && !getenv("BNMTF_FORCE_COMM")) {
    if ((rcode = small_build(h, R, M))) return fail(rcode);
  }
  if (!h->one_arena) {   // the full matrix and the training mask (predict / validation; the layout passes read them on the device); small scalars -- one allocation
    const size_t bR = ((size_t)I * J * sizeof(float) + 255) & ~(size_t)255, bM = ((size_t)I * J + 255) & ~(size_t)255;
    char* base = nullptr;
    if ((rcode = dalloc(&base, bR + bM + 256, false))) return fail(rcode);
    h->Rfull = reinterpret_cast<float*>(base); h->Mtrain = reinterpret_cast<uint8_t*>(base + bR);
    h->out6 = reinterpret_cast<double*>(base + bR + bM); h->tau_d = h->out6 + 8; h->acc = h->out6 + 12; h->tau_f = reinterpret_cast<float*>(h->out6 + 16);
    if (hipMemsetAsync(base + bR + bM, 0, 256, h->stream) != hipSuccess) { set_error("memset failed"); return fail(BNMTF_EHIP); }
  }
  if (hipMemcpyAsync(h->Rfull, R, (size_t)I * J * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess) { set_error("copy R failed"); return fail(BNMTF_EHIP); }
  if (hipMemcpyAsync(h->Mtrain, M, (size_t)I * J, hipMemcpyHostToDevice, h->stream) != hipSuccess) { set_error("copy M failed"); return fail(BNMTF_EHIP); }
  if (h->small) {
    if (hipStreamSynchronize(h->stream) != hipSuccess) { set_error("bnmtf_create: uploads failed"); return fail(BNMTF_EHIP); }    // (R, M are the caller's)
    h->std_built = false;
    laps.lap("small-model arena");
  } else {
    if ((rcode = build_standard(h, p->lambda_S, p->comm_id))) return fail(rcode);
  }
  h->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create0).count();
  describe_model(h);
  *out = h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD
}  // extern "C"

namespace bnmtf {
// The multi-launch path's part of a handle: both directions' contraction operands and slot layouts, factor buffers, the BNMTF
// extras, the communicator, the q hand-over tables.  Called by bnmtf_create, or -- for a model that started on the small path --
// by the first entry point that needs it.
static int build_standard(bnmtf_model* h, const double* lambda_S, const uint8_t* comm_id) {
  const auto t_create0 = std::chrono::steady_clock::now();
  const int I = h->I, J = h->J;
  const int Wr = h->K, Wc = h->L > 0 ? h->L : h->K;
  CreateLaps laps;
  int rcode;
  const std::vector<uint32_t> rc = h->rows.obs_count, cc = h->cols.obs_count;
  rcode = build_dir(h->rows, I, J, Wr, h->rank, h->world, h->lam_rows.data(), h->Rfull, h->Mtrain, I, J, true, rc, h->stream);
  if (rcode) return rcode;
  rcode = build_dir(h->cols, J, I, Wc, h->rank, h->world, h->lam_cols.data(), h->Rfull, h->Mtrain, I, J, false, cc, h->stream);
  if (rcode) return rcode;
  laps.lap("both directions built (total)");
  h->rows.obs_count = rc; h->cols.obs_count = cc;
  if ((rcode = alloc_factor(h->rows, h->cols.inner_pad))) return rcode;
  if ((rcode = alloc_factor(h->cols, h->rows.inner_pad))) return rcode;

  laps.lap("factor buffers");
  if (!h->Ad && (rcode = dalloc(&h->Ad, (size_t)I * 64))) return rcode;
  if (!h->Bd && (rcode = dalloc(&h->Bd, (size_t)J * 64))) return rcode;
  if (h->L > 0 && (rcode = dalloc(&h->S, (size_t)h->K * h->L))) return rcode;
  if (h->L > 0 && (rcode = bnmtf_alloc_extras(h, lambda_S))) return rcode;

  if (h->world > 1) {
    if ((rcode = comm_create(&h->comm, comm_id, h->rank, h->world, h->stream))) return rcode;
    // every rank must hold the same Philox key (same draws, same tau variates): compare through the communicator
    const double mine[4] = {(double)(uint32_t)h->seed, (double)(uint32_t)(h->seed >> 32), -(double)(uint32_t)h->seed, -(double)(uint32_t)(h->seed >> 32)};
    double got[4];
    if (hipMemcpy(h->acc, mine, sizeof(mine), hipMemcpyHostToDevice) != hipSuccess) { set_error("seed check: copy failed"); return BNMTF_EHIP; }
    if ((rcode = comm_allreduce_max(h->comm, h->acc, 4, h->stream))) return rcode;
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipMemcpy(got, h->acc, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) { set_error("seed check: copy failed"); return BNMTF_EHIP; }
    (void)hipMemset(h->acc, 0, 4 * sizeof(double));
    if (memcmp(mine, got, sizeof(mine)) != 0) {
      set_error("bnmtf_create: the ranks were given different seeds (this rank %llu): a sharded model needs one shared seed", (unsigned long long)h->seed);
      return BNMTF_EINVAL;
    }
  } else if (getenv("BNMTF_FORCE_COMM")) {     // test hook: run the RCCL exchange path with a 1-rank communicator
    uint8_t id[128];
    if ((rcode = comm_unique_id(id))) return rcode;
    if ((rcode = comm_create(&h->comm, id, 0, 1, h->stream))) return rcode;
  }

  // q hand-over tables (BNMF on one GPU, both directions on the 16-wave or the plain 8-wave kernel).  By default only for
  // problems of >= 64 blocks per direction: below that the sweep is launch-bound and the pre-pass costs next to nothing.
  // BNMTF_HANDOVER=0: never; =1: whenever the tables can be built.
  {
    const char* e = getenv("BNMTF_HANDOVER");
    auto blocks = [](const Dir& d) { return d.ho_ppb > 0 ? d.f_npairs / d.ho_ppb : 0; };
    const bool want = h->L == 0 && !h->comm && (e ? atoi(e) != 0 : std::min(blocks(h->rows), blocks(h->cols)) >= 64);
    const auto t_ho0 = std::chrono::steady_clock::now();
    if (want && build_handover(h, h->rows, h->cols) && build_handover(h, h->cols, h->rows)) h->rows.ho_ready = h->cols.ho_ready = h->ho_enabled = true;
    if (const char* r = getenv("BNMTF_HANDOVER_REFRESH")) h->ho_refresh = (uint64_t)std::max(1, atoi(r));
    if (const char* u = getenv("BNMTF_UNIT")) h->uw_force = atoi(u) == 1;      // A/B switch: the unit-per-wave shape also where q could be handed over
    if (getenv("BNMTF_CREATE_TIMING")) fprintf(stderr, "hand-over tables: %.1f ms (create so far %.1f ms)\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ho0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create0).count());
  }
  h->std_built = true;
  h->create_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create0).count();
  return BNMTF_OK;
}
static void describe_model(bnmtf_model* h) {
  const int I = h->I, J = h->J;
  const double n_obs = h->n_obs;
  char buf[1024];
  snprintf(buf, sizeof(buf),
           "I=%d J=%d K=%d L=%d rank=%d/%d rows[n=%d n_pad=%d split=%d ipw=%d inner_pad=%d nmiss=%zu nslots=%zu sweep_nw=%d turns=%d twin=%d handover=%d emax=%d generic_units=%d] "
           "cols[n=%d n_pad=%d split=%d ipw=%d inner_pad=%d nmiss=%zu nslots=%zu sweep_nw=%d turns=%d emax=%d generic_units=%d] n_obs=%.0f create_ms=%.0f",
           I, J, h->K, h->L, h->rank, h->world, h->rows.n, h->rows.n_pad, h->rows.split, h->rows.ipw, h->rows.inner_pad,
           h->rows.nmiss, h->rows.nslots, h->rows.f_nw, (int)h->rows.use_turns, (int)h->rows.use_twin, (int)h->ho_enabled, h->rows.f_emax, h->rows.f_gen_count, h->cols.n, h->cols.n_pad, h->cols.split,
           h->cols.ipw, h->cols.inner_pad, h->cols.nmiss, h->cols.nslots, h->cols.f_nw, (int)h->cols.use_turns, h->cols.f_emax, h->cols.f_gen_count, n_obs, h->create_ms);
  h->description = buf;
  // which directions run the unit-per-wave sweep (kernel_sweep_unit.hip), its unit waves per block and most slots per lane
  snprintf(buf, sizeof(buf), " unit_sweep[rows=%d/%d/%d cols=%d/%d/%d]", (int)(h->rows.uw_ok && (!h->ho_enabled || h->uw_force)), h->rows.u_nw, h->rows.u_emax,
           (int)(h->cols.uw_ok && (!h->ho_enabled || h->uw_force)), h->cols.u_nw, h->cols.u_emax);
  h->description += buf;
  // bnmf_gibbs_run's relayout / Gram / finish kernels: beside the contractions on a second stream, or in program order (BNMTF_TAIL)
  h->description += tail_overlap_wanted(h) ? " tail=overlap" : " tail=serial";
  if (h->tail_mode == 0) h->description += "(auto)";
  if (h->small) {
    snprintf(buf, sizeof(buf), " small[block=%d entry_threads=%d/%d slots=%d/%d lds=%zu std_built=%d]", h->small->nt, h->small->dev.rows.nthreads, h->small->dev.cols.nthreads,
             h->small->dev.rows.em, h->small->dev.cols.em, h->small->lds_bytes, (int)h->std_built);
    h->description += buf;
  }
  if (h->L > 0 && h->std_built) {
    // the dense S system (kernel_ssys.hip): its GEMM's column ranges and the blocks of b -- or the per-row path (on=0)
    if (h->ssys) snprintf(buf, sizeof(buf), " ssys[on=1 nsplit=%d range=%d bblocks=%d]", h->ss_nsplit, ssys_gemm_range(h->cols.n, h->ss_nsplit), ssys_b_blocks(h->cols.n));
    else snprintf(buf, sizeof(buf), " ssys[on=0]");
    h->description += buf;
  }
}

// the metric kernel's per-tile partial sums (launch_metric_sums): one buffer per handle, sized by its I x J
static int metric_partials(bnmtf_model* h, double** out) {
  if (!h->metric_part) CHK(dalloc(&h->metric_part, metric_tiles(h->I, h->J) * 8, false));
  *out = h->metric_part;
  return BNMTF_OK;
}
}  // namespace bnmtf
extern "C" {

int bnmtf_destroy(bnmtf_handle h) try {
  if (!h) return BNMTF_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->comm) comm_destroy(h->comm);
  np_free(h);
  obs_free(h);
  heldout_free(h);
  small_free(h);            // (first: a small model's arena also holds Rfull, the posterior sums, Ad / Bd -- their pointers are cleared)
  free_dir(h->rows); free_dir(h->cols); free_dir(h->reff); free_dir(h->ceff);
  dfree(h->slabsS); dfree(h->CfS); dfree(h->deltaS); dfree(h->s_partial); dfree(h->s_w); dfree(h->s_omp); dfree(h->lambdaS); dfree(h->s_numer); dfree(h->s_taup);
  dfree(h->exp_rows); dfree(h->exp_cols); dfree(h->exp_S); dfree(h->exp_tau);
  dfree(h->muS); dfree(h->tauS); dfree(h->varS); dfree(h->mv_rows); dfree(h->mv_cols); dfree(h->tri_order); dfree(h->tri_sums); dfree(h->tri_third); dfree(h->ss_Aperm);
  dfree(h->ss_Wc); dfree(h->ss_Gc); dfree(h->ss_cands); dfree(h->ss_slabs); dfree(h->ss_AB); dfree(h->ss_r); dfree(h->ss_bpart); dfree(h->ss_tinv); dfree(h->ss_rec);
  dfree(h->Rfull); h->Mtrain = nullptr; h->out6 = nullptr; h->tau_d = nullptr; h->tau_f = nullptr; h->acc = nullptr;   // (one allocation: bnmtf_create)
  dfree(h->Mscratch); dfree(h->Ad); dfree(h->Bd); dfree(h->AdW); dfree(h->BdW); dfree(h->metric_part);
  dfree(h->A2d); dfree(h->B2d); dfree(h->vb_rec); dfree(h->vbred);
  dfree(h->rec); dfree(h->gunit); dfree(h->S);
  for (auto& pe : h->pending_events) { (void)hipEventDestroy(pe.second.first); (void)hipEventDestroy(pe.second.second); }
  for (auto e : h->event_pool) (void)hipEventDestroy(e);
  if (h->copy_stream) {
    (void)hipStreamSynchronize(h->copy_stream);
    for (int s2 = 0; s2 < 8; ++s2) { if (h->snap_ready[s2]) (void)hipEventDestroy(h->snap_ready[s2]); if (h->copy_done[s2]) (void)hipEventDestroy(h->copy_done[s2]); }
    (void)hipStreamDestroy(h->copy_stream);
  }
  dfree(h->snap_dev);
  if (h->snap_host) (void)hipHostFree(h->snap_host);
  if (h->xchg_stream) { (void)hipStreamSynchronize(h->xchg_stream); (void)hipStreamDestroy(h->xchg_stream); }
  if (h->tail_stream) { (void)hipStreamSynchronize(h->tail_stream); (void)hipStreamDestroy(h->tail_stream); }
  for (hipEvent_t e : h->ev_tail) if (e) (void)hipEventDestroy(e);
  if (h->aux_stream) { (void)hipStreamSynchronize(h->aux_stream); (void)hipStreamDestroy(h->aux_stream); }
  if (h->ev_aux0) (void)hipEventDestroy(h->ev_aux0);
  if (h->ev_aux1) (void)hipEventDestroy(h->ev_aux1);
  if (h->stream && !(h->pool_stream && device_pool().give_stream(h->device, h->stream))) (void)hipStreamDestroy(h->stream);
  delete h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_sync(bnmtf_handle h) try {
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_handover_dump(bnmtf_handle h, int which, int64_t* info, uint32_t* t_in, uint32_t* t_out, uint32_t* pk, uint32_t* region_ofs,
                        float* region) try {
  CHK(refuse_obs(h, "bnmtf_handover_dump"));
  if (!info || which < 0 || which > 1) { set_error("bnmtf_handover_dump: null info or which=%d (0 rows, 1 cols)", which); return BNMTF_EINVAL; }
  if (!h->ho_enabled) { set_error("bnmtf_handover_dump: the handle has no hand-over tables"); return BNMTF_ESTATE; }
  const Dir& d = which ? h->cols : h->rows;
  const Dir& o = which ? h->rows : h->cols;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  uint32_t total = 0;
  HIPCHK(hipMemcpy(&total, d.ho_region_ofs + d.ho_blocks, sizeof(total), hipMemcpyDeviceToHost));
  const size_t words = ((d.f_slots + 1) / 2) * 64, n_pk = (size_t)d.ho_blocks * o.ho_blocks * 3, n_ofs = (size_t)d.ho_blocks + 1, n_region = (size_t)total + 256;
  const int64_t scalars[BNMTF_HANDOVER_INFO_LEN] = {d.ho_blocks, o.ho_blocks, d.ho_lds_floats, d.ho_ppb, d.ho_filled, h->ho_regions_current,
                                                     (int64_t)words, (int64_t)words, (int64_t)n_pk, (int64_t)n_ofs, (int64_t)n_region};
  memcpy(info, scalars, sizeof(scalars));
  if (t_in && words) HIPCHK(hipMemcpy(t_in, d.ho_in, words * 4, hipMemcpyDeviceToHost));
  if (t_out && words) HIPCHK(hipMemcpy(t_out, d.ho_out, words * 4, hipMemcpyDeviceToHost));
  if (pk) HIPCHK(hipMemcpy(pk, d.ho_pk, n_pk * 4, hipMemcpyDeviceToHost));
  if (region_ofs) HIPCHK(hipMemcpy(region_ofs, d.ho_region_ofs, n_ofs * 4, hipMemcpyDeviceToHost));
  if (region) HIPCHK(hipMemcpy(region, d.ho_region, n_region * 4, hipMemcpyDeviceToHost));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_post_dump(bnmtf_handle h, int which, int64_t* info, float* X, float* S2, float* XT, float* XT2, float* S2T, float* XS,
                    double* C64, float* C32, double* colsum, double* colsum2) try {
  if (!h || h->obs || h->np) { set_error("bnmtf_post_dump: the handle has no dense-layout factor buffers (layout='observed' or bnmtf_np_create)"); return BNMTF_ESTATE; }
  if (!info || which < 0 || which > 1) { set_error("bnmtf_post_dump: null info or which=%d (0 rows, 1 cols)", which); return BNMTF_EINVAL; }
  if (!h->std_built || (h->small && h->small_cur && !h->std_cur)) {
    set_error("bnmtf_post_dump: the state lives on the one-launch small path, which has no relayout or Gram buffers");
    return BNMTF_ESTATE;
  }
  const Dir& d = which ? h->cols : h->rows;
  if (!d.X || !d.XT || !d.XT2 || !d.C64 || !d.C32 || !d.colsum) { set_error("bnmtf_post_dump: the handle has no relayout or Gram buffers"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->tail_stream) HIPCHK(hipStreamSynchronize(h->tail_stream));
  if (h->xchg_stream) HIPCHK(hipStreamSynchronize(h->xchg_stream));
  if (d.gram_pending && d.ev_gram_all) HIPCHK(hipEventSynchronize(d.ev_gram_all));      // (what await_gram waits for; the flag stays)
  // which of its buffers the last variational relayout wrote: enqueue_post's rule
  const bool vb = (h->vb_ready || h->tri_ready) && d.S2 && d.S2T && d.colsum2;
  const bool chip = vb && vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows);
  const bool xs = vb && d.XS && !chip, umax = vb && chip && d.xb_umax_posted;
  const size_t nx = (size_t)d.nglob * d.KP, nt = (size_t)d.KP * d.ldT, nc = (size_t)d.KP * d.KP;
  const int64_t scalars[BNMTF_POST_INFO_LEN] = {d.nglob, d.KP, d.W, d.ldT, post_blocks(d.nglob), vb, xs, umax, d.n0, d.n,
                                                 (int64_t)nx, (int64_t)(vb ? nx : 0), (int64_t)nt, (int64_t)nt, (int64_t)(vb ? nt : 0), (int64_t)(xs ? 2 * nt : 0),
                                                 (int64_t)nc, (int64_t)nc, d.KP, vb ? d.KP : 0};
  memcpy(info, scalars, sizeof(scalars));
  if (X) HIPCHK(hipMemcpy(X, d.X, nx * sizeof(float), hipMemcpyDeviceToHost));
  if (S2 && vb) HIPCHK(hipMemcpy(S2, d.S2, nx * sizeof(float), hipMemcpyDeviceToHost));
  if (XT) HIPCHK(hipMemcpy(XT, d.XT, nt * sizeof(float), hipMemcpyDeviceToHost));
  if (XT2) HIPCHK(hipMemcpy(XT2, d.XT2, nt * sizeof(float), hipMemcpyDeviceToHost));
  if (S2T && vb) HIPCHK(hipMemcpy(S2T, d.S2T, nt * sizeof(float), hipMemcpyDeviceToHost));
  if (XS && xs) HIPCHK(hipMemcpy(XS, d.XS, 2 * nt * sizeof(float), hipMemcpyDeviceToHost));
  if (C64) HIPCHK(hipMemcpy(C64, d.C64, nc * sizeof(double), hipMemcpyDeviceToHost));
  if (C32) HIPCHK(hipMemcpy(C32, d.C32, nc * sizeof(float), hipMemcpyDeviceToHost));
  if (colsum) HIPCHK(hipMemcpy(colsum, d.colsum, d.KP * sizeof(double), hipMemcpyDeviceToHost));
  if (colsum2 && vb) HIPCHK(hipMemcpy(colsum2, d.colsum2, d.KP * sizeof(double), hipMemcpyDeviceToHost));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_omega_counts(bnmtf_handle h, uint64_t* total, uint32_t* row, uint32_t* col) try {
  CHK(refuse_obs(h, "bnmtf_omega_counts"));
  if (total) *total = (uint64_t)h->n_obs;
  if (row) memcpy(row, h->rows.obs_count.data(), sizeof(uint32_t) * h->I);
  if (col) memcpy(col, h->cols.obs_count.data(), sizeof(uint32_t) * h->J);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_host_alloc(size_t bytes, void** out) try {
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();        // the caller falls back to pageable memory: the next call must not find this error waiting
    *out = nullptr;
    set_error("hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return BNMTF_EHIP;
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_host_free(void* p) try {
  if (p) HIPCHK(hipHostFree(p));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_set_expectation(bnmtf_handle h, int burn_in, int thinning) try {
  CHK(refuse_obs(h, "bnmtf_set_expectation"));
  if (burn_in >= 0 && thinning < 1) { set_error("thinning must be >= 1"); return BNMTF_EINVAL; }
  h->exp_burn = burn_in; h->exp_thin = thinning < 1 ? 1 : thinning;
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_get_expectation(bnmtf_handle h, double* A, double* S, double* B, double* tau, uint64_t* count) try {
  CHK(refuse_obs(h, "bnmtf_get_expectation"));
  if (!h->exp_rows || h->exp_count == 0) { set_error("no samples accumulated (bnmtf_set_expectation before run, burn_in < iterations)"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const double inv = 1.0 / (double)h->exp_count;
  auto fetch = [&](const double* dev, int rows, int W, int KP, double* dst) -> int {
    std::vector<double> tmp((size_t)rows * KP);
    HIPCHK(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r) for (int k = 0; k < W; ++k) dst[(size_t)r * W + k] = tmp[(size_t)r * KP + k] * inv;
    return BNMTF_OK;
  };
  if (A) CHK(fetch(h->exp_rows, h->I, h->rows.W, h->rows.KP, A));
  if (B) CHK(fetch(h->exp_cols, h->J, h->cols.W, h->cols.KP, B));
  if (S && h->L > 0) CHK(fetch(h->exp_S, h->K, h->L, h->L, S));
  if (tau) { double t; HIPCHK(hipMemcpy(&t, h->exp_tau, sizeof(double), hipMemcpyDeviceToHost)); *tau = t * inv; }
  if (count) *count = h->exp_count;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_set_iteration(bnmtf_handle h, uint64_t it) { h->iteration = it; return BNMTF_OK; }
int bnmtf_set_tau(bnmtf_handle h, double tau) try {        // the noise precision alone (the factors on the device stay as they are)
  CHK(refuse_obs(h, "bnmtf_set_tau"));
  if (!h->have_state) { set_error("bnmtf_set_tau before the state is set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return set_tau(h, tau);
} BNMTF_ABI_GUARD
int bnmtf_get_iteration(bnmtf_handle h, uint64_t* it) { *it = h->iteration; return BNMTF_OK; }

int bnmtf_set_minimum_tn(bnmtf_handle h, double minimum_TN) try {
  if (!(minimum_TN >= 0.0)) { set_error("minimum_TN must be >= 0"); return BNMTF_EINVAL; }
  h->min_tn = minimum_TN;
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_set_profiling(bnmtf_handle h, int enable) try {
  CHK(refuse_obs(h, "bnmtf_set_profiling"));
  // 0: off; 1: every kernel; 2 + k: kernel k only (so that a timed region carries two event records, not eight)
  h->profiling = enable == 0 ? 0u : (enable == 1 ? 0xFFFFFFFFu : 1u << (unsigned)((enable - 2) & 31));
  h->profile_stride = enable >= 2 ? (uint64_t)((enable - 2) >> 5) + 1 : 1;     // every n-th iteration only: an event record costs the queue a few microseconds
  for (int i = 0; i < BNMTF_KERNEL_COUNT; ++i) { h->kernel_ms[i] = 0; h->kernel_launches[i] = 0; }
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_set_sweep_path(bnmtf_handle h, int fast) { CHK(refuse_obs(h, "bnmtf_set_sweep_path")); h->use_fast = fast != 0; h->ho_regions_current = false; return BNMTF_OK; }
int bnmtf_comm_info(bnmtf_handle h, int* kind, int* ranks) { return comm_info(h->comm, kind, ranks); }
int bnmtf_has_experiments(void) try {
#ifdef BNMTF_EXPERIMENTS
  return 1;
#else
  return 0;
#endif
} BNMTF_ABI_GUARD
int bnmtf_set_small_path(bnmtf_handle h, int mode) try {
  CHK(refuse_obs(h, "bnmtf_set_small_path"));
  if (mode < 0 || mode > 2) { set_error("bnmtf_set_small_path: mode 0 (never), 1 (auto) or 2 (always)"); return BNMTF_EINVAL; }
  h->small_mode = mode;
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_is_small(bnmtf_handle h, int* out) { CHK(refuse_obs(h, "bnmtf_is_small")); *out = small_wanted(h) ? 1 : 0; return BNMTF_OK; }
int bnmtf_kernel_stats(bnmtf_handle h, int kernel, double* total_ms, uint64_t* launches) try {
  CHK(refuse_obs(h, "bnmtf_kernel_stats"));
  if (kernel < 0 || kernel >= BNMTF_KERNEL_COUNT) { set_error("bad kernel id"); return BNMTF_EINVAL; }
  HIPCHK(hipStreamSynchronize(h->stream));
  drain_events(h);
  *total_ms = h->kernel_ms[kernel]; *launches = h->kernel_launches[kernel];
  return BNMTF_OK;
} BNMTF_ABI_GUARD
int bnmtf_describe(bnmtf_handle h, char* buf, size_t buflen) try {
  // (+ which kernels the last variational half sweep ran on: vb_chip_ok)
  static const char* const kVbPath[] = {"", " vb_sweep=generic", " vb_sweep=pairs", " vb_sweep=masked"};
  static const char* const kTriPath[] = {"", " tri_vb_sweeps=generic", " tri_vb_sweeps=pairs+cov", ""};      // (bnmtf_vb_run: api_trivb.inc enqueue_tri_sweep)
  // (+ the held-out mask's entries, bnmtf_set_heldout; a model of the one-launch kind runs the multi-launch path while it has one)
  char held[64] = "";
  if (h->held_n) snprintf(held, sizeof(held), " heldout=%zu%s", h->held_n, h->small ? " run_path=multi-launch" : "");
  // (+ the masked product's inner slices and a slice's inner rows, per direction, once a variational model has built them:
  // ensure_vb in api_models.inc, kernel_maskgemm.hip)
  char mprod[96] = "";
  if (h->vb_ready && h->rows.mslabs && h->cols.mslabs)
    snprintf(mprod, sizeof(mprod), " masked_product[row_units=%d/%d col_units=%d/%d]", h->rows.msplit, h->rows.mipw, h->cols.msplit, h->cols.mipw);
  snprintf(buf, buflen, "%s%s%s%s%s", h->description.c_str(), kVbPath[h->last_vb_path & 3], kTriPath[h->last_tri_path & 3], held, mprod);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// ------------------------------------------------------------------ BNMF Gibbs
int bnmf_set_state(bnmtf_handle h, const double* U, const double* V, double tau) try {
  CHK(refuse_obs(h, "bnmf_set_state"));
  if (h->L != 0) { set_error("bnmf_set_state on a BNMTF handle"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  h->std_cur = false; h->small_cur = false;
  if (h->std_built) {
    CHK(upload_factor(h, h->rows, U));
    CHK(upload_factor(h, h->cols, V));
    h->std_cur = true;
  }
  if (h->small) CHK(small_upload_state(h, U, V));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->ho_regions_current = false;          // (q hand-over: whatever the regions hold belongs to the state that was just replaced)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_get_state(bnmtf_handle h, double* U, double* V, double* tau) try {
  CHK(refuse_obs(h, "bnmf_get_state"));
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  if (h->small && h->small_cur) CHK(small_download_state(h, U, V));
  else {
    if (U) CHK(download_matrix(h, h->rows.X, h->I, h->rows.W, h->rows.KP, U));
    if (V) CHK(download_matrix(h, h->cols.X, h->J, h->cols.W, h->cols.KP, V));
  }
  if (tau) {
    HIPCHK(hipMemcpyAsync(tau, h->tau_d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_cond_params(bnmtf_handle h, int which, int k, double* numer_out, double* tau_out) try {
  CHK(refuse_obs(h, "bnmf_cond_params"));
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  if (h->world != 1) { set_error("cond_params is a single-GPU test hook"); return BNMTF_EINVAL; }
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  if (k < 0 || k >= d.W) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));
  enqueue_gemm(h, d, o, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
  SweepArgs s = sweep_args(h, d, o, kSweepDraw, which == 0 ? kStreamRows : kStreamCols);
  s.cond_k = k;
  enqueue_sweep(h, d, o, s, false);
  HIPCHK(hipMemcpyAsync(numer_out, d.numer, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tau_out, d.taup, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_gibbs_run(bnmtf_handle h, int n_iter, int update, float* U_out, float* V_out,
                   double* tau_out, double* perf_out, double* times_out) try {
  CHK(refuse_obs(h, "bnmf_gibbs_run"));
  if (h->L != 0) { set_error("bnmf_gibbs_run on a BNMTF handle"); return BNMTF_ESTATE; }
  if (!h->have_state) { set_error("bnmf_gibbs_run before bnmf_set_state"); return BNMTF_ESTATE; }
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  HIPCHK(hipSetDevice(h->device));
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  CHK(heldout_begin(h, n_iter));
  if (small_wanted(h)) {                       // a small model: the whole call is one launch (kernel_small.hip)
    SmallOut o{U_out, V_out, tau_out, perf_out, times_out};
    return small_run_many(&h, 1, n_iter, update, &o);
  }
  CHK(ensure_std(h));
  h->std_cur = true; h->small_cur = false;
  CHK(ensure_rec(h, (size_t)n_iter));
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  Dir& r = h->rows; Dir& c = h->cols;
  if (mode == kSweepDraw) CHK(stage_gamma_variates(h, n_iter));
  // q hand-over between the half sweeps: from this call's first rows sweep (a pre-pass) on; off again when the call returns
  HandoverScope ho_scope{h};
  // the [3] accumulator is only written by the generic sweep kernel (and summed across ranks): zero once, reset when used
  const bool acc_used = h->comm != nullptr || !h->use_fast || !c.fast_ok || c.f_gen_count > 0 || !(c.nch == 2 || sweep_fast_supported(c.KP, c.pw));
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  TailOverlap tail;
  CHK(tail.begin(h));
  hipStream_t const tst = tail.stream();         // where the relayouts, the Grams and the end of the iteration go (TailOverlap)
  SampleSink sink;
  sink.add(r.X, h->I, r.W, r.KP, U_out);
  sink.add(c.X, h->J, c.W, c.KP, V_out);
  CHK(sink.begin(h, n_iter, tst));
  CHK(expectation_begin(h));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));

  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    // ---- U columns: P = R~ . V, then the K sequential row-wise updates
    if (!r.gemm_ahead) enqueue_gemm(h, r, c, BNMTF_KERNEL_GEMM_ROWS);      // (several GPUs: launched inside the previous iteration's exchange of V)
    r.gemm_ahead = false;
    CHK(await_gram(h, c));                       // V^T V of the previous iteration's exchange
    CHK(tail.join(1));                           // V's layouts and Gram, tau: the previous iteration's tail, which ran beside the contraction above
    {
      ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_ROWS);
      SweepArgs s = sweep_args(h, r, c, mode, kStreamRows);
      enqueue_sweep(h, r, c, s, false);
    }
#ifdef BNMTF_EXPERIMENTS
    static const bool snap_compact = getenv("BNMTF_SNAP_COMPACT") != nullptr;      // A/B switch: the packing kernel of round 2
#else
    constexpr bool snap_compact = false;
#endif
    if (!snap_compact) r.snap_dst = sink.slot_for(it, r.X);         // the sample of U goes out with the relayout (no packing kernel of its own)
    if (tail.on) {                                                 // one GPU: relayout + Gram beside the contraction below
      CHK(tail.fork(0));
      enqueue_post(h, r, false, tst);
      CHK(tail.done(0));
    } else CHK(exchange_factor(h, r, &c, BNMTF_KERNEL_GEMM_COLS)); // one GPU (BNMTF_TAIL=serial): relayout + Gram; several: see exchange_factor
    if (snap_compact) sink.snapshot(it, r.X);
    // ---- V columns: Pv = R~^T . U
    if (!c.gemm_ahead) enqueue_gemm(h, c, r, BNMTF_KERNEL_GEMM_COLS);
    c.gemm_ahead = false;
    if (acc_used && it > 0) HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
    CHK(await_gram(h, r));
    CHK(tail.join(0));
    {
      ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_COLS);
      SweepArgs s = sweep_args(h, c, r, mode, kStreamCols);
      s.acc = h->acc;
      enqueue_sweep(h, c, r, s, true);
    }
    const bool fast_stats = h->last_sweep_fast;
    if (h->comm && fast_stats) launch_sum_stats(c.stats, c.stats_blocks, h->acc, h->stream);   // fold the slab before the exchange
    if (!snap_compact) c.snap_dst = sink.slot_for(it, c.X);
    if (tail.on) {
      CHK(tail.fork(1));
      enqueue_post(h, c, false, tst);
    } else CHK(exchange_factor(h, c, it + 1 < n_iter ? &r : nullptr, BNMTF_KERNEL_GEMM_ROWS));
    if (snap_compact) sink.snapshot(it, c.X);
    if (h->comm) {
      // the three sums of the SSE identity: behind the Gram on the exchange stream (its event covers the fold above)
      if (h->xchg_stream) {
        CHK(comm_allreduce_sum(h->comm, h->acc, 4, h->xchg_stream));
        HIPCHK(hipEventRecord(c.ev_gram_all, h->xchg_stream));
      } else CHK(comm_allreduce_sum(h->comm, h->acc, 4, h->stream));       // (BNMTF_EXCHANGE=serial)
    }
    CHK(sink.close_slot(it));
    CHK(await_gram(h, c)); CHK(await_gram(h, r));
    // ---- tau and the metrics of this sample
    FinishArgs f;
    f.copy_src = nullptr; f.copy_dst = nullptr; f.copy_n = 0;
    f.Cr64 = r.C64; f.Cc64 = c.C64; f.sr = r.colsum; f.sc = c.colsum; f.KP = r.KP;
    f.acc = h->acc; f.stats = (fast_stats && !h->comm) ? c.stats : nullptr; f.nstats = (fast_stats && !h->comm) ? c.stats_blocks : 0;
    f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2;
    f.alpha = h->alpha; f.beta = h->beta; f.update = update;
    f.key0 = (uint32_t)h->seed; f.key1 = (uint32_t)(h->seed >> 32); f.it = (uint32_t)h->iteration;
    f.gunit = mode == kSweepDraw ? h->gunit + it : nullptr;
    f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->rec + (size_t)it * 5;
    launch_finish(f, tst);
    expectation_add(h, it, tst);
    heldout_enqueue(h, it, tst);                 // (a mask set: U, V are final since their sweeps, which this stream has waited for)
    // the iteration's stamp: behind its finish kernel, on the stream that ran it (the last one of a call is behind everything the
    // call enqueued: the compute stream's last kernel is the sweep this tail waited for)
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], tst));
    if (tail.on) CHK(tail.done(1));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (tail.on) { HIPCHK(hipStreamSynchronize(h->tail_stream)); tail.pending[0] = tail.pending[1] = false; }
  CHK(sink.finish());
  HIPCHK(hipGetLastError());
  ho_scope.commit();
  drain_events(h);
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 5);
  HIPCHK(hipMemcpy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int it = 0; it < n_iter; ++it) {
    if (tau_out) tau_out[it] = rec[(size_t)it * 5];
    if (perf_out) for (int m = 0; m < 3; ++m) perf_out[(size_t)it * 3 + m] = rec[(size_t)it * 5 + 1 + m];
  }
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_gibbs_run_many(const bnmtf_handle* hs, int n_models, int n_iter, int update, float* const* U_outs, float* const* V_outs,
                        double* const* tau_outs, double* const* perf_outs, double* const* times_outs,
                        double* const* U_final, double* const* V_final, double* const* tau_final) try {
  if (n_models < 0 || n_iter < 0) { set_error("negative count"); return BNMTF_EINVAL; }
  if (n_models == 0 || n_iter == 0) return BNMTF_OK;
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  for (int b = 0; b < n_models; ++b) if (hs[b]->L != 0) { set_error("bnmf_gibbs_run_many on a BNMTF handle (model %d)", b); return BNMTF_ESTATE; }
  for (int b = 0; b < n_models; ++b) CHK(heldout_refuse_many(hs[b], "bnmf_gibbs_run_many", b));
  // models of the one-launch path go down in one grid per device; the others run one after the other
  std::vector<bnmtf_model*> batch; std::vector<SmallOut> outs;
  auto out_of = [&](int b) { return SmallOut{U_outs ? U_outs[b] : nullptr, V_outs ? V_outs[b] : nullptr, tau_outs ? tau_outs[b] : nullptr,
                                             perf_outs ? perf_outs[b] : nullptr, times_outs ? times_outs[b] : nullptr,
                                             U_final ? U_final[b] : nullptr, V_final ? V_final[b] : nullptr, tau_final ? tau_final[b] : nullptr}; };
  std::vector<char> taken(n_models, 0);
  // models on model b's device that actually JOIN the launch, b included: the rule of a CU-filling or wide-rank model depends on
  // the batch size (small_wanted), so the count is taken to its fixed point -- a model that would run alone on the multi-launch
  // path does not make a "batch" for the others (round 5's advice)
  auto peers = [&](int b) {
    int n = 0;
    for (int c = 0; c < n_models; ++c) n += (hs[c]->small && hs[c]->small_mode != 0 && hs[c]->device == hs[b]->device) ? 1 : 0;
    for (int round = 0; round < n_models && n > 0; ++round) {
      int m = 0;
      for (int c = 0; c < n_models; ++c) m += (hs[c]->device == hs[b]->device && small_wanted(hs[c], n)) ? 1 : 0;
      if (m == n) break;
      n = m;
    }
    return n;
  };
  for (int b = 0; b < n_models; ++b) {
    if (taken[b]) continue;
    const int np = peers(b);
    if (!small_wanted(hs[b], np)) {
      const SmallOut o = out_of(b);
      CHK(bnmf_gibbs_run(hs[b], n_iter, update, o.U, o.V, o.tau, o.perf, o.times));
      if (o.U_final || o.V_final || o.tau_final) CHK(bnmf_get_state(hs[b], o.U_final, o.V_final, o.tau_final));
      taken[b] = 1;
      continue;
    }
    batch.clear(); outs.clear();
    for (int c = b; c < n_models; ++c)
      if (!taken[c] && small_wanted(hs[c], np) && hs[c]->device == hs[b]->device) {
        bool dup = false;
        for (bnmtf_model* x : batch) dup = dup || x == hs[c];
        if (dup) { set_error("bnmf_gibbs_run_many: the same handle twice"); return BNMTF_EINVAL; }
        batch.push_back(hs[c]); outs.push_back(out_of(c)); taken[c] = 1;
      }
    CHK(small_run_many(batch.data(), (int)batch.size(), n_iter, update, outs.data()));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// ---------------------------------------------------------------------- ranks above 64: a factorisation as column blocks
// The reference takes any K (bnmf_gibbs_optimised.py:54-78).  The kernels hold a latent factor per wave lane (K <= 64), so a wider
// model runs as ceil(K / 64) COLUMN BLOCKS, one handle each (bnmtf_amd/_blocked.py): the conditionals of block b's columns given the
// other blocks are those of a rank-K_b model on the residual data R - sum_{b' != b} U_b' V_b'^T -- exactly the reference's
// sequential column order when the blocks' half sweeps run in turn, rows first (:134-137), then columns (:139-142).
int bnmf_set_column_block(bnmtf_handle h, int col0) try {
  CHK(refuse_obs(h, "bnmf_set_column_block"));
  if (col0 < 0) { set_error("negative column offset"); return BNMTF_EINVAL; }
  if (h->L != 0 || h->comm) { set_error("column blocks: BNMF handles on one GPU"); return BNMTF_ESTATE; }
  h->col0 = (uint32_t)col0;
  h->block_mode = true;
  h->small_mode = 0;                          // (the one-launch kernel runs whole iterations: not a block's half sweeps)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_set_residual_data(bnmtf_handle h, const bnmtf_handle* others, int n_others) try {
  CHK(refuse_obs(h, "bnmf_set_residual_data"));
  if (n_others < 0 || n_others > kMaxOtherBlocks) { set_error("at most %d other column blocks", kMaxOtherBlocks); return BNMTF_EINVAL; }
  if (h->comm) { set_error("residual data: one GPU"); return BNMTF_ESTATE; }       // (the target may be a BNMTF handle -- an S block of a wider tri-factorisation; the others are two-factor products)
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));
  ResidualSpec rs;
  memset(&rs, 0, sizeof(rs));
  rs.n = n_others;
  for (int b = 0; b < n_others; ++b) {
    bnmtf_model* o = others[b];
    if (!o || o == h || o->I != h->I || o->J != h->J || o->L != 0 || o->device != h->device || !o->have_state) { set_error("residual data: block %d does not fit (shape, device, state)", b); return BNMTF_EINVAL; }
    CHK(ensure_std(o));
    if (!o->std_cur && !o->vb_ready) { set_error("residual data: block %d's state is not on its multi-launch structures", b); return BNMTF_ESTATE; }
    HIPCHK(hipStreamSynchronize(o->stream));                 // (its last half sweep runs on its own stream)
    rs.A[b] = o->rows.X; rs.B[b] = o->cols.X; rs.KP[b] = o->rows.KP; rs.W[b] = o->rows.W;
  }
  for (int which = 0; which < 2; ++which) {
    Dir& d = which == 0 ? h->rows : h->cols;
    launch_residual_operand(h->Rfull, h->Mtrain, h->I, h->J, which == 0 ? 1 : 0, d.n0, d.n, d.m, d.big, d.n_pad, rs, h->stream);
  }
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// one half of an iteration of run(): the contraction, the K sequential column updates of one factor (which = 0: U, :134-137; 1: V,
// :139-142) with the handle's current tau and iteration counter, the relayout + Gram the other direction reads.  tau, the
// metrics, the samples and the iteration counter are the caller's (a column-blocked model: bnmtf_amd/_blocked.py).
int bnmf_half_sweep(bnmtf_handle h, int which, int update) try {
  CHK(refuse_obs(h, "bnmf_half_sweep"));
  if (which < 0 || which > 1 || update < 0 || update > BNMTF_UPDATE_ICM) { set_error("bnmf_half_sweep: which in {0, 1}, a known update rule"); return BNMTF_EINVAL; }
  if (h->L != 0 || h->comm) { set_error("bnmf_half_sweep: BNMF handles on one GPU"); return BNMTF_ESTATE; }
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));
  if (!h->std_cur) { set_error("bnmf_half_sweep: set the state first"); return BNMTF_ESTATE; }
  h->small_cur = false;
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  h->ho_active = false;
  h->rows.ho_filled = h->cols.ho_filled = false;
  enqueue_gemm(h, d, o, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
  SweepArgs s = sweep_args(h, d, o, mode, which == 0 ? kStreamRows : kStreamCols);
  enqueue_sweep(h, d, o, s, false);
  CHK(exchange_factor(h, d));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// ---------------------------------------------------------------------- metrics
static int metric_sums_impl(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* S, const double* B, double sums_out[6], int Kc_given);
int bnmtf_metric_sums(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* S, const double* B,
                      double sums_out[6]) { return metric_sums_impl(h, Mp, A, S, B, sums_out, 0); }
int bnmtf_metric_sums_wide(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* B, int Kc, double sums_out[6]) try {
  CHK(refuse_obs(h, "bnmtf_metric_sums_wide"));
  if (!A || !B || Kc <= 0) { set_error("bnmtf_metric_sums_wide: A [I][Kc], B [J][Kc] and Kc > 0 required"); return BNMTF_EINVAL; }
  if (h->L != 0) { set_error("bnmtf_metric_sums_wide on a BNMTF handle"); return BNMTF_ESTATE; }
  return metric_sums_impl(h, Mp, A, nullptr, B, sums_out, Kc);
} BNMTF_ABI_GUARD
static int metric_sums_impl(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* S, const double* B, double sums_out[6], int Kc_given) {
  CHK(refuse_obs(h, "bnmtf_metric_sums"));
  HIPCHK(hipSetDevice(h->device));
  const int I = h->I, J = h->J;
  std::vector<double> a_own, b_own, as;
  int Kc;  // contraction width of the two-factor product handed to the kernel
  if (!A) {
    if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
    a_own.resize((size_t)I * h->rows.W); b_own.resize((size_t)J * h->cols.W);
    const bool from_small = h->small && h->small_cur;
    if (h->L > 0) as.resize((size_t)h->K * h->L);
    if (from_small) CHK(small_download_state(h, a_own.data(), b_own.data(), h->L > 0 ? as.data() : nullptr));
    else {
      CHK(download_matrix(h, h->rows.X, I, h->rows.W, h->rows.KP, a_own.data()));
      CHK(download_matrix(h, h->cols.X, J, h->cols.W, h->cols.KP, b_own.data()));
    }
    A = a_own.data(); B = b_own.data();
    if (h->L > 0) {
      if (!from_small) {
        std::vector<float> sf((size_t)h->K * h->L);
        HIPCHK(hipMemcpy(sf.data(), h->S, sf.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t t = 0; t < sf.size(); ++t) as[t] = sf[t];
      }
      S = as.data();
    }
  }
  std::vector<double> AS;
  if (S) {   // A.S  (I x L), then a plain two-factor product with B (J x L)
    const int K = h->K, L = h->L;
    AS.assign((size_t)I * L, 0.0);
    for (int i = 0; i < I; ++i)
      for (int k = 0; k < K; ++k) {
        const double aik = A[(size_t)i * K + k];
        for (int l = 0; l < L; ++l) AS[(size_t)i * L + l] += aik * S[(size_t)k * L + l];
      }
    A = AS.data(); Kc = L;
  } else {
    Kc = h->L > 0 ? h->L : h->K;
    if (h->L > 0) { set_error("bnmtf_metric_sums: S required for a BNMTF handle"); return BNMTF_EINVAL; }
  }
  if (A && !S && h->L == 0 && Kc_given > 0) Kc = Kc_given;       // (a column-blocked factorisation hands over all its columns: bnmtf_metric_sums_wide)
  // operand copies: the handle's [I][64] / [J][64] buffers (part of a small model's arena: never freed here); factors wider than
  // 64 columns (a column-blocked model) get buffers of their own
  double* Ad = h->Ad; double* Bd = h->Bd;
  if (Kc > 64) {
    if (h->ABd_width < Kc) {
      dfree(h->AdW); dfree(h->BdW); h->AdW = nullptr; h->BdW = nullptr;
      CHK(dalloc(&h->AdW, (size_t)I * Kc, false)); CHK(dalloc(&h->BdW, (size_t)J * Kc, false));
      h->ABd_width = Kc;
    }
    Ad = h->AdW; Bd = h->BdW;
  } else if (!h->Ad) { CHK(dalloc(&h->Ad, (size_t)I * 64, false)); CHK(dalloc(&h->Bd, (size_t)J * 64, false)); Ad = h->Ad; Bd = h->Bd; }
  HIPCHK(hipMemcpyAsync(Ad, A, sizeof(double) * (size_t)I * Kc, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(Bd, B, sizeof(double) * (size_t)J * Kc, hipMemcpyHostToDevice, h->stream));
  const uint8_t* mask = h->Mtrain;
  if (Mp) {
    if (!h->Mscratch) CHK(dalloc(&h->Mscratch, (size_t)I * J, false));
    HIPCHK(hipMemcpyAsync(h->Mscratch, Mp, (size_t)I * J, hipMemcpyHostToDevice, h->stream));
    mask = h->Mscratch;
  }
  MetricArgs m;
  m.R = h->Rfull; m.Mp = mask; m.I = I; m.J = J; m.A = Ad; m.B = Bd; m.K = Kc; m.out6 = h->out6; m.A2 = nullptr; m.B2 = nullptr;
  CHK(metric_partials(h, &m.part));
  launch_metric_sums(m, h->stream);
  HIPCHK(hipMemcpyAsync(sums_out, h->out6, 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
}

int bnmtf_beta_s(bnmtf_handle h, double* out) try {
  CHK(refuse_obs(h, "bnmtf_beta_s"));
  double s[6];
  CHK(bnmtf_metric_sums(h, nullptr, nullptr, nullptr, nullptr, s));
  *out = h->beta + 0.5 * (s[2] - 2.0 * s[5] + s[4]);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// ---------------------------------------------------------------- distributions
int bnmtf_tn_sample(const double* mu, const double* tau, size_t n, uint64_t seed, uint64_t it, uint32_t col,
                    uint32_t elem0, int device, double* out) try {
  if (n == 0) return BNMTF_OK;
  HIPCHK(hipSetDevice(device));
  DevBuf<double> dm, dt, dout;
  CHK(dm.alloc(n)); CHK(dt.alloc(n)); CHK(dout.alloc(n));
  HIPCHK(hipMemcpy(dm.p, mu, n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dt.p, tau, n * sizeof(double), hipMemcpyHostToDevice));
  launch_tn_sample(dm.p, dt.p, n, seed, (uint32_t)it, col, elem0, dout.p, nullptr);
  HIPCHK(hipMemcpy(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_tn_moments(const double* mu, const double* tau, size_t n, int device, double* exp_out, double* var_out) try {
  if (n == 0) return BNMTF_OK;
  HIPCHK(hipSetDevice(device));
  DevBuf<double> dm, dt, de, dv;
  CHK(dm.alloc(n)); CHK(dt.alloc(n)); CHK(de.alloc(n)); CHK(dv.alloc(n));
  HIPCHK(hipMemcpy(dm.p, mu, n * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dt.p, tau, n * sizeof(double), hipMemcpyHostToDevice));
  launch_tn_moments(dm.p, dt.p, n, de.p, dv.p, nullptr);
  HIPCHK(hipMemcpy(exp_out, de.p, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(var_out, dv.p, n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_gamma_sample(double alpha, double beta, uint64_t seed, uint64_t it, int device, double* out) try {
  HIPCHK(hipSetDevice(device));
  DevBuf<double> d;
  CHK(d.alloc(1, true));
  launch_gamma_sample(alpha, beta, seed, (uint32_t)it, d.p, nullptr);
  HIPCHK(hipMemcpy(out, d.p, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"

#include "api_models.inc"
#include "api_trivb.inc"
#include "api_np.inc"
#include "api_obs.inc"
#include "api_obs_tri.inc"
#include "api_obs_trivb.inc"
#include "api_obs_np.inc"
#include "api_many.inc"
#include "api_top.inc"
#include "api_foldin.inc"
#include "api_predictive_q.inc"
#include "api_log_predictive.inc"
#include "api_predictive.inc"
