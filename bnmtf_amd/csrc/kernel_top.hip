// The n best columns of every selected row (bnmtf_top_entries): per selected row q the n columns j, not in
// the row's exclusion list, whose score A[q] . B[j] -- or (F[q] S) . G[j] -- comes first under the total order
//     higher score first (largest; lower first otherwise), equal scores: lower column first, -0.0 equal to 0.0.
// The answer is unique, so it cannot depend on timing, on the launch shape or on the column split.
//
// Score (fixed: the rule of obs_heldout_kernel, predictive_kernel and obs_metric_kernel): the fp64 fma chain over the inner index
// 0 .. W - 1 ascending from 0.0 of the fp64 factor values; for the tri-factorisation (F[q] S)_l is first the chain over k
// (top_fs_kernel, lanes along l) and the score the chain over l.  A score's bits depend on the pair's factor rows alone.
//
// Layout, obs_heldout_kernel's.  A wave owns one (row, segment) pair -- kTopRows pairs per block, consecutive rows of one segment,
// so a block's waves walk the same rows of B --, stages the row's held factor row in LDS as doubles ([4][256], 8 KiB) and reads it
// by broadcast; lane l scores column base + l, kTopStep columns per wave step, and walks row j of B with 16-byte loads (B's row
// stride is even: an odd W ends in one 8-byte load); the first load of the next step is fetched ahead.  A column is dropped when a
// binary search finds it in the row's sorted exclusion list.
//
// Selection, without atomics.  The wave keeps its list sorted, best first, in LDS ([4][128] keys and columns, 6 KiB; key = score,
// or -score when lower comes first: the negation is exact both ways).  The list's n-th element is the threshold; while the list is
// short everything passes.  Per step one ballot of the lanes whose (key, column) beats the threshold; the set bits are offered in
// lane order, each against the threshold as it then stands: its place is the number of list elements that beat it (two ballots, a
// lane per slot pair), the tail moves down one slot (read, wave barrier, write) and lane 0 writes the newcomer.
//
// Split.  Segment s of a row is the steps [s seg_steps, (s + 1) seg_steps) of its ceil(J / 64); a segment past the last step is
// empty.  Every wave writes its list to part_*; top_merge_kernel (a wave per row) offers a row's lists to the same routine and
// writes the answer, padded with -1 / nan.  It runs for split = 1 too: one path, the same bytes for every split.
#include "kernels.h"

namespace bnmtf {

namespace {

__device__ __forceinline__ bool top_beats(double ka, int ca, double kb, int cb) { return ka > kb || (ka == kb && ca < cb); }

__device__ __forceinline__ void top_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Offer every lane's candidate (key, col; `valid`) to the wave's list lk / lc of cnt elements (cnt and n wave-uniform); returns
// the new count.  Called by all 64 lanes.
__device__ __forceinline__ int top_offer(double* lk, int* lc, int cnt, int n, double key, int col, bool valid, int lane) {
  const bool pass = valid && (cnt < n || top_beats(key, col, lk[n - 1], lc[n - 1]));
  unsigned long long mask = __ballot(pass);
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1ull;
    const double k = __shfl(key, src, 64);
    const int c = __shfl(col, src, 64);
    if (cnt == n && !top_beats(k, c, lk[n - 1], lc[n - 1])) continue;         // (the threshold has risen since the ballot)
    const int i0 = lane, i1 = lane + 64;
    const bool b0 = i0 < cnt && top_beats(lk[i0], lc[i0], k, c);
    const bool b1 = i1 < cnt && top_beats(lk[i1], lc[i1], k, c);
    const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));          // (the list is sorted: those that beat it are a prefix)
    const int ncnt = cnt < n ? cnt + 1 : n;                                   // pos < ncnt: a full list's last element lost to it
    const bool m0 = i0 > pos && i0 < ncnt, m1 = i1 > pos && i1 < ncnt;
    double k0 = 0.0, k1 = 0.0;
    int c0 = 0, c1 = 0;
    if (m0) { k0 = lk[i0 - 1]; c0 = lc[i0 - 1]; }
    if (m1) { k1 = lk[i1 - 1]; c1 = lc[i1 - 1]; }
    top_wave_sync();
    if (m0) { lk[i0] = k0; lc[i0] = c0; }
    if (m1) { lk[i1] = k1; lc[i1] = c1; }
    if (lane == 0) { lk[pos] = k; lc[pos] = c; }
    top_wave_sync();
    cnt = ncnt;
  }
  return cnt;
}

// (F[q] S)_l, the fma chain over k ascending: a block per selected row, threads along l
__global__ __launch_bounds__(256) void top_fs_kernel(TopArgs a) {
  const int q = blockIdx.x, l = threadIdx.x;
  if (q >= a.r || l >= a.L) return;
  const double* f = a.A + (size_t)q * a.K;
  double v = 0.0;
  for (int k = 0; k < a.K; ++k) v = fma(f[k], a.S[(size_t)k * a.L + l], v);
  a.FS[(size_t)q * a.L + l] = v;
}

__global__ __launch_bounds__(256) void top_kernel(TopArgs a) {
  __shared__ __attribute__((aligned(16))) double rowf[kTopRows][kObsMaxRank];       // the waves' staged rows
  __shared__ double list_key[kTopRows][kTopMaxN];
  __shared__ int list_col[kTopRows][kTopMaxN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long pair = (long long)blockIdx.x * kTopRows + wave;
  const bool pair_ok = pair < (long long)a.r * a.split;
  const int seg = pair_ok ? (int)(pair / a.r) : 0, q = pair_ok ? (int)(pair % a.r) : 0;
  double* const mine = rowf[wave];
  double* const lk = list_key[wave];
  int* const lc = list_col[wave];
  const int W = a.L > 0 ? a.L : a.K, W2 = W >> 1;
  const int steps = (a.J + kTopStep - 1) / kTopStep;
  const long long s0 = (long long)seg * a.seg_steps;
  const int step_beg = s0 < steps ? (int)s0 : steps;
  const int step_end = s0 + a.seg_steps < steps ? (int)(s0 + a.seg_steps) : steps;
  const bool work = pair_ok && step_beg < step_end;

  if (work) {
    const double* src = a.L > 0 ? a.FS + (size_t)q * a.L : a.A + (size_t)q * a.K;
    for (int k = lane; k < W; k += 64) mine[k] = src[k];
  }
  __syncthreads();
  if (!pair_ok) return;

  int cnt = 0;
  if (work) {
    const uint32_t xbeg = a.exptr[q], xend = a.exptr[q + 1];
    const int col_end = step_end * kTopStep < a.J ? step_end * kTopStep : a.J;
    int j = step_beg * kTopStep + lane;
    bool live = j < col_end;
    const double* brow = a.B + (size_t)(live ? j : 0) * a.stride;                     // (a lane without a column reads row 0: J >= 1)
    double2 b0 = W2 ? *reinterpret_cast<const double2*>(brow) : double2{0.0, 0.0};
    for (int step = step_beg; step < step_end; ++step) {
      const int jn = j + kTopStep;
      const bool ln = jn < col_end;
      const double* bnext = a.B + (size_t)(ln ? jn : 0) * a.stride;
      const double2 nb0 = W2 ? *reinterpret_cast<const double2*>(bnext) : double2{0.0, 0.0};
      // is the column excluded?  (lower bound in the row's ascending list)
      uint32_t lo = xbeg, hi = xend;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.excol[mid] < (uint32_t)j) lo = mid + 1; else hi = mid;
      }
      const bool valid = live && !(lo < xend && a.excol[lo] == (uint32_t)j);
      double p = 0.0;
      if (W2) {
        const double2 m = *reinterpret_cast<const double2*>(mine);
        p = fma(m.x, b0.x, p); p = fma(m.y, b0.y, p);
      }
      const double2* b2 = reinterpret_cast<const double2*>(brow);
#pragma unroll 4
      for (int t = 1; t < W2; ++t) {
        const double2 b = b2[t];
        const double2 m = *reinterpret_cast<const double2*>(mine + 2 * t);
        p = fma(m.x, b.x, p); p = fma(m.y, b.y, p);
      }
      if (W & 1) p = fma(mine[W - 1], brow[W - 1], p);
      cnt = top_offer(lk, lc, cnt, a.n, a.largest ? p : -p, j, valid, lane);
      j = jn; live = ln; brow = bnext; b0 = nb0;
    }
  }
  // ---- the wave's list, best first
  const size_t slot = (size_t)q * a.split + seg;
  for (int t = lane; t < cnt; t += 64) { a.part_key[slot * a.n + t] = lk[t]; a.part_col[slot * a.n + t] = lc[t]; }
  if (lane == 0) a.part_cnt[slot] = cnt;
}

// a wave per selected row: its segments' lists through the same routine, and the answer
__global__ __launch_bounds__(256) void top_merge_kernel(TopArgs a) {
  __shared__ double list_key[kTopRows][kTopMaxN];
  __shared__ int list_col[kTopRows][kTopMaxN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * kTopRows + wave;
  if (q >= a.r) return;
  double* const lk = list_key[wave];
  int* const lc = list_col[wave];
  int cnt = 0;
  for (int seg = 0; seg < a.split; ++seg) {
    const size_t slot = (size_t)q * a.split + seg;
    const int have = a.part_cnt[slot];
    for (int t0 = 0; t0 < have; t0 += 64) {
      const int t = t0 + lane;
      const bool valid = t < have;
      const double key = valid ? a.part_key[slot * a.n + t] : 0.0;
      const int col = valid ? a.part_col[slot * a.n + t] : 0;
      cnt = top_offer(lk, lc, cnt, a.n, key, col, valid, lane);
    }
  }
  for (int t = lane; t < a.n; t += 64) {
    const bool have = t < cnt;
    a.cols[(size_t)q * a.n + t] = have ? lc[t] : -1;
    a.scores[(size_t)q * a.n + t] = have ? (a.largest ? lk[t] : -lk[t]) : __builtin_nan("");
  }
  if (lane == 0) a.counts[q] = cnt;
}

}  // namespace

void launch_top(const TopArgs& a, hipStream_t st) {
  if (a.L > 0) hipLaunchKernelGGL(top_fs_kernel, dim3(a.r), dim3(256), 0, st, a);
  const long long pairs = (long long)a.r * a.split;
  hipLaunchKernelGGL(top_kernel, dim3((unsigned)((pairs + kTopRows - 1) / kTopRows)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(top_merge_kernel, dim3((unsigned)heldout_blocks(a.r)), dim3(256), 0, st, a);
}

}  // namespace bnmtf
