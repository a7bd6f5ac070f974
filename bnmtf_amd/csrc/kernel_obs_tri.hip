// The tri-factorisation R ~ F S G^T on the observed-entry layout: what joins obs_sweep_kernel
// (kernel_obs.hip) to the dense S system (kernel_ssys.hip).  K, L <= 32; every row-major factor has a row stride of 32 floats.
//
// obs_tri_eff_kernel: the effective factor of a half sweep, out = X S (the G sweep's other factor F S) or X S^T (the F sweep's
// G S^T), in the two forms obs_sweep_kernel gathers: row major [n][32] with zero padding columns, and transposed [width][ldT]
// (ldT > n: the words behind a column are never written and stay zero -- the sweep's empty slots gather word n).  A block takes 64
// rows: S and the rows through LDS, thread (row, 8 columns) sums fmaf in inner-index order, the tile goes out through LDS so that
// both forms are written along their contiguous index.
//
// obs_tri_gram_kernel: the S system's inputs per column j of R, over the column list,
//   W_j = sum_{i in Omega_j} F_i F_i^T   (the dense layout forms it as F^T F minus the missing rows' products)
//   Pv_jk = sum_{i in Omega_j} R_ij F_ik (the dense layout's contraction R~^T F)
// One 64-lane wave per column, four columns per block.  The 32 x 32 tile of W_j lives in the accumulators of
// v_mfma_f32_32x32x2_f32: that instruction takes A[i][k] and B[k][j] from lane (i or j) + 32 k, so with F[entry of this half][lane
// & 31] in ONE register as both operands it adds the outer products of two entries -- half 0 of the wave holds one entry's row
// of F, half 1 the next one's.  The 528 packed pairs of K = 32 are therefore not dealt to lanes at all: each lane ends with its 16
// elements of the tile (the C/D layout: column = lane & 31) and stores those of the upper triangle at their tri_pos place.  The
// entries are dealt in list order: a trip of the loop takes 16 entries, half h the entries 8 h .. 8 h + 7 of the trip, step t
// the pair (t, 8 + t); even steps add into one accumulator, odd steps into a second one (an MFMA never waits for the one before
// it), and the two are added at the end.  Pv rides along: lane (c, h) adds R_ij F_ic of its half's entries in that order with
// fmaf, and the halves are added by one exchange.  An entry past the column's end contributes F = 0, R = 0 (+0 into sums that
// are never -0).  Nothing is atomic, nothing depends on the launch: two runs give the same bits.  The F rows come straight from
// global memory, one float per lane (a 128-byte row per half and load), no LDS.  The loop is software-pipelined as
// SColGram's is: a trip's rows are loaded while the trip before it multiplies, its indices a trip earlier still (without
// that a 4096-column launch at 411 entries per column took 97 us: 26 dependent index -> row -> MFMA round trips per wave).
#include "obs_common.h"

namespace bnmtf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

__global__ __launch_bounds__(256) void obs_tri_eff_kernel(ObsTriEffArgs a) {
#pragma clang fp contract(off)
  __shared__ float s[32][33], x[kObsTriEffRows][33], o[kObsTriEffRows][33];
  const int tid = threadIdx.x;
  const int u0 = blockIdx.x * kObsTriEffRows;
  const int inner = a.transposeS ? a.L : a.K, width = a.transposeS ? a.K : a.L;
  for (int e = tid; e < 32 * 32; e += 256) {                       // s[q][c]: what multiplies X[.][q] in output column c
    const int q = e >> 5, c = e & 31;
    float v = 0.f;
    if (q < inner && c < width) v = a.transposeS ? a.S[(size_t)c * a.L + q] : a.S[(size_t)q * a.L + c];
    s[q][c] = v;
  }
  for (int e = tid; e < kObsTriEffRows * 32; e += 256) {
    const int r = e >> 5, c = e & 31;
    x[r][c] = u0 + r < a.n ? a.X[(size_t)(u0 + r) * kObsTriStride + c] : 0.f;
  }
  __syncthreads();
  const int r = tid & 63, c0 = (tid >> 6) * 8;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float acc = 0.f;
    for (int q = 0; q < inner; ++q) acc = fmaf(x[r][q], s[q][c0 + t], acc);
    o[r][c0 + t] = c0 + t < width ? acc : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < kObsTriEffRows * 32; e += 256) {
    const int rr = e >> 5, c = e & 31;
    if (u0 + rr < a.n) a.out[(size_t)(u0 + rr) * kObsTriStride + c] = o[rr][c];
  }
  for (int c = tid >> 6; c < width; c += 4)
    if (u0 + r < a.n) a.outT[(size_t)c * a.ldT + u0 + r] = o[r][c];
}

__global__ __launch_bounds__(kObsTriGramWaves * 64) void obs_tri_gram_kernel(ObsTriGramArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
  const int j = blockIdx.x * kObsTriGramWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (j >= a.n) return;
  const uint32_t beg = __builtin_amdgcn_readfirstlane(a.ptr[j]), cnt = __builtin_amdgcn_readfirstlane(a.ptr[j + 1]) - beg;
  const uint32_t* idx = a.idx + beg;
  const float* val = a.val + beg;
  f32x16 acc, acc2;
#pragma unroll
  for (int t = 0; t < 16; ++t) { acc[t] = 0.f; acc2[t] = 0.f; }
  float pv = 0.f;
  struct Rows { float f[8], r[8]; };
  // the trip that starts at entry e0: half h takes the entries e0 + 8 h .. + 7.  An entry past the column's end reads entry 0 and
  // row 0 (always there) and is replaced by F = 0, R = 0.
  auto load_idx = [&](uint32_t e0, uint32_t (&ix)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint32_t e = e0 + 8u * (uint32_t)half + (uint32_t)t;
      ix[t] = idx[e < cnt ? e : 0u];
    }
  };
  auto load_rows = [&](uint32_t e0, const uint32_t (&ix)[8], Rows& b) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const uint32_t e = e0 + 8u * (uint32_t)half + (uint32_t)t;
      const float f = a.F[(size_t)ix[t] * kObsTriStride + c], r = val[e < cnt ? e : 0u];
      b.f[t] = e < cnt ? f : 0.f; b.r[t] = e < cnt ? r : 0.f;
    }
  };
  auto mfmas = [&](const Rows& b) {
#pragma unroll
    for (int t = 0; t < 8; t += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.f[t], b.f[t], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.f[t + 1], b.f[t + 1], acc2, 0, 0, 0);
      pv = fmaf(b.r[t], b.f[t], pv);
      pv = fmaf(b.r[t + 1], b.f[t + 1], pv);
    }
  };
  // rows a trip ahead of their products, indices two: register sets alternate without copies.  (A trip past the end multiplies
  // zeros: +0 into every sum.)
  uint32_t ia[8], ib[8];
  Rows ra, rb;
  load_idx(0, ia); load_idx(16, ib);
  load_rows(0, ia, ra);
  for (uint32_t e0 = 0; e0 < cnt; e0 += 32) {
    load_rows(e0 + 16, ib, rb); load_idx(e0 + 32, ia);
    mfmas(ra);
    load_rows(e0 + 32, ia, ra); load_idx(e0 + 48, ib);
    mfmas(rb);
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] += acc2[t];
  pv += __shfl_xor(pv, 32, 64);
  if (half == 0) a.Pv[(size_t)j * kObsTriStride + c] = c < a.K ? pv : 0.f;
  float* w = a.Wc + (size_t)j * tri_padded(a.K);
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int row = (t & 3) + 8 * (t >> 2) + 4 * half;             // C/D layout of the 32 x 32 tile: column on the lane
    if (row <= c && c < a.K) w[tri_pos(tri_index(row, c, a.K))] = acc[t];
  }
}

}  // namespace

void launch_obs_tri_eff(const ObsTriEffArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(obs_tri_eff_kernel, dim3(obs_tri_eff_blocks(a.n)), dim3(256), 0, st, a);
}

void launch_obs_tri_gram(const ObsTriGramArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(obs_tri_gram_kernel, dim3(obs_tri_gram_blocks(a.n)), dim3(kObsTriGramWaves * 64), 0, st, a);
}

}  // namespace bnmtf
