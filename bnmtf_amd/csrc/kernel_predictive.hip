// Posterior predictive statistics of stored samples over an entry list (bnmtf_predictive_samples): per
// entry (i, j) and per sample t the prediction p_t = U_t[i] . V_t[j] -- or (F_t[i] S_t) . G_t[j] --, and over the samples of the
// call three numbers: p of the call's first sample, sum_t (p_t - p_first) and sum_t (p_t - p_first)^2.  One launch per chunk of
// samples; the three numbers live in device memory between the launches.
//
// Operands: the chunk's samples as the host holds them, fp32, contiguous, UNPADDED: A [C][I][K], B [C][J][W] with W = K, or L for
// the tri-factorisation, whose S is [C][K][L].  A row of B begins on a 16-byte boundary only when W is a multiple of 4: the kernel
// is instantiated twice, with 16-byte loads for those widths and with 4-byte loads for every other (K = 5, K = 65, ...).
//
// Layout, obs_heldout_kernel's.  The list is sorted by row (the host keeps the permutation and scatters the outputs back).  A wave
// owns one row i (kPredictiveRows consecutive rows per block, heldout_blocks(I) blocks: no grid stride).  Per sample the wave
// stages its held factor row in LDS as doubles ([4][256], 8 KiB) -- for the tri-factorisation (F_t[i] S_t)_l, the fp64 fma chain
// over k ascending, lanes along l -- and reads it by broadcast; the lanes run along the row's entries, lane l the entries beg + l,
// beg + l + 64, ..., and each walks row j of B.  A wave without entries stages nothing.
//
// The accumulators are read-modify-written in a structure of arrays over the sorted list (p_first, sum_d, sum_d2: [n] each), by
// the one lane that owns the entry, in sample order: the samples are the OUTER loop, so the staged row -- and, for the
// tri-factorisation, its K x L product -- is formed once per (row, sample) however long the row is, and a row of any length needs
// no registers per entry.  The traffic is 40 coalesced bytes per entry and sample beside the 4 W gathered ones.
//
// Arithmetic (fixed: an entry's three numbers depend on that entry and the samples alone, not on the chunk size, the order or
// multiplicity of the list or what else is in it; no floating-point atomics): every fp32 value widened to fp64 first; p_t the fma
// chain over the inner index ascending; d = p_t - p_first; sum_d += d; sum_d2 = fma(d, d, sum_d2); t ascending across chunks.
#include "kernels.h"

namespace bnmtf {

namespace {

template <bool kVec4>
__global__ __launch_bounds__(256) void predictive_kernel(PredictiveArgs a) {
  __shared__ __attribute__((aligned(16))) double rowf[kPredictiveRows][kObsMaxRank];     // the waves' staged rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kPredictiveRows + wave;
  const bool row_ok = i < a.I;
  double* const mine = rowf[wave];
  const uint32_t beg = row_ok ? a.rowptr[i] : 0u, end = row_ok ? a.rowptr[i + 1] : 0u;
  const int W = a.L > 0 ? a.L : a.K;
  const int W4 = W >> 2;

  for (int s = 0; s < a.C; ++s) {
    // ---- the row of sample s, fp64 (the barriers are the block's: C is the same for every wave)
    if (s) __syncthreads();
    if (beg < end) {
      const float* arow = a.A + ((size_t)s * a.I + i) * a.K;
      if (a.L > 0) {
        const float* S = a.S + (size_t)s * a.K * a.L;
        for (int l = lane; l < a.L; l += 64) {
          double v = 0.0;
          for (int k = 0; k < a.K; ++k) v = fma((double)arow[k], (double)S[(size_t)k * a.L + l], v);
          mine[l] = v;
        }
      } else {
        for (int k = lane; k < a.K; k += 64) mine[k] = (double)arow[k];
      }
    }
    __syncthreads();

    // ---- the row's entries, 64 per step
    const float* Bs = a.B + (size_t)s * a.J * W;
    const bool first = a.first && s == 0;
    uint32_t e = beg + (uint32_t)lane;
    bool live = e < end;
    uint32_t j = live ? a.col[e] : 0u;
    for (uint32_t base = beg; base < end; base += kPredictiveStep) {
      const float* brow = Bs + (size_t)j * W;                      // (a lane without an entry reads row 0: J >= 1)
      const uint32_t en = e + kPredictiveStep;
      const bool ln = en < end;
      const uint32_t jn = ln ? a.col[en] : 0u;
      double p = 0.0;
      if (kVec4) {
        const float4* b4 = reinterpret_cast<const float4*>(brow);
#pragma unroll 2
        for (int q = 0; q < W4; ++q) {
          const float4 b = b4[q];
          const double2 m01 = *reinterpret_cast<const double2*>(mine + 4 * q);
          const double2 m23 = *reinterpret_cast<const double2*>(mine + 4 * q + 2);
          p = fma(m01.x, (double)b.x, p); p = fma(m01.y, (double)b.y, p);
          p = fma(m23.x, (double)b.z, p); p = fma(m23.y, (double)b.w, p);
        }
      } else {
#pragma unroll 4
        for (int k = 0; k < W; ++k) p = fma(mine[k], (double)brow[k], p);
      }
      if (live) {
        double pf;
        if (first) { pf = p; a.p_first[e] = p; }
        else pf = a.p_first[e];
        const double d = p - pf;
        a.sum_d[e] += d;
        a.sum_d2[e] = fma(d, d, a.sum_d2[e]);
      }
      e = en; live = ln; j = jn;
    }
  }
}

}  // namespace

void launch_predictive(const PredictiveArgs& a, hipStream_t st) {
  const int W = a.L > 0 ? a.L : a.K;
  const dim3 grid(heldout_blocks(a.I)), block(256);
  if (W % 4 == 0) hipLaunchKernelGGL(predictive_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(predictive_kernel<false>, grid, block, 0, st, a);
}

}  // namespace bnmtf
