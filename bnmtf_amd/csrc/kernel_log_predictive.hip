// Log predictive density of known values under stored samples over an entry list (bnmtf_log_predictive_samples; DESIGN.md section
// 2.8b): per entry e = (i, j) with value r and per sample t the prediction p_t = U_t[i] . V_t[j] -- or (F_t[i] S_t) . G_t[j] --,
// the Gaussian log-likelihood l_t = c_t - h_t (r - p_t)^2 with c_t = (log tau_t - log 2 pi) / 2 and h_t = tau_t / 2 from the host,
// and over the samples of the call five numbers: l of the call's first sample, sum_t (l_t - l_first), sum_t (l_t - l_first)^2,
// max_t l_t and sum_t exp(l_t - max).  One launch per chunk of samples; the five live in device memory between the launches.
//
// Operands and layout: predictive_kernel's (kernel_predictive.hip), to the letter.  The chunk's samples as the host holds them,
// fp32, contiguous, unpadded: A [C][I][K], B [C][J][W] with W = K, or L for the tri-factorisation, whose S is [C][K][L]; two
// instantiations, 16-byte loads of a row of B when W % 4 == 0 and 4-byte loads otherwise.  The list is sorted by row; a wave owns
// one row i (kPredictiveRows rows per block, heldout_blocks(I) blocks: no grid stride), stages its fp64 factor row -- or
// (F_t[i] S_t)_l, the fma chain over k ascending -- in LDS once per (row, sample) and reads it by broadcast; lane l takes the
// row's entries beg + l, beg + l + 64, ...  The samples are the OUTER loop.
//
// The accumulators are a structure of arrays over the sorted list ([n] each), read-modify-written by the one lane that owns the
// entry, in sample order: 80 coalesced bytes per entry and sample (five doubles read and written) and 8 for the value, beside the
// 4 W gathered ones.  (A variant that keeps them in registers across a chunk, entries outer and samples inner, has not been built:
// DESIGN.md section 2.8b.)
//
// Arithmetic (fixed: an entry's five numbers depend on that entry, its value and the samples alone, not on the chunk size, the
// order or multiplicity of the list or what else is in it; no floating-point atomics): every fp32 value widened to fp64 first;
// p_t the fma chain over the inner index ascending; d = r - p_t; l_t = fma(-(h_t d), d, c_t).  At the call's first sample
// l_first = l_max = l_t and sum_exp = 1, the two sums stay 0.  After it, t ascending across chunks: delta = l_t - l_first;
// sum_d += delta; sum_d2 = fma(delta, delta, sum_d2); and the running-maximum log-sum-exp: with x = exp(-|l_t - l_max|) -- that is
// exp(l_max - l_t) when l_t > l_max and exp(l_t - l_max) otherwise, one call of exp for both branches --, l_t > l_max: sum_exp =
// fma(sum_exp, x, 1), l_max = l_t; else sum_exp += x.  The shift is the maximum so far, never the first sample: sum_exp stays in
// [1, T] however far below the rest a sample lies.  The device takes no logarithm.
//
// Resources (gfx950, from -Rpass-analysis=kernel-resource-usage, tools/kres.sh): 16-byte loads 78 VGPRs, 6 waves per SIMD;
// 4-byte loads 68 VGPRs, 7 waves per SIMD; 8 192 bytes of LDS per block (the four waves' staged rows); no scratch, no spills.
#include "kernels.h"

namespace bnmtf {

namespace {

template <bool kVec4>
__global__ __launch_bounds__(256) void log_predictive_kernel(LogPredictiveArgs a) {
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
    const double cs = a.c[s], hs = a.h[s];
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
        const double d = a.val[e] - p;
        const double l = fma(-(hs * d), d, cs);
        if (first) {
          a.l_first[e] = l; a.l_max[e] = l; a.sum_exp[e] = 1.0;
        } else {
          const double delta = l - a.l_first[e];
          a.sum_d[e] += delta;
          a.sum_d2[e] = fma(delta, delta, a.sum_d2[e]);
          const double m = a.l_max[e], se = a.sum_exp[e];
          const bool up = l > m;
          const double x = exp(up ? m - l : l - m);
          a.sum_exp[e] = up ? fma(se, x, 1.0) : se + x;
          if (up) a.l_max[e] = l;
        }
      }
      e = en; live = ln; j = jn;
    }
  }
}

}  // namespace

void launch_log_predictive(const LogPredictiveArgs& a, hipStream_t st) {
  const int W = a.L > 0 ? a.L : a.K;
  const dim3 grid(heldout_blocks(a.I)), block(256);
  if (W % 4 == 0) hipLaunchKernelGGL(log_predictive_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(log_predictive_kernel<false>, grid, block, 0, st, a);
}

}  // namespace bnmtf
