// Closed-form predictive mean and variance under a mean-field q over an entry list (bnmtf_predictive_moments; DESIGN.md section
// 2.8a).  With f, a the mean and variance of row i of the rows factor, s, b of S and g, c of row j of the columns factor:
//   two factors   mean = sum_k f_k g_k                 var = sum_k [ a_k g_k^2 + c_k (f_k^2 + a_k) ]
//   three         mean = sum_l P_l g_l, P = f S        var = sum_k a_k H_k^2 + sum_l [ c_l (P_l^2 + u_l) + (g_l^2 + c_l) w_l ]
//                 H = S g,  u_l = sum_k a_k s_kl^2,  w_l = sum_k b_kl (f_k^2 + a_k)
// Every term is a product of non-negative numbers.
//
// Operands: fp64, contiguous, UNPADDED, as the classes hold them: EA, VA [I][K]; ES, VS [K][L]; EB, VB [J][W] with W = K, or L for
// the tri-factorisation.  A null variance is a fixed factor: VA and VS are tested where the row is staged, VB is a template
// parameter (the inner loop then reads half the bytes).  A row of EB / VB begins on a 16-byte boundary only when W is even: the
// entry pass is instantiated with 16-byte and with 8-byte loads.  H is this file's own table, [J][hstride] with hstride = K rounded
// up to 2 and a zero in the pad column, which meets a staged zero: always 16-byte loads.
//
// Table pass (tri only): predictive_q_table_kernel, a wave per column j, row j of EB in LDS, lanes along k, H_jk the fma chain over
// l ascending.
//
// Entry pass: predictive_kernel's layout.  The list is sorted by row (the host keeps the permutation and scatters the outputs
// back).  A wave owns one row i (kPredictiveQRows consecutive rows per block, heldout_blocks(I) blocks: no grid stride) and stages
// the row's quantities once in LDS as doubles -- two factors: f, a, f^2 + a; three: a, P, P^2 + u, w (3 K L fma, lanes along l, k
// ascending) --, at most 4 x 256 doubles per wave, and reads them by broadcast; the lanes run along the row's entries, lane l the
// entries beg + l, beg + l + 64, ..., the next entry's column fetched ahead, and each walks row j of the column operands in index
// order.  A wave without entries stages nothing.
//
// Arithmetic (fixed: an entry's two numbers depend on that entry and the moments alone, not on the order or multiplicity of the
// list or what else is in it; no floating-point atomics; contraction off, every fma written out):
//   two factors   per k ascending: mean = fma(f_k, g_k, mean); var = fma(a_k, g_k * g_k, var); var = fma(c_k, fma(f_k, f_k, a_k), var)
//   three         P_l = chain of fma(f_k, s_kl, .); u_l = chain of fma(a_k, s_kl * s_kl, .); w_l = chain of fma(b_kl, fma(f_k, f_k, a_k), .)
//                 var: per k ascending fma(a_k, H_k * H_k, var), then per l ascending
//                 mean = fma(P_l, g_l, mean); var = fma(c_l, fma(P_l, P_l, u_l), var); var = fma(fma(g_l, g_l, c_l), w_l, var)
// (the lines with c are left out when VB is null: they would add an exact zero).
#include "kernels.h"

namespace bnmtf {

namespace {

__global__ __launch_bounds__(256) void predictive_q_table_kernel(PredictiveQArgs a) {
#pragma clang fp contract(off)
  __shared__ double grow[kPredictiveQRows][kObsMaxRank];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * kPredictiveQRows + wave;
  double* const mine = grow[wave];
  if (j < a.J) {
    const double* g = a.EB + (size_t)j * a.L;
    for (int l = lane; l < a.L; l += 64) mine[l] = g[l];
  }
  __syncthreads();
  if (j >= a.J) return;
  double* h = a.H + (size_t)j * a.hstride;
  for (int k = lane; k < a.hstride; k += 64) {
    double v = 0.0;
    if (k < a.K) {
      const double* s = a.ES + (size_t)k * a.L;
      for (int l = 0; l < a.L; ++l) v = fma(s[l], mine[l], v);
    }
    h[k] = v;
  }
}

// one step of the entry pass's inner loops, on one index of the staged arrays and of row j
template <bool kVarB>
__device__ __forceinline__ void two_step(double f, double va, double q, double g, double c, double& mean, double& var) {
#pragma clang fp contract(off)
  mean = fma(f, g, mean);
  var = fma(va, g * g, var);
  if (kVarB) var = fma(c, q, var);
}
template <bool kVarB>
__device__ __forceinline__ void tri_step(double p, double r, double w, double g, double c, double& mean, double& var) {
#pragma clang fp contract(off)
  mean = fma(p, g, mean);
  if (kVarB) { var = fma(c, r, var); var = fma(fma(g, g, c), w, var); }
  else var = fma(g * g, w, var);
}

template <bool kTri, bool kVec2, bool kVarB>
__global__ __launch_bounds__(256) void predictive_q_kernel(PredictiveQArgs a) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) double rowq[kPredictiveQRows][kPredictiveQStaged][kObsMaxRank];   // the waves' staged rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kPredictiveQRows + wave;
  const bool row_ok = i < a.I;
  const uint32_t beg = row_ok ? a.rowptr[i] : 0u, end = row_ok ? a.rowptr[i + 1] : 0u;
  const int K = a.K, W = kTri ? a.L : a.K;
  // two factors: f, a, f^2 + a over k; three: a over k (a zero behind an odd K), P, P^2 + u, w over l
  double* const q0 = rowq[wave][0]; double* const q1 = rowq[wave][1]; double* const q2 = rowq[wave][2]; double* const q3 = rowq[wave][3];

  if (beg < end) {
    const double* f = a.EA + (size_t)i * K;
    const double* va = a.VA ? a.VA + (size_t)i * K : nullptr;
    if (kTri) {
      for (int k = lane; k < a.hstride; k += 64) q0[k] = (va && k < K) ? va[k] : 0.0;
      for (int l = lane; l < W; l += 64) {
        double p = 0.0, u = 0.0, w = 0.0;
        for (int k = 0; k < K; ++k) {
          const double fk = f[k], ak = va ? va[k] : 0.0;
          const double s = a.ES[(size_t)k * W + l];
          p = fma(fk, s, p);
          u = fma(ak, s * s, u);
          if (a.VS) w = fma(a.VS[(size_t)k * W + l], fma(fk, fk, ak), w);
        }
        q1[l] = p; q2[l] = fma(p, p, u); q3[l] = w;
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        const double fk = f[k], ak = va ? va[k] : 0.0;
        q0[k] = fk; q1[k] = ak; q2[k] = fma(fk, fk, ak);
      }
    }
  }
  __syncthreads();

  // ---- the row's entries, 64 per step
  uint32_t e = beg + (uint32_t)lane;
  bool live = e < end;
  uint32_t j = live ? a.col[e] : 0u;
  for (uint32_t base = beg; base < end; base += kPredictiveQStep) {
    const double* grow = a.EB + (size_t)j * W;                     // (a lane without an entry reads row 0: J >= 1)
    const double* crow = kVarB ? a.VB + (size_t)j * W : nullptr;
    const uint32_t en = e + kPredictiveQStep;
    const bool ln = en < end;
    const uint32_t jn = ln ? a.col[en] : 0u;
    double mean = 0.0, var = 0.0;
    if (kTri) {
      const double2* h2 = reinterpret_cast<const double2*>(a.H + (size_t)j * a.hstride);
      const int K2 = a.hstride >> 1;
#pragma unroll 2
      for (int q = 0; q < K2; ++q) {
        const double2 h = h2[q];
        const double2 av = *reinterpret_cast<const double2*>(q0 + 2 * q);
        var = fma(av.x, h.x * h.x, var);
        var = fma(av.y, h.y * h.y, var);
      }
    }
    if (kVec2) {
      const double2* g2 = reinterpret_cast<const double2*>(grow);
      const double2* c2 = reinterpret_cast<const double2*>(crow);
      const int W2 = W >> 1;
#pragma unroll 2
      for (int q = 0; q < W2; ++q) {
        const double2 g = g2[q];
        double2 c; c.x = 0.0; c.y = 0.0;
        if (kVarB) c = c2[q];
        if (kTri) {
          const double2 p = *reinterpret_cast<const double2*>(q1 + 2 * q);
          const double2 r = *reinterpret_cast<const double2*>(q2 + 2 * q);
          const double2 w = *reinterpret_cast<const double2*>(q3 + 2 * q);
          tri_step<kVarB>(p.x, r.x, w.x, g.x, c.x, mean, var);
          tri_step<kVarB>(p.y, r.y, w.y, g.y, c.y, mean, var);
        } else {
          const double2 f = *reinterpret_cast<const double2*>(q0 + 2 * q);
          const double2 av = *reinterpret_cast<const double2*>(q1 + 2 * q);
          const double2 fa = *reinterpret_cast<const double2*>(q2 + 2 * q);
          two_step<kVarB>(f.x, av.x, fa.x, g.x, c.x, mean, var);
          two_step<kVarB>(f.y, av.y, fa.y, g.y, c.y, mean, var);
        }
      }
    } else {
#pragma unroll 2
      for (int k = 0; k < W; ++k) {
        const double g = grow[k], c = kVarB ? crow[k] : 0.0;
        if (kTri) tri_step<kVarB>(q1[k], q2[k], q3[k], g, c, mean, var);
        else two_step<kVarB>(q0[k], q1[k], q2[k], g, c, mean, var);
      }
    }
    if (live) { a.mean[e] = mean; a.var[e] = var; }
    e = en; live = ln; j = jn;
  }
}

template <bool kTri, bool kVec2>
void launch_entries(const PredictiveQArgs& a, hipStream_t st) {
  const dim3 grid(heldout_blocks(a.I)), block(256);
  if (a.VB) hipLaunchKernelGGL((predictive_q_kernel<kTri, kVec2, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((predictive_q_kernel<kTri, kVec2, false>), grid, block, 0, st, a);
}

}  // namespace

void launch_predictive_q(const PredictiveQArgs& a, hipStream_t st) {
  if (a.L > 0) {
    hipLaunchKernelGGL(predictive_q_table_kernel, dim3(heldout_blocks(a.J)), dim3(256), 0, st, a);
    if (a.L % 2 == 0) launch_entries<true, true>(a, st);
    else launch_entries<true, false>(a, st);
  } else {
    if (a.K % 2 == 0) launch_entries<false, true>(a, st);
    else launch_entries<false, false>(a, st);
  }
}

}  // namespace bnmtf
