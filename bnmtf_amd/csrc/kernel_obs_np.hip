// Observed-entry layout of the non-probabilistic models: the multiplicative updates of kernel_np.hip
//   x_k <- x_k (sum_{j in Omega} v_jk R_j / P_j) / (sum_{j in Omega} v_jk),   P_j += (x_k' - x_k) v_jk
// column after column, with P = U V^T (NMTF: F S G^T) kept on the OBSERVED entries of a unit only: a pass costs what the observed
// entries cost, nothing of size I x J exists and no row or column is too long.
//
// onp_sweep_kernel (kernel_obs.hip's shape): one 64-lane wave per unit, kObsWaves units per block; lane l owns the unit's entries
// l, l + 64, ... in list order; the unit's factor row sits in LDS and is read by broadcast.
//   Phase 1  P = x . Xo_j for every entry, from whole rows of the other factor (row major [m][KP], float4 loads): no P is carried
//            between half sweeps.
//   Phase 2  per column: gather v = XoT[k][j], per-lane fp32 partials of sum v (r rcp(p)) and sum v in entry order -- the quotient
//            as NpSweep takes it, r times the hardware reciprocal of p --, a butterfly over the wave (every lane ends with
//            the same bits), x_k' = (float)((double)x_k num / den) in every lane alike, then p += (x_k' - x_k) v.
// Every per-entry loop is written once, on the unit's two forms (obs_common.h, "the contract"), with P in the place of the
// residual: the register form keeps p, r, j and v, and a slot without an entry holds r = 0 and p = 1 -- it adds +0 to both sums;
// OnpSweepArgs::force_long sends every unit down the long form.  The single-column form is the same kernel on [k, k + 1); resume / keep hand P from one such call to the next
// through escratch, so the columns one by one are the half sweep.
// End of the iteration (part != null: the V / G half sweep): per lane the eight sums of np_entry_stats from the final P, fp64, in
// entry order; butterfly; the block's waves in wave order; obs_fold_kernel<8> folds the blocks' partials -- thread t the blocks t,
// t + 256, ..., then a tree -- into the iteration's record.  No floating-point atomics anywhere.
//
// onp_eff_kernel: NMTF's effective factors G S^T and F S, fp32, any K, L <= 256, in both forms.
// onp_s_pass_kernel: one pass of NMTF's S step (NpSPass's scheme on the row list): a wave owns a row, the lanes run along
// its entries; P per entry in escratch in row-list order; a pass sums the previous pass's block partials -- every block in the same
// order, block 0 stores S --, moves P by that entry's change and sums the next entry's numerator and denominator.
// onp_metric_kernel: the eight sums over an arbitrary entry list, P in fp64 from the fp32 factors ((F_i S) . G_j with F_i S in fp64).
#include <math.h>

#include "obs_common.h"

namespace bnmtf {

namespace {

// the eight sums of one observed entry (kernel_np.hip np_entry_stats), fp64
__device__ __forceinline__ void onp_entry_stats(double* s, double r, double p) {
#pragma clang fp contract(off)
  s[0] += 1.0; s[1] += r; s[2] = fma(r, r, s[2]); s[3] += p; s[4] = fma(p, p, s[4]); s[5] = fma(r, p, s[5]);
  s[6] += r * log(r / p) - r + p;                              // nmf_np.py:146-148 (0 log 0 is NaN there too)
  const double d = r - p;
  s[7] = fma(d, d, s[7]);
}

// One unit in the form S (obs_common.h): the form's e is P, an empty slot holds P = 1 and r = 0.  xs: the unit's factor row in LDS.
template <int S>
__device__ __forceinline__ void onp_unit(const OnpSweepArgs& a, int u, int lane, float* xs, double* sums) {
#pragma clang fp contract(off)
  ObsForm<S> F(a.ptr, a.idx, a.val, a.escratch, u, lane);
  const int K = a.K, KP = a.KP;

  // ---- phase 1: P of every entry -- or, in the single-column form, the P the previous column's call left in escratch
  F.init((uint32_t)a.m, 1.f);
  if (a.resume) F.from_scratch();
  else F.each([&](int s, uint32_t t) __attribute__((always_inline)) { if (F.has(t)) F.E(s, t) = obs_dot(xs, a.Xo, KP, F.J(s, t)); });

  // ---- phase 2: the columns
  for (int k = a.k0; k < a.k1; ++k) {
    const float* vcol = a.XoT + (size_t)k * a.ldT_o;
    float sn = 0.f, sd = 0.f;
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
      const float vv = F.hold(s, vcol[F.J(s, t)]);
      sn = fmaf(vv, F.R(s, t) * __builtin_amdgcn_rcpf(F.E(s, t)), sn); sd = sd + vv;
    });
    sn = wave_sum(sn); sd = wave_sum(sd);
    const float xk = xs[k];
    const float xnew = (float)((double)xk * (double)sn / (double)sd);
    const float d = xnew - xk;
    xs[k] = xnew;                               // (every lane stores the same value, and reads back its own store)
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) { F.E(s, t) = fmaf(d, F.V(s, t, vcol), F.E(s, t)); });
  }

  // ---- the unit's new row: row major and transposed
  for (int k = lane; k < KP; k += 64) {
    const float x = k < K ? xs[k] : 0.f;
    a.X[(size_t)u * KP + k] = x;
    if (k < K) a.XT[(size_t)k * a.ldT + u] = x;
  }

  // ---- the single-column form: P for the next column's call
  if (a.keep) F.to_scratch();

  // ---- end of the iteration: the lane's sums over its entries, in entry order
  if (a.part)
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) { if (F.has(t)) onp_entry_stats(sums, (double)F.R(s, t), (double)F.E(s, t)); });
}

__global__ __launch_bounds__(kObsWaves * 64) void onp_sweep_kernel(OnpSweepArgs a) {
  __shared__ float xsh[kObsWaves][kObsMaxRank];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * kObsWaves + wave;
  const bool ok = u < a.n;
  float* xs = xsh[wave];
  if (ok) obs_stage_row(xs, a.X + (size_t)u * a.KP, a.K, a.KP, lane);
  __syncthreads();
  double sums[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (ok)
    obs_dispatch<kObsMaxSlots>(obs_count(a.ptr, u), a.force_long, [&](auto form) __attribute__((always_inline)) {
      onp_unit<decltype(form)::value>(a, u, lane, xs, sums);
    });
  if (a.part) {                      // (wave-uniform, and the same in every wave: all of them reach the barrier)
    const double s = obs_block_sums<8, kObsWaves>(sums, 8);
    if (threadIdx.x < 8) a.part[(size_t)blockIdx.x * 8 + threadIdx.x] = s;
  }
}

// element (x, c) of X . S or X . S^T, the inner index in order; the padding columns of the row-major form are written as zeros
__global__ __launch_bounds__(256) void onp_eff_kernel(OnpEffArgs a) {
#pragma clang fp contract(off)
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)a.n * a.ldo) return;
  const int x = (int)(q / a.ldo), c = (int)(q - (size_t)x * a.ldo);
  const int W = a.transposeS ? a.K : a.L, A = a.transposeS ? a.L : a.K;
  float s = 0.f;
  if (c < W) {
    const float* xr = a.X + (size_t)x * a.ldX;
    const float* sp = a.transposeS ? a.S + (size_t)c * a.L : a.S + c;
    const int ss = a.transposeS ? 1 : a.L;
    for (int t = 0; t < A; ++t) s = fmaf(sp[(size_t)t * ss], xr[t], s);
    a.outT[(size_t)c * a.ldT + x] = s;
  }
  a.out[q] = s;
}

template <bool BUILD>
__global__ __launch_bounds__(kObsWaves * 64) void onp_s_pass_kernel(OnpSPassArgs a) {
#pragma clang fp contract(off)
  __shared__ double wred[kObsWaves][2];
  __shared__ float s_delta;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float d = 0.f;
  if (a.prev >= 0) {                 // finish entry prev: every block sums the previous pass's partials in the same order
    double nd[2];                    // numerator and denominator
    obs_fold<2>(a.part_prev, a.nb, nd);
    if (t == 0) {
      const float s0 = a.S_in[a.prev];
      const float s1 = (float)((double)s0 * nd[0] / nd[1]);
      s_delta = s1 - s0;
      if (blockIdx.x == 0) a.S_out[a.prev] = s1;
    }
    __syncthreads();
    d = s_delta;
  }
  if (a.cur < 0 && !a.apply) return;
  const int kp = a.prev >= 0 ? a.prev / a.L : 0, lp = a.prev >= 0 ? a.prev % a.L : 0;
  const int k = a.cur >= 0 ? a.cur / a.L : 0, l = a.cur >= 0 ? a.cur % a.L : 0;
  const float* gp = a.GT + (size_t)lp * a.ldGT;
  const float* gl = a.GT + (size_t)l * a.ldGT;
  float nu = 0.f, de = 0.f;
  for (int i = blockIdx.x * kObsWaves + wave; i < a.I; i += (int)gridDim.x * kObsWaves) {
    const uint32_t beg = a.ptr[i], end = a.ptr[i + 1];
    const float* frow = a.F + (size_t)i * a.ldF;
    const float fp = d * frow[kp], fk = frow[k];
    for (uint32_t e = beg + (uint32_t)lane; e < end; e += 64) {
      const uint32_t j = a.idx[e];
      float p = BUILD ? obs_dot(frow, a.Xo, a.ldF, j) : a.P[e];
      if (a.prev >= 0) p = fmaf(fp, gp[j], p);
      if (BUILD || a.prev >= 0) a.P[e] = p;
      if (a.cur >= 0) {
        const float w = fk * gl[j];
        nu = fmaf(w, a.val[e] * __builtin_amdgcn_rcpf(p), nu);
        de = de + w;
      }
    }
  }
  if (a.cur < 0) return;
  const double nud = wave_sum_d((double)nu), ded = wave_sum_d((double)de);
  if (lane == 0) { wred[wave][0] = nud; wred[wave][1] = ded; }
  __syncthreads();
  if (t == 0) {
    double sn = 0.0, sd = 0.0;
    for (int w = 0; w < kObsWaves; ++w) { sn += wred[w][0]; sd += wred[w][1]; }
    a.part_cur[(size_t)blockIdx.x * 2] = sn; a.part_cur[(size_t)blockIdx.x * 2 + 1] = sd;
  }
}

__global__ __launch_bounds__(256) void onp_metric_kernel(OnpMetricArgs a) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + tid; e < a.n; e += stride) {
    uint32_t i;
    if (a.row) i = a.row[e];
    else {                             // the last row whose list begins at or before e (no row is empty)
      uint32_t lo = 0, hi = (uint32_t)a.I;
      while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if ((size_t)a.ptr[mid] <= e) lo = mid; else hi = mid; }
      i = lo;
    }
    const float* ar = a.A + (size_t)i * a.ldA;
    const float* br = a.B + (size_t)a.col[e] * a.ldB;
    double p = 0.0;
    if (a.L == 0) {
      for (int k = 0; k < a.K; ++k) p = fma((double)ar[k], (double)br[k], p);
    } else {
      for (int l = 0; l < a.L; ++l) {
        double fs = 0.0;
        for (int k = 0; k < a.K; ++k) fs = fma((double)ar[k], (double)a.S[(size_t)k * a.L + l], fs);
        p = fma(fs, (double)br[l], p);
      }
    }
    onp_entry_stats(s, (double)a.val[e], p);
  }
  obs_tree_sums<8>(s);
  if (tid == 0)
    for (int m = 0; m < 8; ++m) a.part[(size_t)blockIdx.x * 8 + m] = s[m];
}

}  // namespace

void launch_onp_sweep(const OnpSweepArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(onp_sweep_kernel, dim3(obs_sweep_blocks(a.n)), dim3(kObsWaves * 64), 0, st, a);
}

void launch_onp_fold(const double* part, int nb, double* out8, hipStream_t st) {
  hipLaunchKernelGGL(obs_fold_kernel<8>, dim3(1), dim3(256), 0, st, part, nb, out8);
}

void launch_onp_eff(const OnpEffArgs& a, hipStream_t st) {
  const size_t tot = (size_t)a.n * a.ldo;
  hipLaunchKernelGGL(onp_eff_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a);
}

void launch_onp_s_pass(const OnpSPassArgs& a, hipStream_t st) {
  const dim3 grid(a.cur < 0 && !a.apply ? 1 : a.nb), block(kObsWaves * 64);     // (only finishing prev: block 0 stores S)
  if (a.build) hipLaunchKernelGGL(onp_s_pass_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(onp_s_pass_kernel<false>, grid, block, 0, st, a);
}

void launch_onp_metric(const OnpMetricArgs& a, double* out8, hipStream_t st) {
  const int nb = obs_metric_blocks(a.n);
  hipLaunchKernelGGL(onp_metric_kernel, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(obs_fold_kernel<8>, dim3(1), dim3(256), 0, st, (const double*)a.part, nb, out8);
}

}  // namespace bnmtf
