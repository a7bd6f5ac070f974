// Observed-entry layout of the two-factor Gibbs / ICM models ("form A"): the residual
//   e_ij = R_ij - U_i . V_j
// is kept on the OBSERVED entries of a unit, so a half sweep costs what the unit's observed entries cost and nothing of size
// I x J exists.  For column k of unit i (bnmf_gibbs_optimised.py:133-155, :167-177 restated):
//   a_ik = sum_{j in Omega_i} V_jk^2,   s_ik = sum_{j in Omega_i} e_ij V_jk
//   tauU_ik = tau a_ik,   muU_ik = (-lambda_ik + tau (s_ik + U_ik a_ik)) / tauU_ik
//   x' = draw / max(0, mu) / max(max(0, mu), minimum_TN);   e_ij -= (x' - U_ik) V_jk
// columns in order k = 0 .. K - 1; the V half sweep is the same on the column lists.  No contraction, no Gram matrix.
//
// obs_sweep_kernel: one 64-lane wave per unit, kObsWaves units per block; lane l owns the unit's entries l, l + 64, ... in list
// order.  The unit's own factor row and prior rates sit in LDS (2 x 1 KiB per wave) and are read by broadcast.
//   Phase 1  e = r - x . Xo_j for every entry, from whole rows of the other factor (row major [m][KP], float4 loads): no residual is
//            carried between half sweeps.
//   Phase 2  per column: gather v = XoT[k][j], per-lane fp32 partials of sum e v and sum v^2 in entry order, a butterfly over the
//            wave (every lane ends with the same bits), the wave-uniform conditional, the candidates of a draw 64 at a time across
//            the lanes -- Philox counter (unit, column, iteration, stream | candidate), first accepted candidate: oracle/rng.py's
//            chain, as sweep_generic_kernel draws it -- then e -= delta v.
// Every per-entry loop is written once, on the unit's two forms (obs_common.h, "the contract": registers for a unit of at most
// kObsMaxSlots x 64 entries, escratch behind that or under ObsSweepArgs::force_long; the same bits either way).
// End of the iteration (the V half sweep, part != null): per lane SSE = sum e^2, sum P, sum P^2, sum R P with P = R - e, fp64, in
// entry order; butterfly; the block's waves in wave order; obs_finish_kernel folds the blocks' partials -- thread t the blocks t,
// t + 256, ..., then a tree -- and makes tau and the record as finish_kernel does.  No floating-point atomics anywhere.
//
// obs_metric_kernel: the six sums of metrics_from_sums over an arbitrary (row, col, value) list, fp64 factors, fp64 dot products in
// column order, a thread's entries in list order, the same fold.
#include "obs_common.h"
#include "device_rng.h"

namespace bnmtf {

namespace {

// One unit in the form S (obs_common.h).  xs / ls: the unit's factor row and prior rates in LDS.  sums (part != null): the lane's
// share of SSE, sum P, sum P^2, sum R P.
template <int S, int MODE>
__device__ __forceinline__ void obs_unit(const ObsSweepArgs& a, int u, int lane, float* xs, const float* ls, double* sums) {
#pragma clang fp contract(off)
  ObsForm<S> F(a.ptr, a.idx, a.val, a.escratch, u, lane);
  const int K = a.K, KP = a.KP;

  // ---- phase 1: the residual of every entry
  F.init((uint32_t)a.m, 0.f);
  F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
    if (F.has(t)) F.E(s, t) = obs_residual(xs, a.Xo, KP, F.J(s, t), F.val[t]);
  });

  // ---- phase 2: the columns
  const float tau = *a.tau;
  const int cond_k = MODE == kSweepMode ? a.cond_k : -1;          // (the single-column hook runs the mode instantiation, whatever the model draws)
  const int kbeg = cond_k >= 0 ? cond_k : 0, kend = cond_k >= 0 ? cond_k + 1 : K;
  for (int k = kbeg; k < kend; ++k) {
    const float* vcol = a.XoT + (size_t)k * a.ldT_o;
    float se = 0.f, sa = 0.f;
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
      const float vv = F.hold(s, vcol[F.J(s, t)]);
      // (two independent sums; in this order the compiler pairs them so that the long form's load of e is issued beside the
      // index's and not behind it -- 3 to 8 % of a half sweep of long units)
      sa = fmaf(vv, vv, sa); se = fmaf(F.E(s, t), vv, se);
    });
    se = wave_sum(se); sa = wave_sum(sa);
    const float xk = xs[k];
    const float num = fmaf(xk, sa, se);
    const float tau_p = tau * sa;
    const float numer = fmaf(tau, num, -ls[k]);
    if (cond_k >= 0) {
      if (lane == 0) { a.numer_out[u] = (double)numer; a.tau_out[u] = (double)tau_p; }
      return;
    }
    const float mu = numer / tau_p;
    float xnew = 0.f;
    if (MODE == kSweepDraw) {
      // the key and the iteration word in vector registers: as wave-uniform values the compiler keeps the ten round keys of
      // Philox in scalar registers across the column loop, more than there are (seen as scalar spills in tools/kres.sh)
      uint32_t k0 = a.key0, k1 = a.key1, itw = a.it;
      asm volatile("" : "+v"(k0), "+v"(k1), "+v"(itw));
      xnew = tn_draw_wave(tn_params(mu, tau_p), (uint32_t)u, (uint32_t)k, itw, a.stream, lane, k0, k1);
    } else {
      xnew = fmaxf((tau_p > 0.f && mu > 0.f) ? mu : 0.f, a.min_x);
    }
    const float nd = xk - xnew;                 // e -= (x' - x) v
    xs[k] = xnew;                               // (every lane stores the same value, and reads back its own store)
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) { F.E(s, t) = fmaf(nd, F.V(s, t, vcol), F.E(s, t)); });
  }

  // ---- the unit's new row: row major, transposed, and packed into the sample slot
  for (int k = lane; k < KP; k += 64) {
    const float x = k < K ? xs[k] : 0.f;
    a.X[(size_t)u * KP + k] = x;
    if (k < K) {
      a.XT[(size_t)k * a.ldT + u] = x;
      if (a.snap) a.snap[(size_t)u * K + k] = x;
    }
  }

  // ---- end of the iteration: the lane's sums over its entries, in entry order
  if (a.part) {
    double sse = 0.0, sp = 0.0, spp = 0.0, srp = 0.0;
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
      if (F.has(t)) {
        const double ed = (double)F.E(s, t), r = (double)F.val[t], p = r - ed;
        sse = fma(ed, ed, sse); sp += p; spp = fma(p, p, spp); srp = fma(r, p, srp);
      }
    });
    sums[0] = sse; sums[1] = sp; sums[2] = spp; sums[3] = srp;
  }
}

template <int MODE>
__global__ __launch_bounds__(kObsWaves * 64) void obs_sweep_kernel(ObsSweepArgs a) {
  __shared__ float xsh[kObsWaves][kObsMaxRank];
  __shared__ float lsh[kObsWaves][kObsMaxRank];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * kObsWaves + wave;
  const bool ok = u < a.n;
  float* xs = xsh[wave];
  float* ls = lsh[wave];
  if (ok) {
    obs_stage_row(xs, a.X + (size_t)u * a.KP, a.K, a.KP, lane);
    obs_stage_row(ls, a.lambda + (size_t)u * a.KP, a.K, a.KP, lane);
  }
  __syncthreads();
  double sums[4] = {0.0, 0.0, 0.0, 0.0};
  if (ok)
    obs_dispatch<kObsMaxSlots>(obs_count(a.ptr, u), a.force_long, [&](auto form) __attribute__((always_inline)) {
      obs_unit<decltype(form)::value, MODE>(a, u, lane, xs, ls, sums);
    });
  if (a.part) {                      // (wave-uniform, and the same in every wave: all of them reach the barrier)
    const double s = obs_block_sums<4, kObsWaves>(sums, 4);
    if (threadIdx.x < 4) a.part[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
  }
}

// tau and the iteration's record from the V half sweep's sums (kernel_misc.hip finish_kernel: the same rules)
__global__ __launch_bounds__(256) void obs_finish_kernel(ObsFinishArgs a) {
  double t[4];
  obs_fold<4>(a.part, a.nb, t);
  if (threadIdx.x == 0) {
    const double sse = t[0], sp = t[1], spp = t[2], srp = t[3], n = a.n_obs;
    const double alpha_s = a.alpha + 0.5 * n, beta_s = a.beta + 0.5 * sse;
    double tau;
    if (a.update == 2) tau = (alpha_s - 1.0) / beta_s;            // gamma_mode (distributions/gamma.py:27-29)
    else if (a.update != 0) tau = alpha_s / beta_s;
    else tau = *a.gunit / beta_s;
    *a.tau_d = tau;
    *a.tau_f = (float)tau;
    const double ss_tot = a.sumR2 - a.sumR * a.sumR / n;
    const double cov = srp - a.sumR * sp / n;
    const double vp = spp - sp * sp / n;
    a.rec[0] = tau;
    a.rec[1] = sse / n;
    a.rec[2] = ss_tot != 0.0 ? 1.0 - sse / ss_tot : __longlong_as_double(0x7ff0000000000000LL);
    a.rec[3] = cov / (sqrt(ss_tot) * sqrt(vp));
    a.rec[4] = sse;
  }
}

__global__ __launch_bounds__(256) void obs_metric_kernel(ObsMetricArgs a) {
  const int tid = threadIdx.x;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t e = (size_t)blockIdx.x * 256 + tid; e < a.n; e += stride) {
    const double* ar = a.A + (size_t)a.row[e] * a.K;
    const double* br = a.B + (size_t)a.col[e] * a.K;
    double p = 0.0;
    for (int k = 0; k < a.K; ++k) p = fma(ar[k], br[k], p);
    const double r = (double)a.val[e];
    s[0] += 1.0; s[1] += r; s[2] = fma(r, r, s[2]); s[3] += p; s[4] = fma(p, p, s[4]); s[5] = fma(r, p, s[5]);
  }
  obs_tree_sums<6>(s);
  if (tid == 0)
    for (int m = 0; m < 8; ++m) a.part[(size_t)blockIdx.x * 8 + m] = m < 6 ? s[m] : 0.0;
}

}  // namespace

void launch_obs_sweep(const ObsSweepArgs& a, hipStream_t st) {
  const dim3 grid(obs_sweep_blocks(a.n)), block(kObsWaves * 64);
  if (a.mode == kSweepDraw && a.cond_k < 0) hipLaunchKernelGGL(obs_sweep_kernel<kSweepDraw>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(obs_sweep_kernel<kSweepMode>, grid, block, 0, st, a);
}

void launch_obs_finish(const ObsFinishArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(obs_finish_kernel, dim3(1), dim3(256), 0, st, a);
}

void launch_obs_metric(const ObsMetricArgs& a, double* out8, hipStream_t st) {
  const int nb = obs_metric_blocks(a.n);
  hipLaunchKernelGGL(obs_metric_kernel, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(obs_fold_kernel<8>, dim3(1), dim3(256), 0, st, a.part, nb, out8);
}

}  // namespace bnmtf
