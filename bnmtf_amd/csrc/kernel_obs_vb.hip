// Observed-entry layout of the variational two-factor model ("VB on the entry lists"): kernel_obs.hip's
// form A with the variational column update (bnmf_vb_optimised.py:189-211 restated on the OBSERVED entries of a unit).  For
// column k of unit i, with E / S2 = var + E^2 of the other factor:
//   sa = sum_{j in Omega_i} S2_jk,   sb = sum_{j in Omega_i} E_jk^2,   se = sum_{j in Omega_i} e_ij E_jk
//   tau_ik = exptau sa,   mu_ik = (-lambda_ik + exptau (se + x_ik sb)) / tau_ik
//   (x', var') = the truncated normal's moments (tn_moments_f32);   e_ij += (x_ik - x') E_jk
// columns in order k = 0 .. K - 1; the V half sweep is the same on the column lists.
//
// obs_vb_sweep_kernel: one 64-lane wave per unit, kObsWaves units per block, lane l the unit's entries l, l + 64, ... in list
// order; every per-entry loop written once on the unit's two forms (obs_common.h: a slot without an entry gathers the zero word
// behind the columns of both transposed operands).  The wave-uniform results of a column -- mu, tau, var, sa, sb; the expectation replaces x in the unit's row -- are
// parked in LDS (every lane stores the same value and reads back its own store); behind the column loop lane k mod 64 forms the
// fp64 pieces of column k: the four sums elbo() needs of q(x) (quad, log erfc, log tau, lambda E: kernel_sweep.hip's pieces) and,
// in the V half sweep, q2 = (var + E^2) sa and q3 = E^2 sb, whose difference summed over all (unit, column) is the variance
// part of exp_square_diff over the observed entries.  A lane's columns in order, the butterfly, the block's waves in wave
// order; obs_vb_finish_kernel folds the blocks' partials in obs_fold's order.  No floating-point atomics anywhere.
//
// obs_trivb_sweep_kernel: the same body with the tri-factorisation's covariance term and column order (template parameter COV;
// bnmtf_vb_observed, api_obs_trivb.inc).  obs_vb_sweep_kernel is the COV = false instantiation and compiles to the code it had.
//
// obs_vb_esd_kernel: exp_square_diff of the state the device holds, fp64 over the row list (a block's rows b, b + grid, ...; a
// thread's entries in list order; a tree; the fold).
#include "obs_common.h"
#include "device_rng.h"

namespace bnmtf {

namespace {

constexpr int kVbParked = 5;           // mu, tau, var, sa, sb of every column, beside the unit's row and its prior rates
constexpr int kVbSums = 10;            // quad, log erfc, log tau, lambda E, q2, q3; SSE, sum P, sum P^2, sum R P

// One unit in the form S (obs_common.h).  xs / ls: the unit's expectations and prior rates in LDS, pk: the parked column results.
// sums (part != null): the lane's share of SSE, sum P, sum P^2, sum R P in sums[6 .. 9].
// COV: the tri-factorisation's F / G half sweep against an effective factor (bnmtf_vb_optimised.py:241-250 / :264-273): the columns in
// the order handed over, and the numerator less  sum_t S(k,t) mv_t (fs_t - x_k S(k,t)),  lane t holding mv_t (the other factor's
// variance summed over the unit's entries: fixed for the half sweep) and fs_t = sum_c x_c S(c,t) (from the unit's current row; one
// fmaf per new expectation).  The term is the butterfly's sum, whatever the form: the forms still give the same bits.
template <int S, bool COV>
__device__ __forceinline__ void obs_vb_unit(const ObsVbSweepArgs& a, int u, int lane, float* xs, const float* ls, float* pk, double* sums) {
#pragma clang fp contract(off)
  ObsForm<S> F(a.ptr, a.idx, a.val, a.escratch, u, lane);
  const int K = a.K, KP = a.KP;
  float* mus = pk; float* tps = pk + kObsMaxRank; float* vrs = pk + 2 * kObsMaxRank; float* sas = pk + 3 * kObsMaxRank; float* sbs = pk + 4 * kObsMaxRank;

  // ---- phase 1: the residual of every entry
  F.init((uint32_t)a.m, 0.f);
  F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
    if (F.has(t)) F.E(s, t) = obs_residual(xs, a.Xo, KP, F.J(s, t), F.val[t]);
  });

  // ---- phase 2: the columns
  const float exptau = *a.tau;
  const int only = a.only_k;
  const int kbeg = only >= 0 ? only : 0, kend = only >= 0 ? only + 1 : K;
  float fs = 0.f, mvl = 0.f;
  const bool cov_lane = COV && lane < a.cov_n;
  if (COV) {
    for (int c = 0; c < K; ++c) fs = fmaf(xs[c], cov_lane ? a.cov_S[c * a.cov_sc + lane * a.cov_st] : 0.f, fs);
    mvl = cov_lane ? a.cov_mv[(size_t)u * 32 + lane] : 0.f;
  }
  for (int kk = kbeg; kk < kend; ++kk) {
    const int k = (COV && a.order && only < 0) ? a.order[kk] : kk;
    const float* vcol = a.XoT + (size_t)k * a.ldT_o;
    const float* wcol = a.S2oT + (size_t)k * a.ldT_o;
    float se = 0.f, sb = 0.f, sa = 0.f;
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) {
      const uint32_t j = F.J(s, t);
      const float vv = F.hold(s, vcol[j]), w = wcol[j];
      // (two independent sums; their order decides how the compiler pairs them, and with that when the long form's load of e is
      // issued -- kernel_obs.hip, the same place.  Each instantiation has the order in which its rates were level with those of
      // the hand-copied loops: the other order cost COV 1 % on long units and the two-factor kernel 0.5 to 1 % on short ones)
      if (COV) { sb = fmaf(vv, vv, sb); se = fmaf(F.E(s, t), vv, se); }
      else { se = fmaf(F.E(s, t), vv, se); sb = fmaf(vv, vv, sb); }
      sa += w;
    });
    se = wave_sum(se); sb = wave_sum(sb); sa = wave_sum(sa);
    const float xk = xs[k];
    const float tau_p = exptau * sa;
    float sc = 0.f, cov = 0.f;
    if (COV) {
      sc = cov_lane ? a.cov_S[k * a.cov_sc + lane * a.cov_st] : 0.f;
      cov = wave_sum(sc * mvl * fmaf(-xk, sc, fs));
    }
    const float numer = COV ? fmaf(exptau, fmaf(xk, sb, se) - cov, -ls[k]) : fmaf(exptau, fmaf(xk, sb, se), -ls[k]);
    const float mu = numer / tau_p;
    float ef = xk, vf = 0.f;
    if (only < 0 || a.moments) tn_moments_f32(mu, tau_p, &ef, &vf);
    if (only >= 0) {                        // update_U(k) / update_V(k): mu and tau of the column -- and its moments when asked for
      if (lane == 0) {
        const size_t at = (size_t)u * KP + k;
        a.mu[at] = mu; a.tauq[at] = tau_p;
        if (a.moments) {
          a.var[at] = vf; a.X[at] = ef;
          if (!COV) { a.XT[(size_t)k * a.ldT + u] = ef; a.S2T[(size_t)k * a.ldT + u] = fmaf(ef, ef, vf); }
        }
      }
      return;
    }
    mus[k] = mu; tps[k] = tau_p; vrs[k] = vf; sas[k] = sa; sbs[k] = sb;      // (every lane stores the same value, and reads back its own store)
    xs[k] = ef;
    const float nd = xk - ef;                   // e -= (x' - x) v
    if (COV) fs = fmaf(-nd, sc, fs);
    F.each([&](int s, uint32_t t) __attribute__((always_inline)) { F.E(s, t) = fmaf(nd, F.V(s, t, vcol), F.E(s, t)); });
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
    sums[6] = sse; sums[7] = sp; sums[8] = spp; sums[9] = srp;
  }
}

// The unit's new q -- row major, the expectation and S2 transposed -- and the fp64 pieces of the lane's columns, in column order.
// One copy behind the forms, with none of their registers live.
template <bool COV>
__device__ __forceinline__ void obs_vb_pieces(const ObsVbSweepArgs& a, int u, int lane, const float* xs, const float* ls, const float* pk, double* sums) {
#pragma clang fp contract(off)
  const int K = a.K, KP = a.KP;
  const float* mus = pk; const float* tps = pk + kObsMaxRank; const float* vrs = pk + 2 * kObsMaxRank; const float* sas = pk + 3 * kObsMaxRank; const float* sbs = pk + 4 * kObsMaxRank;
  double quad = 0.0, lerfc = 0.0, ltau = 0.0, lamx = 0.0, q2 = 0.0, q3 = 0.0;
  for (int k = lane; k < KP; k += 64) {
    const size_t at = (size_t)u * KP + k;
    if (k < K) {
      const float ef = xs[k], vf = vrs[k], mu = mus[k], tau_p = tps[k];
      a.X[at] = ef; a.mu[at] = mu; a.tauq[at] = tau_p; a.var[at] = vf;
      if (!COV) {
        a.XT[(size_t)k * a.ldT + u] = ef;
        a.S2T[(size_t)k * a.ldT + u] = fmaf(ef, ef, vf);
      }
      // pieces of elbo() (bnmf_vb_optimised.py:163-177) and of exp_square_diff (:185-187) for this (unit, k)
      const double e_ = (double)ef, v_ = (double)vf, dm = e_ - (double)mu;
      quad += 0.5 * (double)tau_p * (v_ + dm * dm);
      lerfc += log(0.5 * erfc(-(double)mu * sqrt((double)tau_p) * 0.7071067811865476));
      ltau += log((double)tau_p);
      lamx += (double)ls[k] * e_;
      if (a.part) {
        q2 += (v_ + e_ * e_) * (double)sas[k];                      // sum_obs S2self_k S2other_k
        q3 += e_ * e_ * (double)sbs[k];                             // sum_obs exp_self_k^2 exp_other_k^2
      }
    } else {
      a.X[at] = 0.f; a.mu[at] = 0.f; a.tauq[at] = 0.f; a.var[at] = 0.f;
    }
  }
  sums[0] = quad; sums[1] = lerfc; sums[2] = ltau; sums[3] = lamx; sums[4] = q2; sums[5] = q3;
}

template <bool COV>
__device__ __forceinline__ void obs_vb_sweep_body(const ObsVbSweepArgs& a) {
  __shared__ float xsh[kObsWaves][kObsMaxRank];
  __shared__ float lsh[kObsWaves][kObsMaxRank];
  __shared__ float pkh[kObsWaves][kVbParked * kObsMaxRank];
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
  double sums[kVbSums];
#pragma unroll
  for (int m = 0; m < kVbSums; ++m) sums[m] = 0.0;
  if (ok) {
    obs_dispatch<kObsMaxSlots>(obs_count(a.ptr, u), a.force_long, [&](auto form) __attribute__((always_inline)) {
      obs_vb_unit<decltype(form)::value, COV>(a, u, lane, xs, ls, pkh[wave], sums);
    });
    if (a.only_k < 0) obs_vb_pieces<COV>(a, u, lane, xs, ls, pkh[wave], sums);
  }
  if (a.stat) {                      // (wave-uniform, and the same in every wave: all of them reach the barrier)
    const int nsum = a.part ? kVbSums : 4;
    const double s = obs_block_sums<kVbSums, kObsWaves>(sums, nsum);
    const int t = threadIdx.x;
    if (t < nsum) {
      if (!a.part) a.stat[(size_t)blockIdx.x * 4 + t] = s;                   // the U half sweep: the four ELBO sums
      else if (t < 6) a.stat[(size_t)blockIdx.x * 6 + t] = s;                // the V half sweep: those, q2 and q3 ...
      else a.part[(size_t)blockIdx.x * 4 + (t - 6)] = s;                     // ... and the residual's four sums
    }
  }
}

__global__ __launch_bounds__(kObsWaves * 64) void obs_vb_sweep_kernel(ObsVbSweepArgs a) { obs_vb_sweep_body<false>(a); }
__global__ __launch_bounds__(kObsWaves * 64) void obs_trivb_sweep_kernel(ObsVbSweepArgs a) { obs_vb_sweep_body<true>(a); }

// exptau and the iteration's record from the two half sweeps' sums (kernel_misc.hip vb_finish_body: the same rules and the same
// record), with exp_square_diff = SSE + sum (q2 - q3) of the V half sweep, which saw the final U
__global__ __launch_bounds__(256) void obs_vb_finish_kernel(ObsVbFinishArgs a) {
  double su[4], sv[6], t[4];
  obs_fold<4>(a.stat_r, a.nb_r, su);
  __syncthreads();
  obs_fold<6>(a.stat_c, a.nb_c, sv);
  __syncthreads();
  obs_fold<4>(a.part, a.nb_c, t);
  if (threadIdx.x == 0) {
    const double sse = t[0], sp = t[1], spp = t[2], srp = t[3], n = a.n_obs;
    const double esd = sse + (sv[4] - sv[5]);
    const double alpha_s = a.alpha + 0.5 * n, beta_s = a.beta + 0.5 * esd;
    const double exptau = alpha_s / beta_s;
    *a.tau_d = exptau; *a.tau_f = (float)exptau;
    const double ss_tot = a.sumR2 - a.sumR * a.sumR / n;
    const double cov = srp - a.sumR * sp / n, vp = spp - sp * sp / n;
    a.rec[0] = exptau; a.rec[1] = sse / n;
    a.rec[2] = ss_tot != 0.0 ? 1.0 - sse / ss_tot : __longlong_as_double(0x7ff0000000000000LL);
    a.rec[3] = cov / (sqrt(ss_tot) * sqrt(vp));
    a.rec[4] = esd; a.rec[5] = beta_s;
    for (int c = 0; c < 4; ++c) { a.rec[6 + c] = su[c]; a.rec[10 + c] = sv[c]; }
  }
}

// sum over the observed entries of (R_ij - E_i . E_j)^2 + sum_k [(var + E^2)_ik (var + E^2)_jk - E_ik^2 E_jk^2], fp64
__global__ __launch_bounds__(256) void obs_vb_esd_kernel(ObsVbEsdArgs a) {
  const int tid = threadIdx.x;
  double s[1] = {0.0};
  for (int u = blockIdx.x; u < a.n; u += gridDim.x) {
    const float* xr = a.X + (size_t)u * a.KP;
    const float* vr = a.var + (size_t)u * a.KP;
    for (uint32_t t = a.ptr[u] + (uint32_t)tid; t < a.ptr[u + 1]; t += 256) {
      const size_t j = a.idx[t];
      const float* xo = a.Xo + j * a.KP;
      const float* vo = a.varo + j * a.KP;
      double p = 0.0, vs = 0.0;
      for (int k = 0; k < a.K; ++k) {
        const double x = (double)xr[k], y = (double)xo[k], x2 = x * x, y2 = y * y;
        p = fma(x, y, p);
        vs += ((double)vr[k] + x2) * ((double)vo[k] + y2) - x2 * y2;
      }
      const double d = (double)a.val[t] - p;
      s[0] += d * d + vs;
    }
  }
  obs_tree_sums<1>(s);
  if (tid == 0) a.part[blockIdx.x] = s[0];
}

}  // namespace

void launch_obs_vb_sweep(const ObsVbSweepArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(obs_vb_sweep_kernel, dim3(obs_sweep_blocks(a.n)), dim3(kObsWaves * 64), 0, st, a);
}

void launch_obs_trivb_sweep(const ObsVbSweepArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(obs_trivb_sweep_kernel, dim3(obs_sweep_blocks(a.n)), dim3(kObsWaves * 64), 0, st, a);
}

void launch_obs_vb_finish(const ObsVbFinishArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(obs_vb_finish_kernel, dim3(1), dim3(256), 0, st, a);
}

void launch_obs_vb_esd(const ObsVbEsdArgs& a, double* out, hipStream_t st) {
  const int nb = obs_vb_esd_blocks(a.n);
  hipLaunchKernelGGL(obs_vb_esd_kernel, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(obs_fold_kernel<1>, dim3(1), dim3(256), 0, st, a.part, nb, out);
}

}  // namespace bnmtf
