// The variational tri-factorisation on the observed-entry layout ("Variational tri-factorisation"): what joins
// obs_trivb_sweep_kernel (kernel_obs_vb.hip), obs_tri_gram_vb_kernel (below) and the second-moment S system with its
// chain (kernel_ssys.hip, kernel_trivb.hip, both called as they are).  K, L <= 32; every row-major matrix has a row stride of 32.
//
// obs_trivb_eff_kernel: the effective factor of a half sweep with its second moment (bnmtf_vb_optimised.py:242-243 / :265-266),
//   m_rc = sum_q X_rq S(q,c),   S2e_rc = sum_q S2X_rq S2S(q,c) - sum_q X_rq^2 S(q,c)^2 + m_rc^2,   S2 = var + E^2,
// S(q,c) = S[q][c] (the G half sweep's F S) or S[c][q] (the F half sweep's G S^T), in the forms the sweep reads: row major [n][32]
// with zero padding columns and transposed [width][ldT] with the zero word behind every column (ldT > n; never written).  A block
// takes 64 rows as obs_tri_eff_kernel does; the three sums are fmaf in inner-index order with contraction off.
//
// obs_tri_gram_vb_kernel: the S system's per-column inputs from second moments, W~_j = sum_{i in Omega_j} (E[F_i] E[F_i]^T + diag(varF_i)),
// Pv_j and mv_j = sum_{i in Omega_j} varF_i: obs_tri_gram_kernel's loop with the variance sums riding along (at the kernel).
//
// obs_mv_kernel: the masked variance sums of the F half sweep, mv_ic = sum_{j in Omega_i} varG_jc over the row list: one wave per
// row, half h of the wave the entries h, h + 2, ... in list order, lane c the column; the halves are added by one exchange.
//
// obs_trivb_finish_kernel: obs_vb_finish_kernel's rules and record with exp_square_diff = SSE + sum (q2 - q3) + third, the third
// term (:238) from launch_tri_third's partial sums.
//
// obs_trivb_esd_kernel: exp_square_diff (:235-239) of the state the device holds, fp64, all four terms per observed entry over the
// row list: a block takes the rows b, b + grid, ...; per row it forms a_l = (F_i S)_l, b_l = (S2F_i S2S)_l, c_l = (F_i^2 S^2)_l once.
// No floating-point atomics anywhere: two runs give the same bits.
#include "obs_common.h"

namespace bnmtf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

__global__ __launch_bounds__(256) void obs_trivb_eff_kernel(ObsTriVbEffArgs a) {
#pragma clang fp contract(off)
  __shared__ float s[32][33], s2[32][33], x[kObsTriEffRows][33], x2[kObsTriEffRows][33], o[kObsTriEffRows][33], o2[kObsTriEffRows][33];
  const int tid = threadIdx.x;
  const int u0 = blockIdx.x * kObsTriEffRows;
  const int inner = a.transposeS ? a.L : a.K, width = a.transposeS ? a.K : a.L;
  for (int e = tid; e < 32 * 32; e += 256) {                       // s[q][c]: what multiplies X[.][q] in output column c
    const int q = e >> 5, c = e & 31;
    float v = 0.f, w = 0.f;
    if (q < inner && c < width) {
      const size_t at = a.transposeS ? (size_t)c * a.L + q : (size_t)q * a.L + c;
      v = a.S[at]; w = fmaf(v, v, a.varS[at]);
    }
    s[q][c] = v; s2[q][c] = w;
  }
  for (int e = tid; e < kObsTriEffRows * 32; e += 256) {
    const int r = e >> 5, c = e & 31;
    float v = 0.f, w = 0.f;
    if (u0 + r < a.n) { v = a.X[(size_t)(u0 + r) * kObsTriStride + c]; w = fmaf(v, v, a.varX[(size_t)(u0 + r) * kObsTriStride + c]); }
    x[r][c] = v; x2[r][c] = w;
  }
  __syncthreads();
  const int r = tid & 63, c0 = (tid >> 6) * 8;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    float m = 0.f, ss = 0.f, sq = 0.f;
    for (int q = 0; q < inner; ++q) {
      const float xv = x[r][q], sv = s[q][c0 + t];
      m = fmaf(xv, sv, m);
      ss = fmaf(x2[r][q], s2[q][c0 + t], ss);
      sq = fmaf(xv * xv, sv * sv, sq);
    }
    const bool in = c0 + t < width;
    o[r][c0 + t] = in ? m : 0.f;
    o2[r][c0 + t] = in ? fmaf(m, m, ss - sq) : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < kObsTriEffRows * 32; e += 256) {
    const int rr = e >> 5, c = e & 31;
    if (u0 + rr < a.n) { a.out[(size_t)(u0 + rr) * kObsTriStride + c] = o[rr][c]; a.out2[(size_t)(u0 + rr) * kObsTriStride + c] = o2[rr][c]; }
  }
  for (int c = tid >> 6; c < width; c += 4)
    if (u0 + r < a.n) { a.outT[(size_t)c * a.ldT + u0 + r] = o[r][c]; a.out2T[(size_t)c * a.ldT + u0 + r] = o2[r][c]; }
}

// obs_tri_gram_kernel (kernel_obs_tri.hip) with the second moments' diagonal: the same trips, the same MFMA Gram and Pv; lane (c, h)
// also adds varF_ic of its half's entries, in the order it adds R_ij F_ic, and the halves are added by the same exchange: the sum
// mv_jc = sum_{i in Omega_j} varF_ic goes onto the diagonal of the packed tile and out as mv [n][32].  A sibling, not a second
// instantiation of a shared body: with the body shared the sampler's kernel came out with another instruction schedule (the same
// 1 002 instructions and 95 VGPRs), and that kernel keeps its code.
__global__ __launch_bounds__(kObsTriGramWaves * 64) void obs_tri_gram_vb_kernel(ObsTriGramArgs a, ObsTriGramVbArgs vb) {
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
  float pv = 0.f, mv = 0.f;
  struct Rows { float f[8], r[8], v[8]; };
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
      const float v = vb.varF[(size_t)ix[t] * kObsTriStride + c];
      b.f[t] = e < cnt ? f : 0.f; b.r[t] = e < cnt ? r : 0.f; b.v[t] = e < cnt ? v : 0.f;
    }
  };
  auto mfmas = [&](const Rows& b) {
#pragma unroll
    for (int t = 0; t < 8; t += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.f[t], b.f[t], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(b.f[t + 1], b.f[t + 1], acc2, 0, 0, 0);
      pv = fmaf(b.r[t], b.f[t], pv);
      pv = fmaf(b.r[t + 1], b.f[t + 1], pv);
      mv += b.v[t]; mv += b.v[t + 1];
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
  mv += __shfl_xor(mv, 32, 64);                                    // (both halves hold the sum: a + b = b + a)
  if (half == 0) { a.Pv[(size_t)j * kObsTriStride + c] = c < a.K ? pv : 0.f; vb.mv[(size_t)j * kObsTriStride + c] = c < a.K ? mv : 0.f; }
  float* w = a.Wc + (size_t)j * tri_padded(a.K);
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int row = (t & 3) + 8 * (t >> 2) + 4 * half;             // C/D layout of the 32 x 32 tile: column on the lane
    if (row <= c && c < a.K) w[tri_pos(tri_index(row, c, a.K))] = row == c ? acc[t] + mv : acc[t];
  }
}

__global__ __launch_bounds__(kObsMvWaves * 64) void obs_mv_kernel(ObsMvArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
  const int u = blockIdx.x * kObsMvWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (u >= a.n) return;
  const uint32_t beg = __builtin_amdgcn_readfirstlane(a.ptr[u]), cnt = __builtin_amdgcn_readfirstlane(a.ptr[u + 1]) - beg;
  const uint32_t* idx = a.idx + beg;
  float sum = 0.f;
  uint32_t t = (uint32_t)half;
  for (; t + 6 < cnt; t += 8) {                                    // four rows in flight, added in list order
    const float v0 = a.V[(size_t)idx[t] * kObsTriStride + c], v1 = a.V[(size_t)idx[t + 2] * kObsTriStride + c];
    const float v2 = a.V[(size_t)idx[t + 4] * kObsTriStride + c], v3 = a.V[(size_t)idx[t + 6] * kObsTriStride + c];
    sum += v0; sum += v1; sum += v2; sum += v3;
  }
  for (; t < cnt; t += 2) sum += a.V[(size_t)idx[t] * kObsTriStride + c];
  sum += __shfl_xor(sum, 32, 64);
  if (half == 0) a.out[(size_t)u * kObsTriStride + c] = sum;
}

__global__ __launch_bounds__(256) void obs_trivb_finish_kernel(ObsTriVbFinishArgs b) {
  const ObsVbFinishArgs& a = b.f;
  double su[4], sv[6], t[4], th[1];
  obs_fold<4>(a.stat_r, a.nb_r, su);
  __syncthreads();
  obs_fold<6>(a.stat_c, a.nb_c, sv);
  __syncthreads();
  obs_fold<4>(a.part, a.nb_c, t);
  __syncthreads();
  obs_fold<1>(b.third, b.n_third, th);
  if (threadIdx.x == 0) {
    const double sse = t[0], sp = t[1], spp = t[2], srp = t[3], n = a.n_obs;
    const double esd = sse + (sv[4] - sv[5]) + th[0];
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

__global__ __launch_bounds__(256) void obs_trivb_esd_kernel(ObsTriVbEsdArgs a) {
  __shared__ double Sd[32 * 32], S2d[32 * 32];                     // E[S], E[S]^2 as [k][l], row stride L
  __shared__ double al[32], bl[32], cl[32], dl[32], vf[32];
  const int tid = threadIdx.x, K = a.K, L = a.L;
  for (int t = tid; t < K * L; t += 256) { const double sv = (double)a.S[t]; Sd[t] = sv; S2d[t] = sv * sv; }
  double s[1] = {0.0};
  for (int u = blockIdx.x; u < a.n; u += gridDim.x) {
    __syncthreads();
    if (tid < L) {
      double av = 0.0, bv = 0.0, cv = 0.0;
      for (int k = 0; k < K; ++k) {
        const double f = (double)a.F[(size_t)u * kObsTriStride + k], f2 = f * f, v = (double)a.varF[(size_t)u * kObsTriStride + k];
        const double sv = Sd[k * L + tid], s2 = S2d[k * L + tid];
        av = fma(f, sv, av);
        bv = fma(v + f2, (double)a.varS[k * L + tid] + s2, bv);
        cv = fma(f2, s2, cv);
      }
      al[tid] = av; bl[tid] = bv; cl[tid] = cv; dl[tid] = av * av - cv;
    }
    if (tid >= 64 && tid < 64 + K) vf[tid - 64] = (double)a.varF[(size_t)u * kObsTriStride + (tid - 64)];
    __syncthreads();
    for (uint32_t t = a.ptr[u] + (uint32_t)tid; t < a.ptr[u + 1]; t += 256) {
      const float* g = a.G + (size_t)a.idx[t] * kObsTriStride;
      const float* vg = a.varG + (size_t)a.idx[t] * kObsTriStride;
      double p = 0.0, t2 = 0.0, t4 = 0.0, t3 = 0.0;
      for (int l = 0; l < L; ++l) {
        const double gl = (double)g[l], g2 = gl * gl, vl = (double)vg[l];
        p = fma(al[l], gl, p);
        t2 += bl[l] * (vl + g2) - cl[l] * g2;
        t4 = fma(dl[l], vl, t4);
      }
      for (int k = 0; k < K; ++k) {
        double m = 0.0, sq = 0.0;
        for (int l = 0; l < L; ++l) { const double gl = (double)g[l]; m = fma(Sd[k * L + l], gl, m); sq = fma(S2d[k * L + l], gl * gl, sq); }
        t3 = fma(vf[k], m * m - sq, t3);
      }
      const double d = (double)a.val[t] - p;
      s[0] += d * d + t2 + t3 + t4;
    }
  }
  obs_tree_sums<1>(s);
  if (tid == 0) a.part[blockIdx.x] = s[0];
}

}  // namespace

void launch_obs_trivb_eff(const ObsTriVbEffArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(obs_trivb_eff_kernel, dim3(obs_tri_eff_blocks(a.n)), dim3(256), 0, st, a);
}

void launch_obs_tri_gram_vb(const ObsTriGramArgs& a, const ObsTriGramVbArgs& vb, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(obs_tri_gram_vb_kernel, dim3(obs_tri_gram_blocks(a.n)), dim3(kObsTriGramWaves * 64), 0, st, a, vb);
}

void launch_obs_mv(const ObsMvArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(obs_mv_kernel, dim3(obs_mv_blocks(a.n)), dim3(kObsMvWaves * 64), 0, st, a);
}

void launch_obs_trivb_finish(const ObsTriVbFinishArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(obs_trivb_finish_kernel, dim3(1), dim3(256), 0, st, a);
}

void launch_obs_trivb_esd(const ObsTriVbEsdArgs& a, double* out, hipStream_t st) {
  const int nb = obs_vb_esd_blocks(a.n);
  hipLaunchKernelGGL(obs_trivb_esd_kernel, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(obs_fold_kernel<1>, dim3(1), dim3(256), 0, st, a.part, nb, out);
}

}  // namespace bnmtf
