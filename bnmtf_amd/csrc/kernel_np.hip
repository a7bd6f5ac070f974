// Non-probabilistic NMF / NMTF (nmf_np.py, Lee-Seung; nmtf_np.py, Yoo-Choi): multiplicative updates.
//
// The half sweep (NpSweep) is the hot path: U_ik *= (sum_{j in Omega_i} V_jk R_ij / P_ij) / (sum_{j in Omega_i} V_jk),
// column after column, with P = U V^T moved by every column's change.  Given V the rows of U are independent, so a block owns
// RB rows: their data and their P live in registers (thread t holds the inner indices t + T e, e < E, of every row), the
// block's U rows in LDS.  P is rebuilt from U and V at the start of every half sweep (no P in HBM, no drift carried from one half
// sweep to the next).  Each column V[:, k] is read once per block from L2 into registers -- one slice per thread, so no wave
// reads more than its own share of V and every element serves RB rows.  The V half sweep is the same kernel on the transposed
// data; NMTF's F step is this kernel with V := G S^T, its G step with U := F S.
//
// Unobserved entries are NaN in the kernel's copy of R (np_prepare_kernel): they add nothing and are never divided by.
// Per-lane sums are fp32, folded over the wave in a fixed butterfly, across waves and blocks in fp64 in a fixed order: a run
// gives the same bits every time.
#include <math.h>

#include "kernels.h"
#include "many.h"

namespace bnmtf {

constexpr int kNpMaxWaves = 16;

// Rn[i][j] = R[i][j] where observed, NaN elsewhere; RnT = Rn^T.  32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void np_prepare_kernel(const float* __restrict__ R, const uint8_t* __restrict__ M, int I, int J,
                                                         float* __restrict__ Rn, float* __restrict__ RnT) {
  __shared__ float tile[32][33];
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, j = j0 + tx;
    float v = __builtin_nanf("");
    if (i < I && j < J) {
      const size_t o = (size_t)i * J + j;
      if (M[o]) v = R[o];
      Rn[o] = v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + r, i = i0 + tx;
    if (i < I && j < J) RnT[(size_t)j * I + i] = tile[tx][r];
  }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The eight training-mask sums of one observed entry (n, R, R^2, P, P^2, R P, I-divergence, (R - P)^2), fp64.
__device__ __forceinline__ void np_entry_stats(double* s, float r, float p) {
  const double rd = r, pd = p;
  s[0] += 1.0; s[1] += rd; s[2] += rd * rd; s[3] += pd; s[4] += pd * pd; s[5] += rd * pd;
  s[6] += rd * log(rd / pd) - rd + pd;                         // nmf_np.py:146-148 (0 log 0 is NaN there too)
  s[7] += (rd - pd) * (rd - pd);
}

// Block reduction of the eight sums in a fixed order; thread 0 writes out[0..7].
__device__ void np_block_stats(double* s, double* out) {
  __shared__ double red[kNpMaxWaves][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int v = 0; v < 8; ++v) s[v] = wave_sum(s[v]);
  if (lane == 0)
    for (int v = 0; v < 8; ++v) red[w][v] = s[v];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 0; v < 8; ++v) {
      double a = 0.0;
      for (int q = 0; q < nw; ++q) a += red[q][v];
      out[v] = a;
    }
  }
}

__host__ __device__ inline int np_row_blocks(int n, int RB) { return (n + RB - 1) / RB; }

// The half sweep of the RB rows from blockIdx.x * RB (both forms: many.h).
template <int E, int RB>
struct NpSweep {
  typedef NpSweepArgs Args;
  static constexpr int kThreads = 1024;
  static __host__ __device__ int blocks(const Args& a) { return np_row_blocks(a.n, RB); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int) {
    extern __shared__ float xs[];                               // [RB][K] the block's rows of X
    __shared__ float red[kNpMaxWaves][2 * RB];
    __shared__ float delta[RB];
    const int T = blockDim.x, t = threadIdx.x, lane = t & 63, w = t >> 6, nw = T >> 6;
    const int u0 = blockIdx.x * RB, K = a.K, m = a.m;
    float R[RB][E], P[RB][E], y[E];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = t + T * e;
        R[r][e] = (u0 + r < a.n && j < m) ? a.Rn[(size_t)(u0 + r) * m + j] : __builtin_nanf("");
        P[r][e] = 0.f;
      }
    for (int q = t; q < RB * K; q += T) {
      const int r = q / K, k = q - r * K;
      xs[q] = u0 + r < a.n ? a.Xt[(size_t)k * a.n + u0 + r] : 0.f;
    }
    __syncthreads();
    // P of the block's rows from X and Y
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int e = 0; e < E; ++e) { const int j = t + T * e; y[e] = j < m ? a.Yt[(size_t)k * m + j] : 0.f; }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const float x = xs[r * K + k];
#pragma unroll
        for (int e = 0; e < E; ++e) P[r][e] = fmaf(x, y[e], P[r][e]);
      }
    }
    // the columns k0 .. k1-1, in order
    for (int k = a.k0; k < a.k1; ++k) {
#pragma unroll
      for (int e = 0; e < E; ++e) { const int j = t + T * e; y[e] = j < m ? a.Yt[(size_t)k * m + j] : 0.f; }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const bool obs = R[r][e] == R[r][e];
          const float q = obs ? R[r][e] * __builtin_amdgcn_rcpf(P[r][e]) : 0.f;
          num = fmaf(y[e], q, num);
          den += obs ? y[e] : 0.f;
        }
        num = wave_sum(num); den = wave_sum(den);
        if (lane == 0) { red[w][2 * r] = num; red[w][2 * r + 1] = den; }
      }
      __syncthreads();
      if (t < RB) {
        float d = 0.f;
        if (u0 + t < a.n) {
          double nu = 0.0, de = 0.0;
          for (int q = 0; q < nw; ++q) { nu += (double)red[q][2 * t]; de += (double)red[q][2 * t + 1]; }
          const float x = xs[t * K + k];
          const float nx = (float)((double)x * nu / de);
          d = nx - x;
          xs[t * K + k] = nx;
        }
        delta[t] = d;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const float d = delta[r];
#pragma unroll
        for (int e = 0; e < E; ++e) P[r][e] = fmaf(d, y[e], P[r][e]);
      }
    }
    for (int q = t; q < RB * K; q += T) {
      const int r = q / K, k = q - r * K;
      if (u0 + r < a.n && k >= a.k0 && k < a.k1) a.Xt[(size_t)k * a.n + u0 + r] = xs[q];
    }
    if (a.stats) {                                              // the iteration's metrics from the final P
      double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (R[r][e] == R[r][e]) np_entry_stats(s, R[r][e], P[r][e]);
      np_block_stats(s, a.stats + (size_t)blockIdx.x * 8);
    }
  }
};

// Configuration of a half sweep over n units of inner extent m: E entries per thread and row, T threads, RB rows per block
// (E RB = 32 values of R and of P per thread; 16 for the longest rows, whose 1 024-thread blocks leave 128 registers a lane).
static void np_sweep_shape(int m, int* E, int* T, int* RB) {
  int e = 2;
  while (e < 16 && (m + e - 1) / e > 1024) e *= 2;
  *E = e;
  *T = ((m + e - 1) / e + 63) / 64 * 64;
  *RB = e == 16 ? 1 : 32 / e;
}

int np_sweep_blocks(int n, int m) {
  int E, T, RB;
  np_sweep_shape(m, &E, &T, &RB);
  return np_row_blocks(n, RB);
}

bool np_sweep_supported(int m, int K) {
  int E, T, RB;
  np_sweep_shape(m, &E, &T, &RB);
  return T <= 1024 && (size_t)RB * K * sizeof(float) <= 48 * 1024;
}

void launch_np_sweep(const NpSweepArgs& a, hipStream_t st) {
  int E, T, RB;
  np_sweep_shape(a.m, &E, &T, &RB);
  const size_t lds = (size_t)RB * a.K * sizeof(float);
  switch (E) {
    case 2: launch_forms<NpSweep<2, 16>>(a, st, T, lds); break;
    case 4: launch_forms<NpSweep<4, 8>>(a, st, T, lds); break;
    case 8: launch_forms<NpSweep<8, 4>>(a, st, T, lds); break;
    default: launch_forms<NpSweep<16, 1>>(a, st, T, lds); break;
  }
}

void launch_np_prepare(const float* R, const uint8_t* M, int I, int J, float* Rn, float* RnT, hipStream_t st) {
  dim3 g((J + 31) / 32, (I + 31) / 32);
  np_prepare_kernel<<<g, 256, 0, st>>>(R, M, I, J, Rn, RnT);
}

// out[8] = sums over the nb rows of part[nb][8], each in a fixed order (one block).
__device__ __forceinline__ void np_stats_finish_body(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double red[256];
  for (int v = 0; v < 8; ++v) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += part[(size_t)b * 8 + v];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[v] = red[0];
    __syncthreads();
  }
}
// (out = the run's FIRST record, the iteration's one is `it` records behind it: a recorded argument list stays the same)
struct NpStatsFinish {
  struct Args { const double* part; double* out; int nb, pad; };
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args&) { return 1; }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int it) { np_stats_finish_body(a.part, a.nb, a.out + (size_t)it * 8); }
};

void launch_np_stats_finish(const double* part, int nb, double* out, hipStream_t st) {
  NpStatsFinish::Args a; memset(&a, 0, sizeof(a));
  a.part = part; a.out = out; a.nb = nb;
  launch_forms<NpStatsFinish>(a, st);
}

// out[c][x] = sum_a S[c sc + a sa] in[a][x]  (c < C, a < A, x < n): G S^T as [K][J] (sc = L, sa = 1) or (F S)^T as [L][I]
// (sc = 1, sa = L).  S is [K][L] row major.
__device__ __forceinline__ void np_small_product_body(const float* __restrict__ S, int sc, int sa, const float* __restrict__ in,
                                                      int A, int C, int n, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)C * n) return;
  const int c = (int)(idx / n), x = (int)(idx - (size_t)c * n);
  float s = 0.f;
  for (int q = 0; q < A; ++q) s = fmaf(S[c * sc + q * sa], in[(size_t)q * n + x], s);
  out[idx] = s;
}
struct NpSmallProduct {
  struct Args { const float* S; const float* in; float* out; int sc, sa, A, C, n, pad; };
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args& a) { return (int)(((size_t)a.C * a.n + 255) / 256); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int) { np_small_product_body(a.S, a.sc, a.sa, a.in, a.A, a.C, a.n, a.out); }
};

void launch_np_small_product(const float* S, int sc, int sa, const float* in, int A, int C, int n, float* out, hipStream_t st) {
  NpSmallProduct::Args a; memset(&a, 0, sizeof(a));
  a.S = S; a.in = in; a.out = out; a.sc = sc; a.sa = sa; a.A = A; a.C = C; a.n = n;
  launch_forms<NpSmallProduct>(a, st);
}

// P[i][j] = sum_k Ut[k][i] Yt[k][j] on the observed entries (NMTF's S step keeps P in memory).
__device__ __forceinline__ void np_build_p_body(const float* __restrict__ Rn, const float* __restrict__ Ut, const float* __restrict__ Yt,
                                                int I, int J, int K, float* __restrict__ P, int i, int j) {
  if (j >= J) return;
  const size_t o = (size_t)i * J + j;
  const float r = Rn[o];
  if (!(r == r)) return;
  float s = 0.f;
  for (int k = 0; k < K; ++k) s = fmaf(Ut[(size_t)k * I + i], Yt[(size_t)k * J + j], s);
  P[o] = s;
}
// A one-dimensional grid of I row groups of (J + 255) / 256 blocks each (the models of a launch differ in I and J).
struct NpBuildP {
  struct Args { const float* Rn; const float* Ut; const float* Yt; float* P; int I, J, K, pad; };
  static constexpr int kThreads = 256;
  static __host__ __device__ int row_blocks(const Args& a) { return (a.J + 255) / 256; }
  static __host__ __device__ int blocks(const Args& a) { return a.I * row_blocks(a); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int) {
    const int bj = row_blocks(a), i = (int)blockIdx.x / bj, jb = (int)blockIdx.x - i * bj;
    np_build_p_body(a.Rn, a.Ut, a.Yt, a.I, a.J, a.K, a.P, i, jb * 256 + threadIdx.x);
  }
};

void launch_np_build_p(const float* Rn, const float* Ut, const float* Yt, int I, int J, int K, float* P, hipStream_t st) {
  NpBuildP::Args a; memset(&a, 0, sizeof(a));
  a.Rn = Rn; a.Ut = Ut; a.Yt = Yt; a.P = P; a.I = I; a.J = J; a.K = K;
  launch_forms<NpBuildP>(a, st);
}

// One pass of NMTF's S step (nmtf_np.py:169-174).  A pass first finishes entry `prev` (if >= 0) -- every block sums the previous
// pass's block partials in the same order, so all agree on its new value -- and moves P by dS F[:, k'] G[:, l']^T, then
// accumulates entry `cur`'s (if >= 0) numerator sum F_ik G_jl R_ij / P_ij and denominator sum F_ik G_jl over the observed entries.
// S_in holds the values at the start of the step (read only); S_out receives each entry as it is finished.
// (nb: the pass's block count np_s_blocks(I) -- the stride of the rows and the number of partials)
struct NpSPass {
  typedef NpSPassArgs Args;
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args& a) { return np_s_blocks(a.I); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int nb, int) {
    __shared__ double red[256][2];
    __shared__ float s_delta;
    const int t = threadIdx.x;
    const int I = a.I, J = a.J;
    const int kp = a.prev >= 0 ? a.prev / a.L : 0, lp = a.prev >= 0 ? a.prev % a.L : 0;
    if (a.prev >= 0) {
      double nu = 0.0, de = 0.0;
      for (int b = t; b < nb; b += 256) { nu += a.part_prev[(size_t)b * 2]; de += a.part_prev[(size_t)b * 2 + 1]; }
      red[t][0] = nu; red[t][1] = de;
      __syncthreads();
      for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { red[t][0] += red[t + h][0]; red[t][1] += red[t + h][1]; }
        __syncthreads();
      }
      if (t == 0) {
        const float s0 = a.S_in[a.prev];
        const float s1 = (float)((double)s0 * red[0][0] / red[0][1]);
        s_delta = s1 - s0;
        if (blockIdx.x == 0) a.S_out[a.prev] = s1;
      }
      __syncthreads();
    }
    const float d = a.prev >= 0 ? s_delta : 0.f;
    if (a.cur < 0) {                                            // only the change of entry prev
      for (int i = blockIdx.x; i < I; i += nb) {
        const float fp = d * a.Ft[(size_t)kp * I + i];
        for (int j = t; j < J; j += 256) {
          const size_t o = (size_t)i * J + j;
          const float r = a.Rn[o];
          if (r == r) a.P[o] = fmaf(fp, a.Gt[(size_t)lp * J + j], a.P[o]);
        }
      }
      return;
    }
    const int k = a.cur / a.L, l = a.cur % a.L;
    float nu = 0.f, de = 0.f;
    for (int i = blockIdx.x; i < I; i += nb) {
      const float fp = d * a.Ft[(size_t)kp * I + i], fk = a.Ft[(size_t)k * I + i];
      for (int j = t; j < J; j += 256) {
        const size_t o = (size_t)i * J + j;
        const float r = a.Rn[o];
        if (!(r == r)) continue;
        float p = a.P[o];
        if (a.prev >= 0) { p = fmaf(fp, a.Gt[(size_t)lp * J + j], p); a.P[o] = p; }
        const float wgt = fk * a.Gt[(size_t)l * J + j];
        nu = fmaf(wgt, r * __builtin_amdgcn_rcpf(p), nu);
        de += wgt;
      }
    }
    __syncthreads();                                            // (red is reused)
    red[t][0] = nu; red[t][1] = de;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (t < h) { red[t][0] += red[t + h][0]; red[t][1] += red[t + h][1]; }
      __syncthreads();
    }
    if (t == 0) { a.part_cur[(size_t)blockIdx.x * 2] = red[0][0]; a.part_cur[(size_t)blockIdx.x * 2 + 1] = red[0][1]; }
  }
};

void launch_np_s_pass(const NpSPassArgs& a, hipStream_t st) { launch_forms<NpSPass>(a, st); }

// dst[0 .. n) = src[0 .. n): the list form of the S step's device-to-device copy (a copy cannot be recorded)
struct NpCopyPack { const float* src; float* dst; int n, pad; };
__global__ __launch_bounds__(256) void np_copy_many(const NpCopyPack* list, int) {
  const NpCopyPack p = load_pack(list, blockIdx.z);
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < p.n) p.dst[q] = p.src[q];
}

void record_np_copy(const float* src, float* dst, int n) {
  NpCopyPack p; memset(&p, 0, sizeof(p));
  p.src = src; p.dst = dst; p.n = n;
  record_launch((const void*)np_copy_many, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p, true);
}

// The eight sums of predict() / compute_I_div() for P = Ut^T Yt on the entries of a mask (fp64 per entry; one block per row).
__global__ __launch_bounds__(256) void np_metrics_kernel(const float* __restrict__ R, const uint8_t* __restrict__ M, const float* __restrict__ Ut,
                                                         const float* __restrict__ Yt, int I, int J, int K, double* __restrict__ part) {
  const int i = blockIdx.x;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = threadIdx.x; j < J; j += 256) {
    const size_t o = (size_t)i * J + j;
    if (!M[o]) continue;
    float p = 0.f;
    for (int k = 0; k < K; ++k) p = fmaf(Ut[(size_t)k * I + i], Yt[(size_t)k * J + j], p);
    np_entry_stats(s, R[o], p);
  }
  np_block_stats(s, part + (size_t)i * 8);
}

void launch_np_metrics(const float* R, const uint8_t* M, const float* Ut, const float* Yt, int I, int J, int K, double* part, hipStream_t st) {
  np_metrics_kernel<<<I, 256, 0, st>>>(R, M, Ut, Yt, I, J, K, part);
}

}  // namespace bnmtf
