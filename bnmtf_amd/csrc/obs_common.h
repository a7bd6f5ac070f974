// What the observed-entry layout's translation units share (DESIGN.md sections 2.7 and 2.10).  Users: kernel_obs.hip (Gibbs / ICM,
// and the tri-factorisation's F and G sweeps), kernel_obs_vb.hip (the variational models of both factorisations), kernel_obs_np.hip
// (NMF / NMTF), kernel_foldin.hip (fold-in: the butterfly and the residual; its loops are its own), kernel_obs_heldout.hip,
// kernel_obs_tri.hip and kernel_obs_trivb.hip.
//
// The sweep kernels (obs_sweep_kernel, obs_vb_sweep_kernel / obs_trivb_sweep_kernel, onp_sweep_kernel) have one
// skeleton: one 64-lane wave per unit, lane l the unit's entries l, l + 64, ... in list order; the unit's row (and prior rates) in
// the wave's LDS row (obs_stage_row), read by broadcast; the form chosen by the unit's entry count (obs_count, obs_dispatch); the
// per-entry loops written once on ObsForm<S>; per-lane sums in entry order, the butterfly over the wave (wave_sum / wave_sum_d:
// every lane ends with the same bits), the block's waves in wave order (obs_block_sums), the blocks' partials in obs_fold's order.
// No floating-point atomics anywhere.
//
// The two forms of a unit -- the contract.  A quantity per entry (the residual e; NMF's product P) lives through the unit's column
// loop.  The REGISTER form (S = 1, 2, 4, 8 slots per lane, a unit of at most S x 64 entries) keeps it, the entry's inner index and
// the last value gathered for it in registers.  A slot without an entry holds the inner index m, where every transposed operand
// keeps a zero word behind its columns (ld > m), and a neutral e (0 for the residual, 1 for P, with r = 0): it gathers v = 0 and adds
// +0 to sums that are never -0, so no per-slot predicate lives across the column loop.  The LONG form (S = 0, any length) keeps e in
// a global scratch array at the entry's own list position and gathers index and v again.  A body handed to each() runs on both:
// the same operations on the same operands in the same order (explicit fmaf, contraction off), so a unit's bits do not depend on the
// form -- force_long in the argument structs sends every unit down the long one, and the suites compare the two byte for byte.
#pragma once
#include "kernels.h"

namespace bnmtf {

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// x . Xo_j, the columns in order (the padding columns of both are zero), and r less that
__device__ __forceinline__ float obs_dot(const float* xs, const float* Xo, int KP, uint32_t j) {
#pragma clang fp contract(off)
  const float4* row = reinterpret_cast<const float4*>(Xo + (size_t)j * KP);
  float acc = 0.f;
  for (int q = 0; q < KP / 4; ++q) {
    const float4 b = row[q];
    acc = fmaf(xs[4 * q + 0], b.x, acc); acc = fmaf(xs[4 * q + 1], b.y, acc);
    acc = fmaf(xs[4 * q + 2], b.z, acc); acc = fmaf(xs[4 * q + 3], b.w, acc);
  }
  return acc;
}
__device__ __forceinline__ float obs_residual(const float* xs, const float* Xo, int KP, uint32_t j, float r) {
  return r - obs_dot(xs, Xo, KP, j);
}

// One unit in one of its two forms (the contract: this file's header).  S > 0: the register form with S slots per lane; S == 0:
// the long form.  Bodies take (s, t): the lane's slot and the entry's position in the unit's list.
template <int S>
struct ObsForm {
  static constexpr int N = S > 0 ? S : 1;
  const uint32_t* idx;
  const float* val;
  float* es;
  uint32_t cnt;
  int lane;
  float e[N], v[N], r[N];        // (register form only; what a kernel does not use costs nothing)
  uint32_t jj[N];

  __device__ __forceinline__ ObsForm(const uint32_t* ptr, const uint32_t* idx_, const float* val_, float* escratch, int u, int lane_) {
    const uint32_t beg = ptr[u];
    idx = idx_ + beg; val = val_ + beg; es = escratch + beg; cnt = ptr[u + 1] - beg; lane = lane_;
  }
  // register form: f(s, s * 64 + lane) for every slot of the lane, unrolled -- t may lie behind the unit's last entry: has(t);
  // long form: f(0, t) for every entry t of the lane
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    if constexpr (S > 0) {
#pragma unroll
      for (int s = 0; s < S; ++s) f(s, (uint32_t)(s * 64 + lane));
    } else {
      for (uint32_t t = (uint32_t)lane; t < cnt; t += 64) f(0, t);
    }
  }
  __device__ __forceinline__ bool has(uint32_t t) const { return S > 0 ? t < cnt : true; }
  // every slot of the lane: its entry's index and value, or the empty slot -- index m, e = e0, r = 0, v = 0
  __device__ __forceinline__ void init(uint32_t m, float e0) {
    if constexpr (S > 0) {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const uint32_t t = (uint32_t)(s * 64 + lane);
        e[s] = e0; v[s] = 0.f; jj[s] = m; r[s] = 0.f;
        if (t < cnt) { jj[s] = idx[t]; r[s] = val[t]; }
      }
    }
  }
  __device__ __forceinline__ float& E(int s, uint32_t t) { return S > 0 ? e[s] : es[t]; }
  __device__ __forceinline__ uint32_t J(int s, uint32_t t) const { return S > 0 ? jj[s] : idx[t]; }
  __device__ __forceinline__ float R(int s, uint32_t t) const { return S > 0 ? r[s] : val[t]; }       // (val[t] itself: no register held)
  // the value gathered for the entry: kept by the register form from the column's sums to its update, gathered again by the long one
  __device__ __forceinline__ float hold(int s, float x) { if (S > 0) v[s] = x; return x; }
  __device__ __forceinline__ float V(int s, uint32_t t, const float* col) const { return S > 0 ? v[s] : col[idx[t]]; }
  // e from and to its scratch word, where the long form has it anyway (a launch handing e to the next one)
  __device__ __forceinline__ void from_scratch() {
    if constexpr (S > 0) each([&](int s, uint32_t t) __attribute__((always_inline)) { if (t < cnt) e[s] = es[t]; });
  }
  __device__ __forceinline__ void to_scratch() {
    if constexpr (S > 0) each([&](int s, uint32_t t) __attribute__((always_inline)) { if (t < cnt) es[t] = e[s]; });
  }
};

// the unit's entry count, wave-uniform
__device__ __forceinline__ uint32_t obs_count(const uint32_t* ptr, int u) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(ptr[u + 1] - ptr[u]));
}

// f(ObsSlots<S>()) with the form of a unit of cnt entries: S = 1, 2, 4, 8 slots by the count, the long form (S = 0) behind
// MAXS x 64 entries or when forced
template <int S> struct ObsSlots { static constexpr int value = S; };
template <int MAXS, class F>
__device__ __forceinline__ void obs_dispatch(uint32_t cnt, int force_long, F&& f) {
  static_assert(MAXS == 8, "the ladder ends at 8 slots");
  if (force_long || cnt > (uint32_t)MAXS * 64u) f(ObsSlots<0>());
  else if (cnt <= 64u) f(ObsSlots<1>());
  else if (cnt <= 128u) f(ObsSlots<2>());
  else if (cnt <= 256u) f(ObsSlots<4>());
  else f(ObsSlots<8>());
}

// src[0 .. n) into the wave's LDS row dst[0 .. np), the padding columns as zeros
__device__ __forceinline__ void obs_stage_row(float* dst, const float* src, int n, int np, int lane) {
  for (int k = lane; k < np; k += 64) dst[k] = k < n ? src[k] : 0.f;
}

// The block's sums of the lanes' s[0 .. nsum): the butterfly, then the NW waves in wave order.  Thread m < nsum gets sum m, every
// other thread 0.  Every wave of the block calls it (a barrier inside).
template <int W, int NW>
__device__ __forceinline__ double obs_block_sums(double (&s)[W], int nsum) {
  __shared__ double red[NW][W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < W; ++m)
    if (m < nsum) s[m] = wave_sum_d(s[m]);
  if (lane == 0)
    for (int m = 0; m < W; ++m) red[wave][m] = s[m];
  __syncthreads();
  double t = 0.0;
  if ((int)threadIdx.x < nsum)
    for (int w = 0; w < NW; ++w) t += red[w][threadIdx.x];
  return t;
}

// The sums over a 256-thread block of the threads' s[0 .. W), by a tree: halves from 128 down.  Every thread gets all of them.
template <int W>
__device__ __forceinline__ void obs_tree_sums(double (&s)[W]) {
  __shared__ double red[W][256];
  const int tid = threadIdx.x;
  for (int m = 0; m < W; ++m) red[m][tid] = s[m];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) for (int m = 0; m < W; ++m) red[m][tid] += red[m][tid + w];
    __syncthreads();
  }
  for (int m = 0; m < W; ++m) s[m] = red[m][0];
}

// column sums of part[nb][W] (W <= 8) in a fixed order: thread t the rows t, t + 256, ..., then the tree
template <int W>
__device__ __forceinline__ void obs_fold(const double* part, int nb, double (&out)[W]) {
  for (int m = 0; m < W; ++m) out[m] = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256)
    for (int m = 0; m < W; ++m) out[m] += part[(size_t)b * W + m];
  obs_tree_sums<W>(out);
}
// ... into out[0 .. W): a launch of one block (instantiated where it is launched)
template <int W>
__global__ __launch_bounds__(256) void obs_fold_kernel(const double* part, int nb, double* out) {
  double t[W];
  obs_fold<W>(part, nb, t);
  if (threadIdx.x == 0)
    for (int m = 0; m < W; ++m) out[m] = t[m];
}

}  // namespace

}  // namespace bnmtf
