// What the observed-entry layout's translation units share (kernel_obs.hip: Gibbs / ICM; kernel_obs_vb.hip: variational): the
// wave butterflies, the residual of an entry from whole factor rows and the fixed-order fold of the blocks' partial sums.
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

// r - x . Xo_j, the columns in order (the padding columns of both are zero)
__device__ __forceinline__ float obs_residual(const float* xs, const float* Xo, int KP, uint32_t j, float r) {
#pragma clang fp contract(off)
  const float4* row = reinterpret_cast<const float4*>(Xo + (size_t)j * KP);
  float acc = 0.f;
  for (int q = 0; q < KP / 4; ++q) {
    const float4 b = row[q];
    acc = fmaf(xs[4 * q + 0], b.x, acc); acc = fmaf(xs[4 * q + 1], b.y, acc);
    acc = fmaf(xs[4 * q + 2], b.z, acc); acc = fmaf(xs[4 * q + 3], b.w, acc);
  }
  return r - acc;
}

// column sums of part[nb][W] (W <= 8) in a fixed order: thread t the rows t, t + 256, ..., then a tree; out[m] valid in thread 0
template <int W>
__device__ __forceinline__ void obs_fold(const double* part, int nb, double* out) {
  __shared__ double red[W][256];
  const int tid = threadIdx.x;
  double s[W];
  for (int m = 0; m < W; ++m) s[m] = 0.0;
  for (int b = tid; b < nb; b += 256)
    for (int m = 0; m < W; ++m) s[m] += part[(size_t)b * W + m];
  for (int m = 0; m < W; ++m) red[m][tid] = s[m];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) for (int m = 0; m < W; ++m) red[m][tid] += red[m][tid + w];
    __syncthreads();
  }
  for (int m = 0; m < W; ++m) out[m] = red[m][0];
}

}  // namespace

}  // namespace bnmtf
