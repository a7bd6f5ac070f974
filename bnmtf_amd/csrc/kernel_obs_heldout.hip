// Held-out performance per iteration on the observed-entry layout (run(M_test=Entries)): the six sums that
// metrics_from_sums finishes -- n, sum R, sum R^2, sum P, sum P^2, sum R P -- of the handle's own factors over a row-sorted list
// of held-out entries.  One launch pair per iteration (this kernel, then kernel_heldout.hip's fold), enqueued behind the
// iteration's finish kernel on the handle's stream.
//
// Operands: the two-factor handle's row-major fp32 factors, rows.X [I][stride] and cols.X [J][stride], stride = K rounded up to 4,
// K <= kObsMaxRank (for the variational model: the expectations).  Neither kernel of kernel_heldout.hip reads them: Heldout
// is tied to a row stride of 32 or 64, HeldoutNp to column-major factors.
//
// Layout, as heldout_np_body's.  A wave owns one row i (kObsHeldoutRows consecutive rows per block, heldout_blocks(I) blocks: no
// grid stride).  The row's factor row is staged once in LDS as doubles ([4][256], 8 KiB) and read by broadcast: every lane of a
// wave reads the same address in the same instruction, which the LDS serves as one access whatever the width.  The lanes run along
// the row's entries -- lane l takes entries beg + l, beg + l + 64, ... -- and each walks row j of the other factor with 16-byte
// loads (aligned: the stride is a multiple of 4 floats); the first load of a row brings its line, the following ones hit it.
// P_ij is the fp64 fma chain over k = 0 .. K - 1 in column order; the padding columns take no part, whatever they hold.  Column
// index and value of the lane's next entry are fetched before the current entry's arithmetic.
//
// Order of the sums (fixed: two runs give the same bits, no floating-point atomics): a lane's entries in list order; a butterfly
// over the wave; the block's waves in wave order; HeldoutFold (launch_fold) over the blocks' partials.
#include "obs_common.h"

namespace bnmtf {

namespace {

__global__ __launch_bounds__(256) void obs_heldout_kernel(ObsHeldoutArgs a) {
  __shared__ __attribute__((aligned(16))) double rowf[kObsHeldoutRows][kObsMaxRank];     // the waves' factor rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kObsHeldoutRows + wave;
  const bool row_ok = i < a.I;
  double* const mine = rowf[wave];

  // ---- the row's factor row, fp64, lanes along its columns
  if (row_ok)
    for (int k = lane; k < a.K; k += 64) mine[k] = (double)a.A[(size_t)i * a.stride + k];
  __syncthreads();

  // ---- the row's entries, 64 per step
  const uint32_t beg = row_ok ? a.rowptr[i] : 0u, end = row_ok ? a.rowptr[i + 1] : 0u;
  const int K4 = a.K >> 2, rem = a.K & 3;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t e = beg + (uint32_t)lane;
  bool live = e < end;
  uint32_t j = live ? a.col[e] : 0u;
  float r32 = live ? a.rval[e] : 0.f;
  for (uint32_t base = beg; base < end; base += kObsHeldoutStep) {
    const float4* brow = reinterpret_cast<const float4*>(a.B + (size_t)j * a.stride);      // (a lane without an entry reads row 0: J >= 1)
    const uint32_t en = e + kObsHeldoutStep;
    const bool ln = en < end;
    const uint32_t jn = ln ? a.col[en] : 0u;
    const float rn = ln ? a.rval[en] : 0.f;
    double p = 0.0;
#pragma unroll 2
    for (int q = 0; q < K4; ++q) {
      const float4 b = brow[q];
      const double2 m01 = *reinterpret_cast<const double2*>(mine + 4 * q);
      const double2 m23 = *reinterpret_cast<const double2*>(mine + 4 * q + 2);
      p = fma(m01.x, (double)b.x, p); p = fma(m01.y, (double)b.y, p);
      p = fma(m23.x, (double)b.z, p); p = fma(m23.y, (double)b.w, p);
    }
    if (rem) {                           // the last columns: the stride's padding behind them takes no part
      const float4 b = brow[K4];
      p = fma(mine[4 * K4], (double)b.x, p);
      if (rem > 1) p = fma(mine[4 * K4 + 1], (double)b.y, p);
      if (rem > 2) p = fma(mine[4 * K4 + 2], (double)b.z, p);
    }
    if (live) {
      const double r = (double)r32;
      s[0] += 1.0; s[1] += r; s[2] = fma(r, r, s[2]); s[3] += p; s[4] = fma(p, p, s[4]); s[5] = fma(r, p, s[5]);
    }
    e = en; live = ln; j = jn; r32 = rn;
  }

  // ---- wave, then block
  const double v = obs_block_sums<6, kObsHeldoutRows>(s, 6);
  if (threadIdx.x < 8) a.part[(size_t)blockIdx.x * 8 + threadIdx.x] = v;           // (0 in the two words of padding)
}

}  // namespace

void launch_obs_heldout(const ObsHeldoutArgs& a, hipStream_t st) {
  const int nb = heldout_blocks(a.I);
  hipLaunchKernelGGL(obs_heldout_kernel, dim3(nb), dim3(256), 0, st, a);
  launch_fold(a.part, nb, a.rec, st);
}

}  // namespace bnmtf
