// Fold new units into a fitted model: the conditional of one factor row given the OTHER factor, which stays
// fixed -- phase 2 of obs_unit (kernel_obs.hip) restated.  With the other factor fixed the new units are independent of each other
// along the whole chain, so a unit's chain lives in one wave of one launch: no return to the host between sweeps.  With Omega the
// unit's entries, e_j = r_j - x . B_j, for t = 0 .. T - 1 and then k = 0 .. W - 1:
//   a_k = sum_{j in Omega} B_jk^2,   s_k = sum_{j in Omega} e_j B_jk
//   tau_p = tau a_k,   numer = -lambda_k + tau (s_k + x_k a_k),   mu = numer / tau_p
//   x' = draw / max(max(0, mu), min_x);   e_j -= (x' - x_k) B_jk
// foldin_kernel: one 64-lane wave per unit, kFoldInWaves units per block; lane l owns the unit's entries l, l + 64, ... in list
// order.  The unit's x, lambda and a sit in LDS (3 x 1 KiB per wave) and are read by broadcast; its statistics sit there in fp64
// (3 x 2 KiB per wave).
//   Once     a_k for every column: gather v = XoT[k][j], per-lane fp32 partials of sum v^2 in entry order, a butterfly over the wave.
//   Sweep t  e = r - x . Xo_j for every entry from whole rows of the fixed factor (row major [m][KP], float4 loads): the residual is
//            rebuilt at every sweep, as obs_sweep_kernel rebuilds it at every half sweep, so the bound on mu of one half sweep holds
//            for every sweep of the chain.  Then per column: gather v, partials of sum e v in entry order, the butterfly (every lane
//            ends with the same bits), the wave-uniform conditional, the candidates of a draw 64 at a time across the lanes -- Philox
//            counter (id, column, it0 + t, kStreamFoldIn | candidate), key = seed, first accepted candidate: oracle/rng.py's chain --
//            then e -= delta v.  A kept sweep adds x to the statistics, lane l those of columns l, l + 64, l + 128, l + 192, in fp64:
//            the first kept x, sum d and sum d^2 with d = x - first (exact in fp64), in sweep order (kernel_predictive.hip's shifted
//            form; the host makes the two divisions).  The sweep's x goes to samples[t][u][.] when asked for, lanes along k.
// Two forms of the same arithmetic, under obs_common.h's contract, in this file's own loops (written on ObsForm the kernel took
// 128 / 120 VGPRs for 126 / 118 and ran 2 to 3 % longer on batches of 1 and 256 units; the draw loop is this file's own too).  A unit of at most kFoldInMaxSlots x 64 entries keeps e, j and v in
// registers: S slots per lane, S = 1, 2, 4, 8 by the unit's entry count (wave-uniform).  A slot without an entry holds e = 0 and the
// index m, where the transposed factor keeps a zero behind every column (ldT > m): it adds +0 to sums that are never -0.  A longer
// unit keeps e in a global scratch array at the entry's own list position and gathers j and v again.  Both run the same operations
// on the same operands in the same order (explicit fmaf, contraction off), so a unit's bits do not depend on the form
// (FoldInArgs::force_long sends every unit down the long one) -- nor on the batch or the unit's place in it: nothing is shared
// between units, and nothing is summed across them.  Nothing here is read-modify-written by more than one wave.
#include "obs_common.h"
#include "device_rng.h"

namespace bnmtf {

namespace {

// One unit, all its sweeps.  S > 0: the register form with S slots per lane; S == 0: the long form.  xs / ls / as: the unit's factor
// row, prior rates and a in LDS; st: its statistics there, [3][kFoldInMaxRank] -- first, sum d, sum d^2.
template <int S, int MODE>
__device__ __forceinline__ void foldin_unit(const FoldInArgs& a, int u, int lane, float* xs, const float* ls, float* as, double* st) {
#pragma clang fp contract(off)
  constexpr int SS = S > 0 ? S : 1;
  const uint32_t beg = a.ptr[u], cnt = a.ptr[u + 1] - beg;
  const uint32_t* idx = a.idx + beg;
  const float* val = a.val + beg;
  float* es = a.escratch + beg;
  const int W = a.W, KP = a.KP;
  // (the unit's id and the key in vector registers: as wave-uniform values the compiler keeps them, and the ten round keys of Philox,
  // in scalar registers across the loops, more than there are -- kernel_obs.hip, the same place)
  uint32_t elem = a.ids[u], k0 = a.key0, k1 = a.key1;
  asm volatile("" : "+v"(elem), "+v"(k0), "+v"(k1));
  const float tau = a.tau;
  float e[SS], v[SS];
  uint32_t jj[SS];

  if (S > 0) {
#pragma unroll
    for (int s = 0; s < SS; ++s) {
      const uint32_t t = (uint32_t)(s * 64 + lane);
      jj[s] = (uint32_t)a.m; e[s] = 0.f; v[s] = 0.f;    // (a slot without an entry: the zero word behind the fixed factor's columns)
      if (t < cnt) jj[s] = idx[t];
    }
  }

  // ---- once: a_k of every column
#pragma unroll 1
  for (int k = 0; k < W; ++k) {
    const float* vcol = a.XoT + (size_t)k * a.ldT;
    float sa = 0.f;
    if (S > 0) {
#pragma unroll
      for (int s = 0; s < SS; ++s) { const float vv = vcol[jj[s]]; sa = fmaf(vv, vv, sa); }
    } else {
      for (uint32_t t = (uint32_t)lane; t < cnt; t += 64) { const float vv = vcol[idx[t]]; sa = fmaf(vv, vv, sa); }
    }
    sa = wave_sum(sa);
    as[k] = sa;                                   // (every lane stores the same value)
  }

  int next_keep = a.discard;

#pragma unroll 1
  for (int t = 0; t < a.T; ++t) {
    // ---- the residual of every entry, from x as it stands
    if (S > 0) {
      // (obs_residual's chain for every slot, four columns of all slots at a time: a slot without an entry reads row 0 and keeps its 0)
      float acc[SS];
#pragma unroll
      for (int s = 0; s < SS; ++s) acc[s] = 0.f;
#pragma unroll 1
      for (int q = 0; q < KP / 4; ++q) {
        const float x0 = xs[4 * q + 0], x1 = xs[4 * q + 1], x2 = xs[4 * q + 2], x3 = xs[4 * q + 3];
#pragma unroll
        for (int s = 0; s < SS; ++s) {
          const float4 b = reinterpret_cast<const float4*>(a.Xo + (size_t)((uint32_t)(s * 64 + lane) < cnt ? jj[s] : 0u) * KP)[q];
          acc[s] = fmaf(x0, b.x, acc[s]); acc[s] = fmaf(x1, b.y, acc[s]);
          acc[s] = fmaf(x2, b.z, acc[s]); acc[s] = fmaf(x3, b.w, acc[s]);
        }
      }
#pragma unroll
      for (int s = 0; s < SS; ++s) e[s] = (uint32_t)(s * 64 + lane) < cnt ? val[s * 64 + lane] - acc[s] : 0.f;
    } else {
#pragma unroll 1
      for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) es[i] = obs_residual(xs, a.Xo, KP, idx[i], val[i]);
    }

    // ---- the columns
#pragma unroll 1
    for (int k = 0; k < W; ++k) {
      const float* vcol = a.XoT + (size_t)k * a.ldT;
      float se = 0.f;
      if (S > 0) {
#pragma unroll
        for (int s = 0; s < SS; ++s) {
          // (opaque here: otherwise the 64-bit offsets of every slot, the same in all sweeps, are kept in registers across the draws)
          asm volatile("" : "+v"(jj[s]));
          v[s] = vcol[jj[s]]; se = fmaf(e[s], v[s], se);
        }
      } else {
        for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) se = fmaf(es[i], vcol[idx[i]], se);
      }
      se = wave_sum(se);
      const float sa = as[k];
      const float xk = xs[k];
      const float num = fmaf(xk, sa, se);
      const float tau_p = tau * sa;
      const float numer = fmaf(tau, num, -ls[k]);
      const float mu = numer / tau_p;
      float xnew = 0.f;
      if (MODE == kSweepDraw) {
        const TnParams tp = tn_params(mu, tau_p);
        uint32_t itw = a.it0 + (uint32_t)t;
        asm volatile("" : "+v"(itw));
        if (tp.live) {
#pragma unroll 1
          for (uint32_t round = 0; round < 64u; ++round) {
            float xc;
            const bool acc = tn_candidate(tp, elem, (uint32_t)k, itw, kStreamFoldIn, round * 64u + (uint32_t)lane, k0, k1, &xc);
            const unsigned long long m = __ballot(acc);
            if (m) { xnew = tn_guard(__shfl(xc, __ffsll((long long)m) - 1, 64)); break; }
          }
        }
      } else {
        xnew = fmaxf((tau_p > 0.f && mu > 0.f) ? mu : 0.f, a.min_x);
      }
      const float nd = xk - xnew;                 // e -= (x' - x) v
      xs[k] = xnew;                               // (every lane stores the same value, and reads back its own store)
      if (S > 0) {
#pragma unroll
        for (int s = 0; s < SS; ++s) e[s] = fmaf(nd, v[s], e[s]);
      } else {
        for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) es[i] = fmaf(nd, vcol[idx[i]], es[i]);
      }
    }

    // ---- the sweep's x: the sample slot and, for a kept sweep, the statistics
    if (a.samples) {
      float* out = a.samples + ((size_t)t * a.n + u) * W;
      for (int k = lane; k < W; k += 64) out[k] = xs[k];
    }
    if (t == next_keep) {                         // (wave-uniform)
      next_keep += a.keep_every;
      for (int k = lane; k < W; k += 64) {
        const double x = (double)xs[k];
        if (t == a.discard) { st[k] = x; st[kFoldInMaxRank + k] = 0.0; st[2 * kFoldInMaxRank + k] = 0.0; }
        else { const double d = x - st[k]; st[kFoldInMaxRank + k] += d; st[2 * kFoldInMaxRank + k] = fma(d, d, st[2 * kFoldInMaxRank + k]); }
      }
    }
  }

  const size_t nW = (size_t)a.n * W;
  for (int k = lane; k < W; k += 64) {
    const size_t o = (size_t)u * W + k;
    a.stats[o] = st[k]; a.stats[nW + o] = st[kFoldInMaxRank + k]; a.stats[2 * nW + o] = st[2 * kFoldInMaxRank + k];
  }
}

template <int MODE>
__global__ __launch_bounds__(kFoldInWaves * 64) void foldin_kernel(FoldInArgs a) {
  __shared__ float xsh[kFoldInWaves][kFoldInMaxRank];
  __shared__ float lsh[kFoldInWaves][kFoldInMaxRank];
  __shared__ float ash[kFoldInWaves][kFoldInMaxRank];
  __shared__ double ssh[kFoldInWaves][3 * kFoldInMaxRank];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * kFoldInWaves + wave;
  const bool ok = u < a.n;
  float* xs = xsh[wave];
  float* ls = lsh[wave];
  if (ok)
    for (int k = lane; k < a.KP; k += 64) {
      xs[k] = k < a.W ? a.init[(size_t)u * a.W + k] : 0.f;
      ls[k] = k < a.W ? a.lambda[(size_t)u * a.W + k] : 0.f;
    }
  __syncthreads();
  if (!ok) return;
  const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.ptr[u + 1] - a.ptr[u]));
  if (a.force_long || cnt > (uint32_t)kFoldInMaxSlots * 64u) foldin_unit<0, MODE>(a, u, lane, xs, ls, ash[wave], ssh[wave]);
  else if (cnt <= 64u) foldin_unit<1, MODE>(a, u, lane, xs, ls, ash[wave], ssh[wave]);
  else if (cnt <= 128u) foldin_unit<2, MODE>(a, u, lane, xs, ls, ash[wave], ssh[wave]);
  else if (cnt <= 256u) foldin_unit<4, MODE>(a, u, lane, xs, ls, ash[wave], ssh[wave]);
  else foldin_unit<8, MODE>(a, u, lane, xs, ls, ash[wave], ssh[wave]);
}

}  // namespace

void launch_foldin(const FoldInArgs& a, hipStream_t st) {
  const dim3 grid(foldin_blocks(a.n)), block(kFoldInWaves * 64);
  if (a.mode == kSweepDraw) hipLaunchKernelGGL(foldin_kernel<kSweepDraw>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(foldin_kernel<kSweepMode>, grid, block, 0, st, a);
}

}  // namespace bnmtf
