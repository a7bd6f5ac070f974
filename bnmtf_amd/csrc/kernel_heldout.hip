// Held-out performance per iteration (run(M_test=)): the six masked sums that metrics_from_sums finishes -- n, sum R, sum R^2,
// sum P, sum P^2, sum R P -- of the CURRENT factors over a sparse, row-sorted list of held-out entries.  One launch pair per
// iteration, enqueued behind the iteration's last kernel; nothing of R's I x J entries is read.
//
// Layout.  A wave owns one row i of R (four waves = four consecutive rows per block, heldout_blocks(I) blocks: no grid stride).
// The row's factor row is loaded once and held for all of the row's entries: the 64 lanes form 64 / (KP / 4) groups of KP / 4
// lanes, lane `sub` of every group holds columns 4 sub .. 4 sub + 3 as four doubles (one coalesced 16-byte load per lane).
// A step of the wave takes one entry per group: the group's lanes read their 16 bytes of row j of the other factor (a row of KP
// floats = one or two whole 128-byte lines per group), multiply and add in fp64, and a butterfly over the group's lanes sums
// the KP / 4 partial dot products.  Column index and value of the next step's entry are fetched before the current step's
// arithmetic.
// Tri-factorisation: the held row is (F_i S) in fp64 -- formed once per row from F's fp32 row and S's fp32 entries (both staged
// in LDS), K fused multiply-adds per held column, never through the sweeps' fp32 effective factor.
// Order of the sums (fixed: two runs give the same bits, no floating-point atomics): lane 0 of a group adds its entries in list
// order; a butterfly over the wave; the block's four waves in wave order (LDS [4][6]: consecutive doubles, one bank pair each);
// HeldoutFold adds the blocks' partials, thread t blocks t, t + 256, ..., then a tree over LDS [6][256] (thread-major:
// conflict-free).
//
// Column-major factors of rank up to 256 (the handles of bnmtf_np_create: U [K][I], V [K][J], or F, S, G): HeldoutNp.
// Same grid, same partials, same fold.  The lanes run along the row's entries instead -- lane l takes entries beg + l, beg + l + 64,
// ... -- and for a fixed k the 64 addresses V[k J + j_l] ascend within one stretch of column k.  The row's own factor row (U_ik, or
// (F_i S)_l formed in fp64 from the fp32 F_i and S, lanes along l) is staged once per row in LDS as doubles ([4][256], 8 KiB) and
// read by broadcast.  Order of the sums: the lane's entries in list order, then as above.
//
// Both forms of the three kernels: many.h.  The main kernels run heldout_blocks(I) blocks; the fold finds its record `it` records
// behind the run's first, so a model's argument bytes are the same in every iteration.
#include "kernels.h"
#include "many.h"

namespace bnmtf {

namespace {

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int KP, bool TRI>
struct Heldout {
  typedef HeldoutArgs Args;
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args& a) { return heldout_blocks(a.I); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int) {
    constexpr int LPE = KP / 4;          // lanes per entry
    constexpr int EPS = 64 / LPE;        // entries per wave step
    __shared__ __attribute__((aligned(16))) float Ssh[TRI ? 64 * KP : 4];     // S [K][KP], zero beyond column L
    __shared__ __attribute__((aligned(16))) float Fsh[TRI ? 4 * 64 : 4];      // the waves' rows of F
    __shared__ double red[kHeldoutRowsPerBlock][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPE, grp = lane / LPE;
    const int i = blockIdx.x * kHeldoutRowsPerBlock + wave;
    const bool row_ok = i < a.I;

    // ---- the row's held factor: columns 4 sub .. 4 sub + 3 of A_i (or of F_i S), fp64
    double av[4] = {0.0, 0.0, 0.0, 0.0};
    if (TRI) {
      for (int t = threadIdx.x; t < a.K * KP; t += 256) {
        const int k = t / KP, l = t % KP;
        Ssh[t] = l < a.L ? a.S[k * a.L + l] : 0.f;
      }
      if (row_ok && lane < a.KPa / 4)
        *reinterpret_cast<float4*>(&Fsh[wave * 64 + 4 * lane]) = *reinterpret_cast<const float4*>(a.A + (size_t)i * a.KPa + 4 * lane);
      __syncthreads();
      if (row_ok)
        for (int k = 0; k < a.K; ++k) {
          const double f = (double)Fsh[wave * 64 + k];
          const float4 s4 = *reinterpret_cast<const float4*>(&Ssh[k * KP + 4 * sub]);
          av[0] = fma(f, (double)s4.x, av[0]); av[1] = fma(f, (double)s4.y, av[1]);
          av[2] = fma(f, (double)s4.z, av[2]); av[3] = fma(f, (double)s4.w, av[3]);
        }
    } else if (row_ok) {
      const float4 a4 = *reinterpret_cast<const float4*>(a.A + (size_t)i * KP + 4 * sub);
      av[0] = (double)a4.x; av[1] = (double)a4.y; av[2] = (double)a4.z; av[3] = (double)a4.w;
    }

    // ---- the row's entries, EPS per step
    const uint32_t beg = row_ok ? a.rowptr[i] : 0u, end = row_ok ? a.rowptr[i + 1] : 0u;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t e = beg + (uint32_t)grp;
    bool live = e < end;
    uint32_t j = live ? a.col[e] : 0u;
    float r32 = live ? a.rval[e] : 0.f;
    for (uint32_t base = beg; base < end; base += EPS) {
      const float4 b4 = *reinterpret_cast<const float4*>(a.B + (size_t)j * KP + 4 * sub);
      const uint32_t en = e + EPS;
      const bool ln = en < end;
      const uint32_t jn = ln ? a.col[en] : 0u;
      const float rn = ln ? a.rval[en] : 0.f;
      double p = 0.0;                    // (the padding columns take no part, whatever they hold)
      if (4 * sub + 0 < a.Wb) p = fma(av[0], (double)b4.x, p);
      if (4 * sub + 1 < a.Wb) p = fma(av[1], (double)b4.y, p);
      if (4 * sub + 2 < a.Wb) p = fma(av[2], (double)b4.z, p);
      if (4 * sub + 3 < a.Wb) p = fma(av[3], (double)b4.w, p);
#pragma unroll
      for (int m = LPE / 2; m >= 1; m >>= 1) p += __shfl_xor(p, m, 64);
      if (live && sub == 0) {
        const double r = (double)r32;
        s[0] += 1.0; s[1] += r; s[2] = fma(r, r, s[2]); s[3] += p; s[4] = fma(p, p, s[4]); s[5] = fma(r, p, s[5]);
      }
      e = en; live = ln; j = jn; r32 = rn;
    }

    // ---- wave, then block
#pragma unroll
    for (int m = 0; m < 6; ++m) s[m] = wave_sum(s[m]);
    if (lane == 0)
      for (int m = 0; m < 6; ++m) red[wave][m] = s[m];
    __syncthreads();
    if (threadIdx.x < 8) {
      double v = 0.0;
      if (threadIdx.x < 6)
        for (int w = 0; w < kHeldoutRowsPerBlock; ++w) v += red[w][threadIdx.x];
      a.part[(size_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
  }
};

// Column-major fp32 factors, ranks up to kHeldoutNpMaxRank: a lane per entry of the row.
template <bool TRI>
struct HeldoutNp {
  typedef HeldoutNpArgs Args;
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args& a) { return heldout_blocks(a.I); }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int) {
    __shared__ double rowf[kHeldoutRowsPerBlock][kHeldoutNpMaxRank];       // the waves' factor rows: U_i, or F_i S
    __shared__ double red[kHeldoutRowsPerBlock][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kHeldoutRowsPerBlock + wave;
    const bool row_ok = i < a.I;
    const int W = TRI ? a.L : a.K;                 // columns of the row's factor row = rows of Xc
    double* const mine = rowf[wave];

    // ---- the row's factor row, fp64, lanes along its columns
    if (row_ok) {
      if (TRI) {
        for (int l = lane; l < W; l += 64) {
          double v = 0.0;
          for (int k = 0; k < a.K; ++k) v = fma((double)a.Xr[(size_t)k * a.I + i], (double)a.S[(size_t)k * a.L + l], v);
          mine[l] = v;
        }
      } else {
        for (int k = lane; k < W; k += 64) mine[k] = (double)a.Xr[(size_t)k * a.I + i];
      }
    }
    __syncthreads();

    // ---- the row's entries, 64 per step
    const uint32_t beg = row_ok ? a.rowptr[i] : 0u, end = row_ok ? a.rowptr[i + 1] : 0u;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t e = beg + (uint32_t)lane;
    bool live = e < end;
    uint32_t j = live ? a.col[e] : 0u;
    float r32 = live ? a.rval[e] : 0.f;
    for (uint32_t base = beg; base < end; base += 64) {
      const float* bcol = a.Xc + j;                // (a lane without an entry reads column 0: J >= 1)
      const uint32_t en = e + 64;
      const bool ln = en < end;
      const uint32_t jn = ln ? a.col[en] : 0u;
      const float rn = ln ? a.rval[en] : 0.f;
      double p = 0.0;
#pragma unroll 4
      for (int k = 0; k < W; ++k) p = fma(mine[k], (double)bcol[(size_t)k * a.J], p);
      if (live) {
        const double r = (double)r32;
        s[0] += 1.0; s[1] += r; s[2] = fma(r, r, s[2]); s[3] += p; s[4] = fma(p, p, s[4]); s[5] = fma(r, p, s[5]);
      }
      e = en; live = ln; j = jn; r32 = rn;
    }

    // ---- wave, then block
#pragma unroll
    for (int m = 0; m < 6; ++m) s[m] = wave_sum(s[m]);
    if (lane == 0)
      for (int m = 0; m < 6; ++m) red[wave][m] = s[m];
    __syncthreads();
    if (threadIdx.x < 8) {
      double v = 0.0;
      if (threadIdx.x < 6)
        for (int w = 0; w < kHeldoutRowsPerBlock; ++w) v += red[w][threadIdx.x];
      a.part[(size_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
  }
};

// the blocks' partial sums in a fixed order, into the iteration's record (rec: the run's FIRST record)
struct HeldoutFold {
  struct Args { const double* part; double* rec; int nblocks, pad; };
  static constexpr int kThreads = 256;
  static __host__ __device__ int blocks(const Args&) { return 1; }
  template <int FORM>
  static __device__ __forceinline__ void body(const Args& a, int, int it) {
    double* rec = a.rec + (size_t)it * 8;
    __shared__ double red[6][256];
    const int tid = threadIdx.x;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < a.nblocks; b += 256)
      for (int m = 0; m < 6; ++m) s[m] += a.part[(size_t)b * 8 + m];
    for (int m = 0; m < 6; ++m) red[m][tid] = s[m];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
      if (tid < w) for (int m = 0; m < 6; ++m) red[m][tid] += red[m][tid + w];
      __syncthreads();
    }
    if (tid < 8) rec[tid] = tid < 6 ? red[tid][0] : 0.0;
  }
};

}  // namespace

// the fold behind a main kernel of `nblocks` blocks -- launched, or recorded behind the main kernel's record (kernels.h: the
// observed-entry layout's held-out kernel, kernel_obs_heldout.hip, ends in it as well)
void launch_fold(const double* part, int nblocks, double* rec, hipStream_t st) {
  HeldoutFold::Args a; memset(&a, 0, sizeof(a));
  a.part = part; a.rec = rec; a.nblocks = nblocks;
  launch_forms<HeldoutFold>(a, st);
}

namespace {

// the values of R at the listed entries: a wave per row, its lanes along the row's entries
__global__ __launch_bounds__(256) void heldout_values_kernel(const float* R, int I, int J, const uint32_t* rowptr, const uint32_t* col, float* rval) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kHeldoutRowsPerBlock + wave;
  if (i >= I) return;
  const uint32_t end = rowptr[i + 1];
  for (uint32_t e = rowptr[i] + (uint32_t)lane; e < end; e += 64) rval[e] = R[(size_t)i * J + col[e]];
}

}  // namespace

// While a Recorder is installed (many.h): a.rec is the run's first record, and the pair is recorded at kHeldoutSite, behind every
// site of the model's family.  (The caller has zeroed the pack's padding: a recorded list compares argument bytes.)
void launch_heldout(const HeldoutArgs& a, hipStream_t st) {
  site_at(kHeldoutSite);
  if (a.S) {
    if (a.KPb == 32) launch_forms<Heldout<32, true>>(a, st);
    else launch_forms<Heldout<64, true>>(a, st);
  } else {
    if (a.KPb == 32) launch_forms<Heldout<32, false>>(a, st);
    else launch_forms<Heldout<64, false>>(a, st);
  }
  launch_fold(a.part, heldout_blocks(a.I), a.rec, st);
}

void launch_heldout_np(const HeldoutNpArgs& a, hipStream_t st) {
  site_at(kHeldoutSite);
  if (a.S) launch_forms<HeldoutNp<true>>(a, st);
  else launch_forms<HeldoutNp<false>>(a, st);
  launch_fold(a.part, heldout_blocks(a.I), a.rec, st);
}

void launch_heldout_values(const float* R, int I, int J, const uint32_t* rowptr, const uint32_t* col, float* rval, hipStream_t st) {
  hipLaunchKernelGGL(heldout_values_kernel, dim3(heldout_blocks(I)), dim3(256), 0, st, R, I, J, rowptr, col, rval);
}

}  // namespace bnmtf
