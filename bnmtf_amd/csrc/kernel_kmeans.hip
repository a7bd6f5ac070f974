// Masked K-means for initialise(init_FG='kmeans') (code/models/kmeans/kmeans.py:70-204): the two O(points x coordinates x K)
// passes of an iteration on the device.
//   assignment (:87-119): MSE between a point and a centroid over the coordinates both know; no overlap = infinitely far;
//     ties go to the lowest cluster index.  One wave per point, lanes stride the coordinates; points, centroids and sums
//     in fp64 like the reference (an fp32 copy of the data can flip a near-tie between two centroids).
//   update (:126-163, find_known_coordinate_values :170-182): per cluster and coordinate the count and the sum of the
//     members' observed values.  The O(K x coordinates) division, the masks and the empty-cluster rule ('singleton':
//     the point furthest from its centroid moves) stay on the host (bnmtf_amd/kmeans.py).
#include <atomic>
#include <cstring>
#include <vector>

#include "model.h"

namespace bnmtf {

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const double* X, const uint8_t* M, int n, int d, int K, const double* C,
                                                             const uint8_t* Mc, int* assign, double* dist) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const double* x = X + (size_t)p * d;
  const uint8_t* m = M + (size_t)p * d;
  int best = -1;
  double best_mse = 0.0;
  bool have = false;                                   // a finite MSE has been seen
  for (int c = 0; c < K; ++c) {
    double num = 0.0, ov = 0.0;
    for (int j = lane; j < d; j += 64) {
      if (m[j] && Mc[(size_t)c * d + j]) {
        const double df = x[j] - C[(size_t)c * d + j];
        num = fma(df, df, num); ov += 1.0;
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { num += __shfl_xor(num, s, 64); ov += __shfl_xor(ov, s, 64); }
    // kmeans.py:107-113: while no defined MSE has been seen every cluster replaces the choice; after that only a smaller defined MSE does
    const bool defined = ov > 0.0;
    const double mse = defined ? num / ov : 0.0;
    if (!have) { best = c; have = defined; best_mse = mse; }          // (so a point that overlaps no centroid ends in the last cluster)
    else if (defined && mse < best_mse) { best = c; best_mse = mse; }
  }
  if (lane == 0) { assign[p] = best; dist[p] = have ? best_mse : __longlong_as_double(0x7ff0000000000000LL); }
}

// cnt[c][j] = #members of c that observe coordinate j, tot[c][j] = sum of their values, for the clusters c0 .. c0 + KC - 1:
// block = 64 coordinates x 4 point groups, private LDS accumulators per group (no atomics), groups summed in order
constexpr int kKMeansChunk = 40;                        // clusters per launch (8 x 40 x 64 doubles of LDS)
__global__ __launch_bounds__(256) void kmeans_sums_kernel(const double* X, const uint8_t* M, int n, int d, int c0, int KC, const int* assign,
                                                           double* cnt, double* tot) {
  extern __shared__ double acc[];                       // [4][KC][64] counts, then [4][KC][64] totals
  const int jl = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + jl;
  double* ac = acc + (size_t)g * KC * 64;
  double* at = acc + (size_t)(4 + g) * KC * 64;
  for (int c = 0; c < KC; ++c) { ac[c * 64 + jl] = 0.0; at[c * 64 + jl] = 0.0; }
  if (j < d)
    for (int p = g; p < n; p += 4) {
      const int c = assign[p] - c0;
      if (c >= 0 && c < KC && M[(size_t)p * d + j]) { ac[c * 64 + jl] += 1.0; at[c * 64 + jl] += X[(size_t)p * d + j]; }
    }
  __syncthreads();
  if (j < d)
    for (int c = g; c < KC; c += 4) {
      double sc = 0.0, st = 0.0;
      for (int q = 0; q < 4; ++q) { sc += acc[((size_t)q * KC + c) * 64 + jl]; st += acc[((size_t)(4 + q) * KC + c) * 64 + jl]; }
      cnt[(size_t)(c0 + c) * d + j] = sc; tot[(size_t)(c0 + c) * d + j] = st;
    }
}

// ---- the list forms: the same two passes over the observed entries alone, in the dense kernels' summation
// order, so that every output equals the dense form's bit for bit.  The entries are held twice: by point, a point's entries ordered
// by (coordinate & 63, coordinate) -- lane l of the dense assignment adds the coordinates j = l (mod 64) in ascending j: a contiguous
// sub-range of that order --, and by coordinate, a coordinate's entries ordered by (point & 3, point) -- point group g of the dense
// sums adds the points p = g (mod 4) in ascending p.  A lane or group finds its sub-range by a binary search over its unit's
// entries keyed by the low bits (no table of 64 or 4 words per unit: memory follows the entries).

// first position in [b, e) whose index has (idx & mask) >= key
__device__ __forceinline__ uint32_t kmeans_first_of(const uint32_t* idx, uint32_t b, uint32_t e, uint32_t mask, uint32_t key) {
  while (b < e) {
    const uint32_t m = b + ((e - b) >> 1);
    if ((idx[m] & mask) < key) b = m + 1; else e = m;
  }
  return b;
}

// centroids and their masks transposed, [d][KP] with KP = K rounded up to kKMeansListC (the padding masked out): the clusters a
// lane needs for one entry are contiguous.  kKMeansListC clusters at a time in registers, one walk of the lane's entries for all of them.
constexpr int kKMeansListC = 8;
__global__ __launch_bounds__(256) void kmeans_assign_list_kernel(const uint32_t* pptr, const uint32_t* pcoord, const double* pval, int n, int K,
                                                                  int KP, const double* CT, const uint8_t* McT, int* assign, double* dist) {
  const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n) return;
  const uint32_t end = pptr[p + 1];
  const uint32_t lo = kmeans_first_of(pcoord, pptr[p], end, 63u, (uint32_t)lane);
  uint32_t hi = (uint32_t)__shfl_down((int)lo, 1, 64);
  if (lane == 63) hi = end;
  int best = -1;
  double best_mse = 0.0;
  bool have = false;                                   // a finite MSE has been seen
  for (int c0 = 0; c0 < K; c0 += kKMeansListC) {
    double num[kKMeansListC], ov[kKMeansListC];
#pragma unroll
    for (int i = 0; i < kKMeansListC; ++i) { num[i] = 0.0; ov[i] = 0.0; }
    for (uint32_t t = lo; t < hi; ++t) {
      const size_t at = (size_t)pcoord[t] * KP + c0;
      const double x = pval[t];
      const uint64_t mk = *reinterpret_cast<const uint64_t*>(McT + at);      // (KP and c0 are multiples of 8)
#pragma unroll
      for (int i = 0; i < kKMeansListC; ++i)
        if ((mk >> (8 * i)) & 0xffull) {
          const double df = x - CT[at + i];
          num[i] = fma(df, df, num[i]); ov[i] += 1.0;
        }
    }
#pragma unroll
    for (int i = 0; i < kKMeansListC; ++i) {
      double nm = num[i], o = ov[i];
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) { nm += __shfl_xor(nm, s, 64); o += __shfl_xor(o, s, 64); }
      if (c0 + i < K) {                                  // kmeans.py:107-113, as kmeans_assign_kernel
        const int c = c0 + i;
        const bool defined = o > 0.0;
        const double mse = defined ? nm / o : 0.0;
        if (!have) { best = c; have = defined; best_mse = mse; }
        else if (defined && mse < best_mse) { best = c; best_mse = mse; }
      }
    }
  }
  if (lane == 0) { assign[p] = best; dist[p] = have ? best_mse : __longlong_as_double(0x7ff0000000000000LL); }
}

// kmeans_sums_kernel with thread (coordinate, g) walking its sub-range of the coordinate's entries instead of all points: the same
// LDS layout, the same combine, the same passes
__global__ __launch_bounds__(256) void kmeans_sums_list_kernel(const uint32_t* cptr, const uint32_t* cpoint, const double* cval, int d, int c0, int KC,
                                                                const int* assign, double* cnt, double* tot) {
  extern __shared__ double acc[];                       // [4][KC][64] counts, then [4][KC][64] totals
  const int jl = threadIdx.x & 63, g = threadIdx.x >> 6, j = blockIdx.x * 64 + jl;
  double* ac = acc + (size_t)g * KC * 64;
  double* at = acc + (size_t)(4 + g) * KC * 64;
  for (int c = 0; c < KC; ++c) { ac[c * 64 + jl] = 0.0; at[c * 64 + jl] = 0.0; }
  if (j < d) {
    const uint32_t end = cptr[j + 1];
    const uint32_t lo = kmeans_first_of(cpoint, cptr[j], end, 3u, (uint32_t)g);
    const uint32_t hi = g == 3 ? end : kmeans_first_of(cpoint, lo, end, 3u, (uint32_t)g + 1u);
    for (uint32_t t = lo; t < hi; ++t) {
      const int c = assign[cpoint[t]] - c0;
      if (c >= 0 && c < KC) { ac[c * 64 + jl] += 1.0; at[c * 64 + jl] += cval[t]; }
    }
  }
  __syncthreads();
  if (j < d)
    for (int c = g; c < KC; c += 4) {
      double sc = 0.0, st = 0.0;
      for (int q = 0; q < 4; ++q) { sc += acc[((size_t)q * KC + c) * 64 + jl]; st += acc[((size_t)(4 + q) * KC + c) * 64 + jl]; }
      cnt[(size_t)(c0 + c) * d + j] = sc; tot[(size_t)(c0 + c) * d + j] = st;
    }
}

// the entries [b, e) of the point list -- one point's -- take their values from row [n_coords], in both lists
__global__ __launch_bounds__(256) void kmeans_set_row_list_kernel(const uint32_t* pcoord, const uint32_t* p2c, uint32_t b, uint32_t e, const double* row,
                                                                   double* pval, double* cval) {
  const uint32_t t = b + blockIdx.x * 256u + threadIdx.x;
  if (t < e) { const double v = row[pcoord[t]]; pval[t] = v; cval[p2c[t]] = v; }
}

struct KMeansModel {
  int n = 0, d = 0, K = 0, device = 0;
  double* X = nullptr; uint8_t* M = nullptr; double* C = nullptr; uint8_t* Mc = nullptr; int* assign = nullptr;
  double *dist = nullptr, *cnt = nullptr, *tot = nullptr;
  // a handle of bnmtf_kmeans_create_list: no X, no M; C and Mc hold the transposed forms [d][KP]
  bool list = false;
  int KP = 0;
  uint32_t *pptr = nullptr, *pcoord = nullptr, *cptr = nullptr, *cpoint = nullptr, *p2c = nullptr;
  double *pval = nullptr, *cval = nullptr, *row = nullptr;
  std::vector<uint32_t> h_pptr;                         // (set_row: where a point's entries lie)
  std::vector<double> h_CT; std::vector<uint8_t> h_McT; // assign's staging
};

// What a list create holds of the entries, built on the host before any device call (and handed out by bnmtf_kmeans_build_lists).
// Refuses an entry outside the matrix and an entry that occurs twice; a point or a coordinate may be empty.
struct KMeansLists {
  std::vector<uint32_t> pptr, pcoord, cptr, cpoint, p2c;
  std::vector<double> pval, cval;
};

// one stable counting pass: `in` (entry numbers) ordered by key(entry) < nkeys
template <class Key>
static void kmeans_pass(const std::vector<uint32_t>& in, std::vector<uint32_t>& out, size_t nkeys, Key key) {
  std::vector<uint32_t> at(nkeys + 1, 0);
  for (uint32_t e : in) at[(size_t)key(e) + 1]++;
  for (size_t k = 0; k < nkeys; ++k) at[k + 1] += at[k];
  out.resize(in.size());
  for (uint32_t e : in) out[at[key(e)]++] = e;
}

static int kmeans_lists(int n_points, int n_coords, uint64_t n, const int32_t* points, const int32_t* coords, const double* values, KMeansLists& ls) {
  if (n >= ((uint64_t)1 << 31)) { set_error("at most 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (points[e] < 0 || points[e] >= n_points || coords[e] < 0 || coords[e] >= n_coords) {
      set_error("entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, points[e], coords[e], n_points, n_coords);
      return BNMTF_EINVAL;
    }
  std::vector<uint32_t> id((size_t)n), tmp, byp, byc;
  for (size_t e = 0; e < (size_t)n; ++e) id[e] = (uint32_t)e;
  // by point: (point, coordinate & 63, coordinate) -- least significant keys first
  const size_t cw = ((size_t)n_coords + 63) / 64, pw = ((size_t)n_points + 3) / 4;
  kmeans_pass(id, tmp, 64 * cw, [&](uint32_t e) { return (size_t)(coords[e] & 63) * cw + (size_t)(coords[e] >> 6); });
  kmeans_pass(tmp, byp, (size_t)n_points, [&](uint32_t e) { return (size_t)points[e]; });
  for (size_t t = 1; t < byp.size(); ++t)
    if (points[byp[t]] == points[byp[t - 1]] && coords[byp[t]] == coords[byp[t - 1]]) {
      set_error("the entry (%d, %d) occurs twice", points[byp[t]], coords[byp[t]]);
      return BNMTF_EINVAL;
    }
  // by coordinate: (coordinate, point & 3, point)
  kmeans_pass(id, tmp, 4 * pw, [&](uint32_t e) { return (size_t)(points[e] & 3) * pw + (size_t)(points[e] >> 2); });
  kmeans_pass(tmp, byc, (size_t)n_coords, [&](uint32_t e) { return (size_t)coords[e]; });
  ls.pptr.assign((size_t)n_points + 1, 0); ls.cptr.assign((size_t)n_coords + 1, 0);
  ls.pcoord.resize((size_t)n); ls.pval.resize((size_t)n); ls.cpoint.resize((size_t)n); ls.cval.resize((size_t)n); ls.p2c.resize((size_t)n);
  for (size_t t = 0; t < (size_t)n; ++t) {
    const uint32_t e = byp[t], f = byc[t];
    ls.pptr[(size_t)points[e] + 1]++; ls.pcoord[t] = (uint32_t)coords[e]; ls.pval[t] = values[e];
    ls.cptr[(size_t)coords[f] + 1]++; ls.cpoint[t] = (uint32_t)points[f]; ls.cval[t] = values[f];
    id[f] = (uint32_t)t;                                // entry -> its place in the coordinate list
  }
  for (size_t t = 0; t < (size_t)n; ++t) ls.p2c[t] = id[byp[t]];
  for (int i = 0; i < n_points; ++i) ls.pptr[(size_t)i + 1] += ls.pptr[i];
  for (int j = 0; j < n_coords; ++j) ls.cptr[(size_t)j + 1] += ls.cptr[j];
  return BNMTF_OK;
}

// a host table onto the device, in an allocation of its own (at least one element); returns with the copy done
template <typename T>
static int kmeans_upload(T** dst, const std::vector<T>& src) {
  HIPCHK(hipMalloc((void**)dst, (src.empty() ? 1 : src.size()) * sizeof(T)));
  if (!src.empty()) HIPCHK(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  return BNMTF_OK;
}

// the dynamic LDS of a sums kernel (160 KiB at kKMeansChunk clusters), once per device
static int kmeans_sums_lds(const void* kernel, std::atomic<uint64_t>& ok, int device) {
  const int dev = device & 63;
  if (!(ok.load() & (1ull << dev))) {
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ok.fetch_or(1ull << dev);
  }
  return BNMTF_OK;
}

}  // namespace bnmtf

using namespace bnmtf;

extern "C" {

int bnmtf_kmeans_destroy(void* hv) {
  KMeansModel* h = static_cast<KMeansModel*>(hv);
  if (!h) return BNMTF_OK;
  (void)hipSetDevice(h->device);
  (void)hipFree(h->X); (void)hipFree(h->M); (void)hipFree(h->C); (void)hipFree(h->Mc); (void)hipFree(h->assign);
  (void)hipFree(h->dist); (void)hipFree(h->cnt); (void)hipFree(h->tot);
  (void)hipFree(h->pptr); (void)hipFree(h->pcoord); (void)hipFree(h->cptr); (void)hipFree(h->cpoint); (void)hipFree(h->p2c);
  (void)hipFree(h->pval); (void)hipFree(h->cval); (void)hipFree(h->row);
  delete h;
  return BNMTF_OK;
}

int bnmtf_kmeans_create(const double* X, const uint8_t* M, int n_points, int n_coords, int K, int device, void** out) {
  *out = nullptr;
  if (!X || !M || n_points < 1 || n_coords < 1 || K < 1 || K > 1024) { set_error("bnmtf_kmeans_create: bad argument"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(device));
  KMeansModel* h = new KMeansModel();
  h->n = n_points; h->d = n_coords; h->K = K; h->device = device;
  const size_t nd = (size_t)n_points * n_coords, kd = (size_t)K * n_coords;
  auto fail = [&](hipError_t e) { set_error("bnmtf_kmeans_create: %s", hipGetErrorString(e)); bnmtf_kmeans_destroy(h); return BNMTF_EHIP; };
  hipError_t e;
  if ((e = hipMalloc((void**)&h->X, nd * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->M, nd)) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->C, kd * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->Mc, kd)) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->assign, (size_t)n_points * sizeof(int))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->dist, (size_t)n_points * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->cnt, kd * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMalloc((void**)&h->tot, kd * sizeof(double))) != hipSuccess) return fail(e);
  if ((e = hipMemcpy(h->X, X, nd * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
  if ((e = hipMemcpy(h->M, M, nd, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
  *out = h;
  return BNMTF_OK;
}

// The host half of bnmtf_kmeans_create_list on its own, checks included (no device call): the point list -- point_ptr
// [n_points + 1], a point's entries ordered by (coordinate & 63, coordinate) --, the coordinate list -- coord_ptr [n_coords + 1], a
// coordinate's entries ordered by (point & 3, point) -- and point_to_coord [n]: the place in the coordinate list of the entry at
// each place of the point list.  Any output may be null.
int bnmtf_kmeans_build_lists(int n_points, int n_coords, uint64_t n, const int32_t* points, const int32_t* coords, const double* values,
                             uint32_t* point_ptr, uint32_t* point_coord, double* point_val, uint32_t* coord_ptr, uint32_t* coord_point,
                             double* coord_val, uint32_t* point_to_coord) try {
  if (!points || !coords || !values) { set_error("bnmtf_kmeans_build_lists: null argument"); return BNMTF_EINVAL; }
  if (n_points < 1 || n_coords < 1) { set_error("bnmtf_kmeans_build_lists: unsupported shape n_points=%d n_coords=%d", n_points, n_coords); return BNMTF_EINVAL; }
  KMeansLists ls;
  CHK(kmeans_lists(n_points, n_coords, n, points, coords, values, ls));
  if (point_ptr) memcpy(point_ptr, ls.pptr.data(), ls.pptr.size() * sizeof(uint32_t));
  if (coord_ptr) memcpy(coord_ptr, ls.cptr.data(), ls.cptr.size() * sizeof(uint32_t));
  if (n) {
    if (point_coord) memcpy(point_coord, ls.pcoord.data(), ls.pcoord.size() * sizeof(uint32_t));
    if (point_val) memcpy(point_val, ls.pval.data(), ls.pval.size() * sizeof(double));
    if (coord_point) memcpy(coord_point, ls.cpoint.data(), ls.cpoint.size() * sizeof(uint32_t));
    if (coord_val) memcpy(coord_val, ls.cval.data(), ls.cval.size() * sizeof(double));
    if (point_to_coord) memcpy(point_to_coord, ls.p2c.data(), ls.p2c.size() * sizeof(uint32_t));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// bnmtf_kmeans_create from the observed entries (point, coordinate, value), in any order: the handle holds the two lists (28 bytes
// an entry) and nothing of size n_points x n_coords; assign, sums, set_row and destroy serve it as they serve a dense handle, with
// the dense form's bits.  Checks and both orderings come before the first device call.
int bnmtf_kmeans_create_list(int n_points, int n_coords, uint64_t n, const int32_t* points, const int32_t* coords, const double* values, int K,
                             int device, void** out) try {
  if (!out) { set_error("bnmtf_kmeans_create_list: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!points || !coords || !values) { set_error("bnmtf_kmeans_create_list: null argument"); return BNMTF_EINVAL; }
  if (n_points < 1 || n_coords < 1) { set_error("bnmtf_kmeans_create_list: unsupported shape n_points=%d n_coords=%d", n_points, n_coords); return BNMTF_EINVAL; }
  if (K < 1 || K > 1024) { set_error("bnmtf_kmeans_create_list: unsupported K=%d (1 .. 1024)", K); return BNMTF_EINVAL; }
  KMeansLists ls;
  CHK(kmeans_lists(n_points, n_coords, n, points, coords, values, ls));
  HIPCHK(hipSetDevice(device));
  struct Guard {
    KMeansModel* h;
    ~Guard() { if (h) bnmtf_kmeans_destroy(h); }
  } guard{new KMeansModel()};
  KMeansModel* h = guard.h;
  h->n = n_points; h->d = n_coords; h->K = K; h->device = device; h->list = true;
  h->KP = (K + kKMeansListC - 1) / kKMeansListC * kKMeansListC;
  const size_t kd = (size_t)K * n_coords, kpd = (size_t)h->KP * n_coords;
  CHK(kmeans_upload(&h->pptr, ls.pptr));
  CHK(kmeans_upload(&h->pcoord, ls.pcoord));
  CHK(kmeans_upload(&h->pval, ls.pval));
  CHK(kmeans_upload(&h->cptr, ls.cptr));
  CHK(kmeans_upload(&h->cpoint, ls.cpoint));
  CHK(kmeans_upload(&h->cval, ls.cval));
  CHK(kmeans_upload(&h->p2c, ls.p2c));
  HIPCHK(hipMalloc((void**)&h->C, kpd * sizeof(double)));
  HIPCHK(hipMalloc((void**)&h->Mc, kpd));
  HIPCHK(hipMalloc((void**)&h->row, (size_t)n_coords * sizeof(double)));
  HIPCHK(hipMalloc((void**)&h->assign, (size_t)n_points * sizeof(int)));
  HIPCHK(hipMalloc((void**)&h->dist, (size_t)n_points * sizeof(double)));
  HIPCHK(hipMalloc((void**)&h->cnt, kd * sizeof(double)));
  HIPCHK(hipMalloc((void**)&h->tot, kd * sizeof(double)));
  h->h_pptr.swap(ls.pptr);
  h->h_CT.assign(kpd, 0.0); h->h_McT.assign(kpd, 0);
  guard.h = nullptr;
  *out = h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// assignment() (kmeans.py:87-119) for the given centroids [K][n_coords] and their masks; assign_out [n_points],
// dist_out [n_points] (MSE to the chosen centroid; +inf when it shares no coordinate with the point)
int bnmtf_kmeans_assign(void* hv, const double* centroids, const uint8_t* mask_centroids, int32_t* assign_out, double* dist_out) {
  KMeansModel* h = static_cast<KMeansModel*>(hv);
  HIPCHK(hipSetDevice(h->device));
  const size_t kd = (size_t)h->K * h->d;
  if (h->list) {                                         // [K][d] -> [d][KP]; the padding stays masked out
    const int K = h->K, KP = h->KP, d = h->d;
    for (int c = 0; c < K; ++c)
      for (int j = 0; j < d; ++j) {
        h->h_CT[(size_t)j * KP + c] = centroids[(size_t)c * d + j];
        h->h_McT[(size_t)j * KP + c] = mask_centroids[(size_t)c * d + j];
      }
    HIPCHK(hipMemcpy(h->C, h->h_CT.data(), h->h_CT.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->Mc, h->h_McT.data(), h->h_McT.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kmeans_assign_list_kernel, dim3((h->n + 3) / 4), dim3(256), 0, nullptr, h->pptr, h->pcoord, h->pval, h->n, K, KP, h->C, h->Mc,
                       h->assign, h->dist);
  } else {
    HIPCHK(hipMemcpy(h->C, centroids, kd * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->Mc, mask_centroids, kd, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((h->n + 3) / 4), dim3(256), 0, nullptr, h->X, h->M, h->n, h->d, h->K, h->C, h->Mc, h->assign, h->dist);
  }
  HIPCHK(hipMemcpy(assign_out, h->assign, (size_t)h->n * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dist_out, h->dist, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
}

// row `index` of X := values [n_coords] (the reference's refilled centroid is a view of its data point, kmeans.py:141: the
// means later written into that centroid change the point); a list handle takes the values of the point's observed entries, in
// both lists
int bnmtf_kmeans_set_row(void* hv, int index, const double* values) {
  KMeansModel* h = static_cast<KMeansModel*>(hv);
  if (!h || !values || index < 0 || index >= h->n) { set_error("bnmtf_kmeans_set_row: bad argument"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  if (h->list) {
    const uint32_t b = h->h_pptr[(size_t)index], e = h->h_pptr[(size_t)index + 1];
    if (e == b) return BNMTF_OK;
    HIPCHK(hipMemcpy(h->row, values, (size_t)h->d * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kmeans_set_row_list_kernel, dim3((e - b + 255) / 256), dim3(256), 0, nullptr, h->pcoord, h->p2c, b, e, h->row, h->pval, h->cval);
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipGetLastError());
    return BNMTF_OK;
  }
  HIPCHK(hipMemcpy(h->X + (size_t)index * h->d, values, (size_t)h->d * sizeof(double), hipMemcpyHostToDevice));
  return BNMTF_OK;
}

// per cluster and coordinate: the number of members observing it and the sum of their values (update(), kmeans.py:126-182)
int bnmtf_kmeans_sums(void* hv, const int32_t* assign, double* cnt_out, double* tot_out) {
  KMeansModel* h = static_cast<KMeansModel*>(hv);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(h->assign, assign, (size_t)h->n * sizeof(int), hipMemcpyHostToDevice));
  static std::atomic<uint64_t> lds_ok{0}, lds_ok_list{0};
  CHK(h->list ? kmeans_sums_lds((const void*)kmeans_sums_list_kernel, lds_ok_list, h->device)
              : kmeans_sums_lds((const void*)kmeans_sums_kernel, lds_ok, h->device));
  for (int c0 = 0; c0 < h->K; c0 += kKMeansChunk) {      // any K: kKMeansChunk clusters per pass over the points
    const int kc = h->K - c0 < kKMeansChunk ? h->K - c0 : kKMeansChunk;
    if (h->list)
      hipLaunchKernelGGL(kmeans_sums_list_kernel, dim3((h->d + 63) / 64), dim3(256), (size_t)8 * kc * 64 * sizeof(double), nullptr,
                         h->cptr, h->cpoint, h->cval, h->d, c0, kc, h->assign, h->cnt, h->tot);
    else
      hipLaunchKernelGGL(kmeans_sums_kernel, dim3((h->d + 63) / 64), dim3(256), (size_t)8 * kc * 64 * sizeof(double), nullptr,
                         h->X, h->M, h->n, h->d, c0, kc, h->assign, h->cnt, h->tot);
  }
  const size_t kd = (size_t)h->K * h->d;
  HIPCHK(hipMemcpy(cnt_out, h->cnt, kd * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tot_out, h->tot, kd * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
}

}  // extern "C"
