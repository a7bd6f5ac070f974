// Test infrastructure (CPU box only): the bnmtf_kmeans_* entry points (csrc/kernel_kmeans.hip: masked K-means, dense handles and
// handles on entry lists) walked on the library's HOST side under AddressSanitizer + UBSan (`make asan_kmeans`, which compiles
// kernel_kmeans.hip's host code with the sanitizers too), linked against hip_stub.cpp instead of the HIP runtime as driver.cpp is.
// Kernels do not run, so no number that comes back means anything; what is checked is the host code the calls go through -- the
// counting passes of both orders and the permutation, every host<->"device" copy's extent, the transposed staging of assign, the
// pass loop of sums, set_row's range --, every refusal, a create that fails midway, and that destroy gives back every buffer.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <random>
#include <vector>

#include "bnmtf_hip.h"

extern "C" long hipstub_launches();
extern "C" long hipstub_live_allocs();
extern "C" void hipstub_throw_at_sync(long n);

#define OK(expr)                                                                                     \
  do {                                                                                               \
    const int rc_ = (expr);                                                                          \
    if (rc_ != BNMTF_OK) { fprintf(stderr, "FAILED %s -> %d (%s)\n", #expr, rc_, bnmtf_last_error()); exit(2); } \
  } while (0)
#define EXPECT_ERR(expr, text)                                                                       \
  do {                                                                                               \
    const int rc_ = (expr);                                                                          \
    if (rc_ != BNMTF_EINVAL) { fprintf(stderr, "expected BNMTF_EINVAL: %s -> %d\n", #expr, rc_); exit(2); } \
    if (!strstr(bnmtf_last_error(), text)) { fprintf(stderr, "%s: the message \"%s\" lacks \"%s\"\n", #expr, bnmtf_last_error(), text); exit(2); } \
  } while (0)

struct Entries { int n_points, n_coords; std::vector<int32_t> points, coords; std::vector<double> vals; uint64_t n; };
// a share `density` of the matrix in shuffled order; point 1 (where there is one) and the last coordinate stay empty
static Entries make_entries(int n_points, int n_coords, double density, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> p(0.0, 1.0), u(-10.0, 10.0);
  std::vector<size_t> at;
  for (int i = 0; i < n_points; ++i)
    for (int j = 0; j < n_coords; ++j)
      if (p(g) < density && i != 1 && (j != n_coords - 1 || n_coords == 1)) at.push_back((size_t)i * n_coords + j);
  std::shuffle(at.begin(), at.end(), g);
  Entries e; e.n_points = n_points; e.n_coords = n_coords;
  for (size_t q : at) { e.points.push_back((int32_t)(q / n_coords)); e.coords.push_back((int32_t)(q % n_coords)); e.vals.push_back(u(g)); }
  e.n = at.size();
  // (so that data() is never null, even without entries)
  e.points.reserve(1); e.coords.reserve(1); e.vals.reserve(1);
  return e;
}

static int create(const Entries& e, int K, void** h) {
  return bnmtf_kmeans_create_list(e.n_points, e.n_coords, e.n, e.points.data(), e.coords.data(), e.vals.data(), K, 0, h);
}

// a create that must be refused with `text`, or fail, and leave nothing behind
static void create_refused(const Entries& e, int K, const char* text) {
  const long live = hipstub_live_allocs();
  void* h = &h;
  EXPECT_ERR(create(e, K, &h), text);
  if (h != nullptr || hipstub_live_allocs() != live) { fprintf(stderr, "a refused create (K=%d) left a handle or %ld allocations\n", K, hipstub_live_allocs() - live); exit(2); }
}

// assign, sums (twice), set_row of every point, assign and sums again, destroy
static void use(void* h, int n_points, int n_coords, int K) {
  std::vector<double> C((size_t)K * n_coords, 1.0), dist(n_points), cnt((size_t)K * n_coords), tot((size_t)K * n_coords), row(n_coords, 2.0);
  std::vector<uint8_t> Mc((size_t)K * n_coords, 1);
  std::vector<int32_t> a(n_points), in(n_points);
  for (int p = 0; p < n_points; ++p) in[p] = p % K;
  OK(bnmtf_kmeans_assign(h, C.data(), Mc.data(), a.data(), dist.data()));
  OK(bnmtf_kmeans_sums(h, in.data(), cnt.data(), tot.data()));
  OK(bnmtf_kmeans_sums(h, in.data(), cnt.data(), tot.data()));
  for (int p = 0; p < n_points; ++p) OK(bnmtf_kmeans_set_row(h, p, row.data()));
  EXPECT_ERR(bnmtf_kmeans_set_row(h, -1, row.data()), "bad argument");
  EXPECT_ERR(bnmtf_kmeans_set_row(h, n_points, row.data()), "bad argument");
  EXPECT_ERR(bnmtf_kmeans_set_row(h, 0, nullptr), "bad argument");
  OK(bnmtf_kmeans_assign(h, C.data(), Mc.data(), a.data(), dist.data()));
  OK(bnmtf_kmeans_sums(h, in.data(), cnt.data(), tot.data()));
  OK(bnmtf_kmeans_destroy(h));
}

static void walk(int n_points, int n_coords, int K, double density, unsigned seed) {
  const Entries e = make_entries(n_points, n_coords, density, seed);
  const long live0 = hipstub_live_allocs();
  // the host builder: every output, then none
  std::vector<uint32_t> pptr(n_points + 1), cptr(n_coords + 1), pc(e.n + 1), cp(e.n + 1), p2c(e.n + 1);
  std::vector<double> pv(e.n + 1), cv(e.n + 1);
  OK(bnmtf_kmeans_build_lists(n_points, n_coords, e.n, e.points.data(), e.coords.data(), e.vals.data(), pptr.data(), pc.data(), pv.data(), cptr.data(),
                              cp.data(), cv.data(), p2c.data()));
  OK(bnmtf_kmeans_build_lists(n_points, n_coords, e.n, e.points.data(), e.coords.data(), e.vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr));
  if (pptr[n_points] != e.n || cptr[n_coords] != e.n) { fprintf(stderr, "walk: the pointers end at %u / %u, not at %llu\n", pptr[n_points], cptr[n_coords], (unsigned long long)e.n); exit(2); }
  for (uint64_t t = 0; t < e.n; ++t)
    if (p2c[t] >= e.n || cv[p2c[t]] != pv[t]) { fprintf(stderr, "walk: the permutation does not tie place %llu\n", (unsigned long long)t); exit(2); }
  void* h = nullptr;
  OK(create(e, K, &h));
  use(h, n_points, n_coords, K);
  // the dense handle of the same matrix through the same calls
  std::vector<double> X((size_t)n_points * n_coords, 0.0);
  std::vector<uint8_t> M((size_t)n_points * n_coords, 0);
  for (uint64_t q = 0; q < e.n; ++q) { X[(size_t)e.points[q] * n_coords + e.coords[q]] = e.vals[q]; M[(size_t)e.points[q] * n_coords + e.coords[q]] = 1; }
  OK(bnmtf_kmeans_create(X.data(), M.data(), n_points, n_coords, K, 0, &h));
  use(h, n_points, n_coords, K);
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "walk(%d, %d, %d): %ld allocations outlive the handles\n", n_points, n_coords, K, hipstub_live_allocs() - live0); exit(2); }
}

// what the create refuses, and a create that fails midway
static void refusals() {
  const Entries e = make_entries(37, 23, 0.2, 51);
  const int K = 3;
  Entries bad = e; bad.coords[5] = e.n_coords;
  create_refused(bad, K, "lies outside the 37 x 23 matrix");
  bad = e; bad.coords[5] = -1;
  create_refused(bad, K, "lies outside the 37 x 23 matrix");
  bad = e; bad.points[6] = e.n_points;
  create_refused(bad, K, "lies outside the 37 x 23 matrix");
  bad = e; bad.points[6] = -1;
  create_refused(bad, K, "lies outside the 37 x 23 matrix");
  bad = e; bad.points[7] = bad.points[3]; bad.coords[7] = bad.coords[3];
  create_refused(bad, K, "occurs twice");
  bad = e; bad.n = (uint64_t)1 << 31;
  create_refused(bad, K, "at most 2^31 - 1 entries");
  bad = e; bad.n_points = 0;
  create_refused(bad, K, "unsupported shape");
  bad = e; bad.n_coords = 0;
  create_refused(bad, K, "unsupported shape");
  create_refused(e, 0, "K=0");
  create_refused(e, 1025, "K=1025");
  for (long at : {1L, 4L, 7L}) {             // a host exception inside the first upload, the fourth and the last (seven, a synchronisation each)
    hipstub_throw_at_sync(at);
    create_refused(e, K, "injected by the stub");
    hipstub_throw_at_sync(0);
  }
  void* h = &h;
  EXPECT_ERR(bnmtf_kmeans_create_list(e.n_points, e.n_coords, e.n, nullptr, e.coords.data(), e.vals.data(), K, 0, &h), "null argument");
  if (h != nullptr) { fprintf(stderr, "a refused create left a handle\n"); exit(2); }
  h = &h;
  EXPECT_ERR(bnmtf_kmeans_create_list(e.n_points, e.n_coords, e.n, e.points.data(), nullptr, e.vals.data(), K, 0, &h), "null argument");
  EXPECT_ERR(bnmtf_kmeans_create_list(e.n_points, e.n_coords, e.n, e.points.data(), e.coords.data(), nullptr, K, 0, &h), "null argument");
  EXPECT_ERR(bnmtf_kmeans_create_list(e.n_points, e.n_coords, e.n, e.points.data(), e.coords.data(), e.vals.data(), K, 0, nullptr), "null argument");
  EXPECT_ERR(bnmtf_kmeans_build_lists(e.n_points, e.n_coords, e.n, nullptr, e.coords.data(), e.vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "null argument");
  EXPECT_ERR(bnmtf_kmeans_build_lists(0, e.n_coords, e.n, e.points.data(), e.coords.data(), e.vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "unsupported shape");
  OK(bnmtf_kmeans_destroy(nullptr));
}

int main() {
  const long live0 = hipstub_live_allocs();
  refusals();
  walk(37, 23, 3, 0.2, 1);
  walk(5, 700, 41, 0.5, 2);          // (two passes of sums)
  walk(257, 129, 81, 0.03, 3);       // (three passes; K padded to 88 in the transposed centroids)
  walk(1, 1, 1, 1.0, 4);
  walk(9, 130, 1024, 1.0, 5);
  walk(6, 5, 8, 0.0, 6);             // (no entries at all)
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs() - live0); return 2; }
  printf("sanitize driver kmeans: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
