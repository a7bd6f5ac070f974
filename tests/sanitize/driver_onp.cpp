// Test infrastructure (CPU box only): the six bnmtf_onp_* entry points (csrc/api_obs_np.inc: NMF / NMTF on the observed-entry
// layout) walked on the library's HOST side under AddressSanitizer + UBSan (`make asan_onp`), linked against hip_stub.cpp instead of
// the HIP runtime as driver.cpp is.  Kernels do not run, so no number that comes back means anything; what is checked is the host
// code the calls go through -- the create path with null prior rates and two row strides, every host<->"device" copy's extent,
// the S step's pass loop and buffer swap, the single-column calls' hand-over, the metric call's lists --, every refusal, a create
// that fails midway, the handle kinds telling each other apart, and that obs_free gives back every buffer of the new family.
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
    if (rc_ == BNMTF_OK) { fprintf(stderr, "expected an error: %s\n", #expr); exit(2); }             \
    if (!strstr(bnmtf_last_error(), text)) { fprintf(stderr, "%s: the message \"%s\" lacks \"%s\"\n", #expr, bnmtf_last_error(), text); exit(2); } \
  } while (0)

struct Entries { int I, J; std::vector<int32_t> rows, cols; std::vector<float> vals; uint64_t n; };
// about a fifth of the matrix, no empty row or column, in shuffled order
static Entries make_entries(int I, int J, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> p(0.0, 1.0);
  std::uniform_real_distribution<float> u(0.5f, 10.f);
  std::vector<size_t> at;
  for (int i = 0; i < I; ++i)
    for (int j = 0; j < J; ++j)
      if (p(g) < 0.2 || j == i % J || i == j % I) at.push_back((size_t)i * J + j);
  std::shuffle(at.begin(), at.end(), g);
  Entries e; e.I = I; e.J = J;
  for (size_t q : at) { e.rows.push_back((int32_t)(q / J)); e.cols.push_back((int32_t)(q % J)); e.vals.push_back(u(g)); }
  e.n = at.size();
  return e;
}

static int create(const Entries& e, int K, int L, bnmtf_handle* h) {
  return bnmtf_onp_create(e.I, e.J, K, L, e.n, e.rows.data(), e.cols.data(), e.vals.data(), 0, h);
}

// a create that must be refused with `text`, or fail, and leave nothing behind
static void create_refused(const Entries& e, int K, int L, const char* text) {
  const long live = hipstub_live_allocs();
  bnmtf_handle h = reinterpret_cast<bnmtf_handle>(&h);
  EXPECT_ERR(create(e, K, L, &h), text);
  if (h != nullptr || hipstub_live_allocs() != live) { fprintf(stderr, "a refused create (K=%d L=%d) left a handle or %ld allocations\n", K, L, hipstub_live_allocs() - live); exit(2); }
}

// create .. destroy of one handle through all six entry points
static void walk(int I, int J, int K, int L, unsigned seed) {
  const Entries e = make_entries(I, J, seed);
  const bool tri = L > 0;
  const int Wc = tri ? L : K, iters = 3;
  const long live0 = hipstub_live_allocs();
  bnmtf_handle h = nullptr;
  OK(create(e, K, L, &h));
  std::vector<double> A((size_t)I * K, 1.0), S((size_t)K * Wc, 1.0), B((size_t)J * Wc, 1.0), perf((size_t)iters * 3), idiv(iters), times(iters);
  double out8[8];
  double* Sp = tri ? S.data() : nullptr;
  // ahead of set_state
  EXPECT_ERR(bnmtf_onp_run(h, 1, nullptr, nullptr, nullptr), "bnmtf_onp_set_state has not been called");
  EXPECT_ERR(bnmtf_onp_get_state(h, A.data(), Sp, B.data()), "has not been called");
  EXPECT_ERR(bnmtf_onp_update(h, 0, 0, 0), "has not been called");
  EXPECT_ERR(bnmtf_onp_metrics(h, 0, nullptr, nullptr, nullptr, out8), "has not been called");
  EXPECT_ERR(bnmtf_onp_set_state(h, A.data(), tri ? nullptr : S.data(), B.data()), "null argument");
  EXPECT_ERR(bnmtf_onp_set_state(h, nullptr, Sp, B.data()), "null argument");
  OK(bnmtf_onp_set_state(h, A.data(), Sp, B.data()));
  OK(bnmtf_onp_run(h, iters, perf.data(), idiv.data(), times.data()));
  OK(bnmtf_onp_run(h, 0, nullptr, nullptr, nullptr));
  OK(bnmtf_onp_run(h, iters + 2, nullptr, nullptr, nullptr));            // (a longer record: reallocated)
  EXPECT_ERR(bnmtf_onp_run(h, -1, nullptr, nullptr, nullptr), "negative iteration count");
  // the single updates: every column in order (each continues the one before), then out of order, then what is out of range
  for (int k = 0; k < K; ++k) OK(bnmtf_onp_update(h, 0, k, 0));
  if (tri) for (int k = 0; k < K; ++k) for (int l = 0; l < L; ++l) OK(bnmtf_onp_update(h, 1, k, l));
  for (int l = 0; l < Wc; ++l) OK(bnmtf_onp_update(h, 2, 0, l));
  OK(bnmtf_onp_update(h, 0, K - 1, 0)); OK(bnmtf_onp_update(h, 2, 0, Wc - 1));
  EXPECT_ERR(bnmtf_onp_update(h, 0, K, 0), "out of range");
  EXPECT_ERR(bnmtf_onp_update(h, 2, 0, Wc), "out of range");
  EXPECT_ERR(bnmtf_onp_update(h, 3, 0, 0), "out of range");
  if (tri) { EXPECT_ERR(bnmtf_onp_update(h, 1, K, 0), "out of range"); EXPECT_ERR(bnmtf_onp_update(h, 1, 0, L), "out of range"); }
  else EXPECT_ERR(bnmtf_onp_update(h, 1, 0, 0), "out of range");
  // the metric sums: the training entries, the same as a list, a short list, one outside the matrix
  const int32_t fr[3] = {I - 1, 0, I / 2}, fc[3] = {0, J - 1, J / 2}, outside[3] = {0, J, 0};
  const float fv[3] = {1.f, 2.f, 3.f};
  OK(bnmtf_onp_metrics(h, 0, nullptr, nullptr, nullptr, out8));
  OK(bnmtf_onp_metrics(h, e.n, e.rows.data(), e.cols.data(), e.vals.data(), out8));
  OK(bnmtf_onp_metrics(h, 3, fr, fc, fv, out8));
  EXPECT_ERR(bnmtf_onp_metrics(h, 3, fr, outside, fv, out8), "lies outside");
  EXPECT_ERR(bnmtf_onp_metrics(h, 3, nullptr, fc, fv, out8), "null argument");
  EXPECT_ERR(bnmtf_onp_metrics(h, 0, nullptr, nullptr, nullptr, nullptr), "null argument");
  OK(bnmtf_onp_get_state(h, A.data(), Sp, B.data()));
  OK(bnmtf_onp_get_state(h, nullptr, nullptr, nullptr));
  if (!tri) EXPECT_ERR(bnmtf_onp_get_state(h, nullptr, S.data(), nullptr), "no S");
  // the other families' calls refuse the handle, with their own messages
  EXPECT_ERR(bnmf_obs_run(h, 1, BNMTF_UPDATE_MODE, nullptr, nullptr, nullptr, nullptr, nullptr), "not a handle of bnmtf_obs_create");
  EXPECT_ERR(bnmtf_otri_run(h, 1, BNMTF_UPDATE_MODE, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "not a handle of bnmtf_otri_create");
  EXPECT_ERR(bnmf_obs_set_state(h, A.data(), B.data(), 1.0), "not a handle of bnmtf_obs_create");
  EXPECT_ERR(bnmf_vbo_set_state(h, A.data(), A.data(), A.data(), A.data(), B.data(), B.data(), B.data(), B.data(), 1.0), "not a handle of bnmtf_obs_create");
  EXPECT_ERR(bnmtf_otvb_exp_square_diff(h, out8), "not a handle of bnmtf_otri_create");
  EXPECT_ERR(bnmf_np_run(h, 1, nullptr, nullptr, nullptr), "not a handle of bnmtf_np_create");
  EXPECT_ERR(bnmf_set_state(h, A.data(), B.data(), 1.0), "bnmtf_onp_create runs only the bnmtf_onp_*");
  char buf[1024];
  OK(bnmtf_describe(h, buf, sizeof buf));
  if (!strstr(buf, "layout=observed")) { fprintf(stderr, "describe: %s\n", buf); exit(2); }
  OK(bnmtf_destroy(h));
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "walk(%d, %d, %d, %d): %ld allocations outlive the handle\n", I, J, K, L, hipstub_live_allocs() - live0); exit(2); }
}

// ... and the reverse: handles of the two other creates at bnmtf_onp_run
static void other_kinds() {
  const Entries e = make_entries(11, 9, 31);
  std::vector<double> lam((size_t)11 * 9, 0.1);
  const long live0 = hipstub_live_allocs();
  bnmtf_handle a = nullptr, b = nullptr;
  OK(bnmtf_obs_create(e.I, e.J, 3, e.n, e.rows.data(), e.cols.data(), e.vals.data(), lam.data(), lam.data(), 1.0, 1.0, 7, 0, &a));
  OK(bnmtf_otri_create(e.I, e.J, 3, 2, e.n, e.rows.data(), e.cols.data(), e.vals.data(), lam.data(), lam.data(), lam.data(), 1.0, 1.0, 7, 0, &b));
  double out8[8];
  for (bnmtf_handle h : {a, b}) {
    EXPECT_ERR(bnmtf_onp_run(h, 1, nullptr, nullptr, nullptr), "not a handle of bnmtf_onp_create");
    EXPECT_ERR(bnmtf_onp_set_state(h, lam.data(), lam.data(), lam.data()), "not a handle of bnmtf_onp_create");
    EXPECT_ERR(bnmtf_onp_update(h, 0, 0, 0), "not a handle of bnmtf_onp_create");
    EXPECT_ERR(bnmtf_onp_metrics(h, 0, nullptr, nullptr, nullptr, out8), "not a handle of bnmtf_onp_create");
  }
  EXPECT_ERR(bnmtf_onp_run(nullptr, 1, nullptr, nullptr, nullptr), "not a handle of bnmtf_onp_create");
  EXPECT_ERR(bnmtf_onp_get_state(nullptr, nullptr, nullptr, nullptr), "not a handle of bnmtf_onp_create");
  OK(bnmtf_destroy(a)); OK(bnmtf_destroy(b));
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "other_kinds: %ld allocations outlive the handles\n", hipstub_live_allocs() - live0); exit(2); }
}

// what the create refuses, with bnmtf_obs_create's texts, and a create that fails midway
static void refusals() {
  const Entries e = make_entries(37, 23, 51);
  for (int L : {0, 2}) {
    const int K = 3;
    Entries bad = e; bad.cols[5] = e.J;
    create_refused(bad, K, L, "lies outside the 37 x 23 matrix");
    bad = e; bad.rows[7] = bad.rows[3]; bad.cols[7] = bad.cols[3];
    create_refused(bad, K, L, "occurs twice");
    bad = e; bad.rows.clear(); bad.cols.clear(); bad.vals.clear();
    for (uint64_t q = 0; q < e.n; ++q) if (e.rows[q] != 4) { bad.rows.push_back(e.rows[q]); bad.cols.push_back(e.cols[q]); bad.vals.push_back(e.vals[q]); }
    bad.n = bad.rows.size();
    create_refused(bad, K, L, "Fully unobserved row in R, row 4.");
    bad = e; bad.rows.clear(); bad.cols.clear(); bad.vals.clear();
    for (uint64_t q = 0; q < e.n; ++q) if (e.cols[q] != 6) { bad.rows.push_back(e.rows[q]); bad.cols.push_back(e.cols[q]); bad.vals.push_back(e.vals[q]); }
    bad.n = bad.rows.size();
    create_refused(bad, K, L, "Fully unobserved column in R, column 6.");
    bad = e; bad.n = 0;
    create_refused(bad, K, L, "between 1 and 2^31 - 1 entries (n=0)");
    create_refused(e, 257, L, "K=257");
    create_refused(e, 0, L, "K=0");
    create_refused(e, K, 257, "L=257");
    create_refused(e, K, -1, "L=-1");
    for (long at : {2L, 5L}) {              // a host exception inside the first direction's build and the second's (three uploads each)
      hipstub_throw_at_sync(at);
      create_refused(e, K, L, "");
      hipstub_throw_at_sync(0);
    }
  }
  bnmtf_handle h = reinterpret_cast<bnmtf_handle>(&h);
  EXPECT_ERR(bnmtf_onp_create(e.I, e.J, 3, 0, e.n, nullptr, e.cols.data(), e.vals.data(), 0, &h), "null argument");
  if (h != nullptr) { fprintf(stderr, "a refused create left a handle\n"); exit(2); }
  EXPECT_ERR(bnmtf_onp_create(e.I, e.J, 3, 0, e.n, e.rows.data(), e.cols.data(), e.vals.data(), 0, nullptr), "null argument");
}

int main() {
  const long live0 = hipstub_live_allocs();
  refusals();
  walk(37, 23, 3, 0, 1);
  walk(5, 700, 2, 0, 2);             // (rows beyond the register form)
  walk(40, 37, 256, 0, 3);
  walk(37, 23, 3, 5, 4);
  walk(23, 37, 7, 2, 5);
  walk(1030, 7, 2, 3, 6);            // (more S blocks than one fold trip)
  walk(12, 9, 130, 256, 7);
  other_kinds();
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs() - live0); return 2; }
  printf("sanitize driver onp: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
