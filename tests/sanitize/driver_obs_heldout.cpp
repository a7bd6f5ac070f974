// Test infrastructure (CPU box only): bnmtf_set_heldout_entries and the held-out hooks of bnmf_obs_run / bnmf_vbo_run
// (csrc/api_obs.inc: run(M_test=Entries) on the observed-entry layout) walked on the library's HOST side under AddressSanitizer +
// UBSan (`make asan_obs_heldout`), linked against hip_stub.cpp instead of the HIP runtime as driver_onp.cpp is.  Kernels do not run,
// so no number that comes back means anything; what is checked is the host code the calls go through -- the sort of the list,
// every upload's extent, set / replace / clear, the record's growth over run calls, bnmtf_get_heldout's copy --, every refusal,
// a build that fails midway, and that nothing outlives the handle.
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
// about the share `p` of the matrix, with a diagonal that leaves no row or column empty, in shuffled order
static Entries make_entries(int I, int J, double share, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> p(0.0, 1.0);
  std::uniform_real_distribution<float> u(0.5f, 10.f);
  std::vector<size_t> at;
  for (int i = 0; i < I; ++i)
    for (int j = 0; j < J; ++j)
      if (p(g) < share || j == i % J || i == j % I) at.push_back((size_t)i * J + j);
  std::shuffle(at.begin(), at.end(), g);
  Entries e; e.I = I; e.J = J;
  for (size_t q : at) { e.rows.push_back((int32_t)(q / J)); e.cols.push_back((int32_t)(q % J)); e.vals.push_back(u(g)); }
  e.n = at.size();
  return e;
}

static int set(bnmtf_handle h, const Entries& e) { return bnmtf_set_heldout_entries(h, e.n, e.rows.data(), e.cols.data(), e.vals.data()); }

static void walk(int I, int J, int K, bool variational, unsigned seed) {
  const Entries train = make_entries(I, J, 0.2, seed), held = make_entries(I, J, 0.1, seed + 100), held2 = make_entries(I, J, 0.4, seed + 200);
  const long live0 = hipstub_live_allocs();
  std::vector<double> lamU((size_t)I * K, 0.1), lamV((size_t)J * K, 0.1), U((size_t)I * K, 1.0), V((size_t)J * K, 1.0);
  bnmtf_handle h = nullptr;
  OK(bnmtf_obs_create(I, J, K, train.n, train.rows.data(), train.cols.data(), train.vals.data(), lamU.data(), lamV.data(), 1.0, 1.0, 7, 0, &h));
  if (variational) OK(bnmf_vbo_set_state(h, U.data(), U.data(), U.data(), U.data(), V.data(), V.data(), V.data(), V.data(), 1.0));
  else OK(bnmf_obs_set_state(h, U.data(), V.data(), 1.0));
  auto run = [&](int it) {
    std::vector<double> tau(it), perf((size_t)it * 3), terms((size_t)it * 10), times(it);
    return variational ? bnmf_vbo_run(h, it, tau.data(), perf.data(), terms.data(), times.data())
                       : bnmf_obs_run(h, it, BNMTF_UPDATE_MODE, nullptr, nullptr, tau.data(), perf.data(), times.data());
  };
  std::vector<double> sums((size_t)8 * 6);
  // no list: a run launches nothing more and leaves no record
  long before = hipstub_launches();
  OK(run(2));
  const long per_iteration = (hipstub_launches() - before) / 2;
  EXPECT_ERR(bnmtf_get_heldout(h, 1, sums.data()), "no held-out mask set");
  // set: two launches more per iteration, and the record
  OK(set(h, held));
  before = hipstub_launches();
  OK(run(3));
  if (hipstub_launches() - before != 3 * (per_iteration + 2)) { fprintf(stderr, "a run with a list: %ld launches, %ld per iteration without\n", hipstub_launches() - before, per_iteration); exit(2); }
  OK(bnmtf_get_heldout(h, 3, sums.data()));
  EXPECT_ERR(bnmtf_get_heldout(h, 4, sums.data()), "recorded 3 iterations");
  OK(run(8));                                   // (a longer record: reallocated)
  OK(bnmtf_get_heldout(h, 8, sums.data()));
  OK(run(1));
  EXPECT_ERR(bnmtf_get_heldout(h, 2, sums.data()), "recorded 1 iterations");
  // replace (a longer list), the training entries themselves (an overlap is allowed), a single entry at the far corner
  OK(set(h, held2)); OK(run(2)); OK(bnmtf_get_heldout(h, 2, sums.data()));
  OK(set(h, train)); OK(run(1)); OK(bnmtf_get_heldout(h, 1, sums.data()));
  const int32_t cr[1] = {I - 1}, cc[1] = {J - 1}; const float cv[1] = {2.f};
  OK(bnmtf_set_heldout_entries(h, 1, cr, cc, cv)); OK(run(1)); OK(bnmtf_get_heldout(h, 1, sums.data()));
  // what is refused leaves the list that was there
  Entries bad = held; bad.cols[2] = J;
  EXPECT_ERR(set(h, bad), "lies outside");
  bad = held; bad.rows[1] = -1;
  EXPECT_ERR(set(h, bad), "entry 1 (-1,");
  bad = held; bad.rows[5] = bad.rows[3]; bad.cols[5] = bad.cols[3];
  EXPECT_ERR(set(h, bad), "occurs twice (position");
  OK(run(1)); OK(bnmtf_get_heldout(h, 1, sums.data()));
  // a build that fails midway (the first synchronisation is the call's own, the next three its uploads') frees what it made
  OK(bnmtf_set_heldout_entries(h, 0, nullptr, nullptr, nullptr));
  const long live1 = hipstub_live_allocs();          // (the handle without a list)
  for (long at : {2L, 3L, 4L}) {
    hipstub_throw_at_sync(at);
    EXPECT_ERR(set(h, held), "");
    hipstub_throw_at_sync(0);
    if (hipstub_live_allocs() != live1) { fprintf(stderr, "a failed build (sync %ld) left %ld allocations\n", at, hipstub_live_allocs() - live1); exit(2); }
    EXPECT_ERR(bnmtf_get_heldout(h, 0, sums.data()), "no held-out mask set");
  }
  // clear, each way; then a run is what it was without a list
  OK(set(h, held)); OK(bnmtf_set_heldout_entries(h, 0, nullptr, nullptr, nullptr));
  OK(set(h, held)); OK(bnmtf_set_heldout_entries(h, held.n, nullptr, held.cols.data(), held.vals.data()));
  OK(bnmtf_set_heldout_entries(h, 0, nullptr, nullptr, nullptr));      // (nothing to clear)
  if (hipstub_live_allocs() != live1) { fprintf(stderr, "a cleared list left %ld allocations\n", hipstub_live_allocs() - live1); exit(2); }
  before = hipstub_launches();
  OK(run(2));
  if (hipstub_launches() - before != 2 * per_iteration) { fprintf(stderr, "a run after the clear: %ld launches\n", hipstub_launches() - before); exit(2); }
  EXPECT_ERR(bnmtf_get_heldout(h, 1, sums.data()), "no held-out mask set");
  // the dense layout's call keeps refusing the handle; a list left on the handle goes with it
  std::vector<double> mask((size_t)I * J, 1.0);
  EXPECT_ERR(bnmtf_set_heldout(h, mask.data()), "bnmtf_obs_create runs only");
  OK(set(h, held2)); OK(run(2));
  OK(bnmtf_destroy(h));
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "walk(%d, %d, %d): %ld allocations outlive the handle\n", I, J, K, hipstub_live_allocs() - live0); exit(2); }
}

// the handles of the other families, and none (a handle of bnmtf_create is refused by the same test as bnmtf_np_create's -- it has
// no ObsState --; its stream and arena go to the per-process pool when it is destroyed, which would outlive this program's count)
static void other_kinds() {
  const Entries e = make_entries(11, 9, 0.3, 31);
  std::vector<double> lam((size_t)11 * 9, 0.1);
  std::vector<float> R((size_t)11 * 9, 1.f);
  std::vector<uint8_t> M((size_t)11 * 9, 1);
  const long live0 = hipstub_live_allocs();
  bnmtf_handle tri = nullptr, onp = nullptr, np = nullptr;
  OK(bnmtf_otri_create(e.I, e.J, 3, 2, e.n, e.rows.data(), e.cols.data(), e.vals.data(), lam.data(), lam.data(), lam.data(), 1.0, 1.0, 7, 0, &tri));
  OK(bnmtf_onp_create(e.I, e.J, 3, 0, e.n, e.rows.data(), e.cols.data(), e.vals.data(), 0, &onp));
  OK(bnmtf_np_create(R.data(), M.data(), 11, 9, 3, 0, 0, &np));
  EXPECT_ERR(set(tri, e), "a handle of bnmtf_otri_create");
  EXPECT_ERR(set(onp, e), "a handle of bnmtf_onp_create");
  EXPECT_ERR(set(np, e), "a handle of bnmtf_np_create");
  for (bnmtf_handle h : {tri, onp, np}) EXPECT_ERR(bnmtf_set_heldout_entries(h, 0, nullptr, nullptr, nullptr), "the two-factor handle of bnmtf_obs_create");
  EXPECT_ERR(set(nullptr, e), "null handle");
  OK(bnmtf_destroy(tri)); OK(bnmtf_destroy(onp)); OK(bnmtf_destroy(np));
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "other_kinds: %ld allocations outlive the handles\n", hipstub_live_allocs() - live0); exit(2); }
}

int main() {
  const long live0 = hipstub_live_allocs();
  for (int variational = 0; variational < 2; ++variational) {
    walk(37, 23, 3, variational != 0, 1);
    walk(5, 700, 2, variational != 0, 2);          // (held-out rows of several wave steps)
    walk(1100, 7, 5, variational != 0, 3);         // (more blocks than one trip of the fold)
    walk(40, 37, 256, variational != 0, 4);
  }
  other_kinds();
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs() - live0); return 2; }
  printf("sanitize driver obs_heldout: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
