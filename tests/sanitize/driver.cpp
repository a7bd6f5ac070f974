// Test infrastructure (CPU box only): drives the C ABI of the library's HOST side, linked against hip_stub.cpp instead of the
// HIP runtime, under AddressSanitizer + UBSan (`make asan`) or ThreadSanitizer (`make tsan`).  Kernels do not run, so no number
// that comes back means anything; what is checked is the host code the calls go through: bnmtf_create's layout passes (worker
// threads, slot tables -- also on their own, from a real mask --, shard ranges, the hand-over table sizes), the arenas and pools of created / destroyed models, every
// host<->"device" copy's extent (device memory is heap memory here), the sample ring of run(), run_many's batching and lock-step walks, the
// in-process multi-rank rendezvous of comm.hip with one host thread per rank, and the observed-entry layout's 24 entry points
// (api_obs*.inc): one state for four models, its lazily allocated variational part, every refusal and the create path's guard.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <numeric>
#include <random>
#include <thread>
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
#define EXPECT_ERR(expr)                                                                             \
  do {                                                                                               \
    const int rc_ = (expr);                                                                          \
    if (rc_ == BNMTF_OK) { fprintf(stderr, "expected an error: %s\n", #expr); exit(2); }             \
  } while (0)

struct Data {
  int I, J;
  std::vector<float> R;
  std::vector<uint8_t> M;
};
static Data make_data(int I, int J, double missing, unsigned seed) {
  Data d{I, J, std::vector<float>((size_t)I * J), std::vector<uint8_t>((size_t)I * J, 1)};
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> u(0.f, 10.f);
  std::uniform_real_distribution<double> p(0.0, 1.0);
  for (auto& x : d.R) x = u(g);
  for (auto& m : d.M) m = p(g) < missing ? 0 : 1;
  for (int i = 0; i < I; ++i) d.M[(size_t)i * J + (i % J)] = 1;          // no empty row ...
  for (int j = 0; j < J; ++j) d.M[(size_t)(j % I) * J + j] = 1;          // ... or column
  return d;
}

static bnmtf_handle create(const Data& d, int K, int L, int rank, int world, const uint8_t* cid, uint64_t seed = 7) {
  std::vector<double> lr((size_t)d.I * K, 0.1), lc((size_t)d.J * (L ? L : K), 0.1), ls((size_t)K * (L ? L : 1), 0.1);
  bnmtf_problem p;
  memset(&p, 0, sizeof p);
  p.I = d.I; p.J = d.J; p.K = K; p.L = L; p.R = d.R.data(); p.M = d.M.data();
  p.lambda_rows = lr.data(); p.lambda_cols = lc.data(); p.lambda_S = L ? ls.data() : nullptr;
  p.alpha = p.beta = 1.0; p.seed = seed; p.device = 0; p.rank = rank; p.world = world; p.comm_id = cid;
  bnmtf_handle h = nullptr;
  OK(bnmtf_create(&p, &h));
  return h;
}

static void bnmf_round_trip(const Data& d, int K, int iters, bool samples) {
  bnmtf_handle h = create(d, K, 0, 0, 1, nullptr);
  std::vector<double> U((size_t)d.I * K, 1.0), V((size_t)d.J * K, 1.0);
  OK(bnmf_set_state(h, U.data(), V.data(), 1.0));
  uint64_t total = 0;
  std::vector<uint32_t> row(d.I), col(d.J);
  OK(bnmtf_omega_counts(h, &total, row.data(), col.data()));
  uint64_t expect = 0;
  for (uint8_t m : d.M) expect += m;
  if (total != expect) { fprintf(stderr, "omega count %llu != %llu\n", (unsigned long long)total, (unsigned long long)expect); exit(2); }
  std::vector<float> Uo, Vo;
  if (samples) { Uo.resize((size_t)iters * d.I * K); Vo.resize((size_t)iters * d.J * K); }
  std::vector<double> tau(iters), perf((size_t)iters * 3), times(iters);
  OK(bnmf_gibbs_run(h, iters, BNMTF_UPDATE_DRAW, samples ? Uo.data() : nullptr, samples ? Vo.data() : nullptr, tau.data(), perf.data(), times.data()));
  OK(bnmf_gibbs_run(h, 2, BNMTF_UPDATE_MODE, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::vector<double> num(d.I), tp(d.I);
  OK(bnmf_cond_params(h, 0, K - 1, num.data(), tp.data()));
  EXPECT_ERR(bnmf_cond_params(h, 0, K, num.data(), tp.data()));
  OK(bnmtf_set_expectation(h, 1, 2));
  OK(bnmf_gibbs_run(h, 5, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr));
  double t = 0; uint64_t cnt = 0;
  OK(bnmtf_get_expectation(h, U.data(), nullptr, V.data(), &t, &cnt));
  OK(bnmf_get_state(h, U.data(), V.data(), &t));
  // the metric entry points: the handle's own operand copies (part of a small model's arena), and factors wider than 64 columns
  double sums[6];
  OK(bnmtf_beta_s(h, &t));
  OK(bnmtf_metric_sums(h, nullptr, U.data(), nullptr, V.data(), sums));
  {
    const int Kw = 96;
    std::vector<double> A((size_t)d.I * Kw, 0.5), B((size_t)d.J * Kw, 0.5);
    OK(bnmtf_metric_sums_wide(h, d.M.data(), A.data(), B.data(), Kw, sums));
    OK(bnmtf_metric_sums(h, nullptr, U.data(), nullptr, V.data(), sums));
  }
  char buf[2048];
  OK(bnmtf_describe(h, buf, sizeof buf));
  OK(bnmtf_destroy(h));
}

// the slot layout's host half on its own (bnmtf_slot_layout; csrc/slot_layout.hip) on a REAL random mask -- under the stub no kernel
// runs, so the lists bnmtf_create "downloads" are whatever the heap held --: balancing, parking and the threaded fills, into
// buffers of exactly the sizes the first call reports
static void slot_layout_walk(int n, int m, int KP, double missing, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> p(0.0, 1.0);
  std::vector<uint32_t> ptr(n + 1, 0), idx;
  for (int u = 0; u < n; ++u) {
    const double frac = missing * 2.0 * p(g);                   // ragged: several slot classes, over-full residue classes
    for (int j = 0; j < m; ++j) if (p(g) < frac) idx.push_back((uint32_t)j);
    ptr[u + 1] = (uint32_t)idx.size();
  }
  int64_t info[BNMTF_SLOT_INFO_LEN], again[BNMTF_SLOT_INFO_LEN];
  OK(bnmtf_slot_layout(n, m, KP, 1, ptr.data(), idx.data(), info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  const int64_t* sz = info + BNMTF_SLOT_INFO_LEN - 11;
  std::vector<int32_t> unit_map(sz[0]), gen(sz[5]), u_unit_map(sz[7]);
  std::vector<uint32_t> pair_E(sz[1]), pair_base(sz[2]), off(sz[3]), off16(sz[4]), u_pair_E(sz[8]), u_pair_base(sz[9]), u_off16(sz[10]);
  std::vector<uint16_t> row_blk(sz[6]);
  OK(bnmtf_slot_layout(n, m, KP, 1, ptr.data(), idx.data(), again, unit_map.data(), pair_E.data(), pair_base.data(), off.data(), off16.data(), gen.data(),
                       row_blk.data(), u_unit_map.data(), u_pair_E.data(), u_pair_base.data(), u_off16.data()));
  if (memcmp(info, again, sizeof info) != 0) { fprintf(stderr, "slot layout: two calls, two answers\n"); exit(2); }
  EXPECT_ERR(bnmtf_slot_layout(n, m, 48, 1, ptr.data(), idx.data(), info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
}

// a C++ exception inside an entry point comes back as a status with its message; the handle is still good afterwards
static void exception_stays_inside(const Data& d, int K) {
  bnmtf_handle h = create(d, K, 0, 0, 1, nullptr);
  std::vector<double> U((size_t)d.I * K, 1.0), V((size_t)d.J * K, 1.0);
  OK(bnmf_set_state(h, U.data(), V.data(), 1.0));
  hipstub_throw_at_sync(1);
  const int rc = bnmf_gibbs_run(h, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (rc != BNMTF_EINVAL || !strstr(bnmtf_last_error(), "injected by the stub")) { fprintf(stderr, "exception guard: rc %d, message '%s'\n", rc, bnmtf_last_error()); exit(1); }
  hipstub_throw_at_sync(0);
  OK(bnmf_gibbs_run(h, 2, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
  OK(bnmtf_destroy(h));
}

static void vb_round_trip(const Data& d, int K) {
  bnmtf_handle h = create(d, K, 0, 0, 1, nullptr);
  std::vector<double> a((size_t)d.I * K, 1.0), b((size_t)d.J * K, 1.0);
  OK(bnmf_vb_set_state(h, a.data(), a.data(), a.data(), a.data(), b.data(), b.data(), b.data(), b.data(), 1.0));
  std::vector<double> et(4), perf(12), times(4), elbo(40);
  OK(bnmf_vb_run(h, 4, et.data(), perf.data(), elbo.data(), times.data()));
  double e = 0;
  OK(bnmf_vb_exp_square_diff(h, &e));
  OK(bnmtf_destroy(h));
}

// SAN_VERBOSE: the stub's launch counter before and after a scenario's calls (name = null: nothing, the scenario shares the counter
// with another thread).  The lock-step scenarios launch once per group of records that meet at a site, so equal counts before and
// after a change to the driver say that the same records still meet.
struct LaunchCount {
  const char* name;
  long before;
  explicit LaunchCount(const char* name_) : name(name_), before(hipstub_launches()) {}
  ~LaunchCount() { if (name && getenv("SAN_VERBOSE")) printf("%s: %ld stub launches before, %ld after\n", name, before, hipstub_launches()); }
};

// several variational models in lock-step (api_many.inc): the recorder, the argument lists, the per-model outputs; two shapes and a
// model given once only
static void vb_many(const Data& d1, const Data& d2, int K, const char* report) {
  LaunchCount count(report);
  std::vector<bnmtf_handle> hs;
  const long live0 = hipstub_live_allocs();
  for (int m = 0; m < 5; ++m) {
    const Data& d = m == 3 ? d2 : d1;
    bnmtf_handle h = create(d, m == 1 ? K + 3 : K, 0, 0, 1, nullptr);
    const int Km = m == 1 ? K + 3 : K;
    std::vector<double> a((size_t)d.I * Km, 1.0), b((size_t)d.J * Km, 1.0);
    OK(bnmf_vb_set_state(h, a.data(), a.data(), a.data(), a.data(), b.data(), b.data(), b.data(), b.data(), 1.0));
    hs.push_back(h);
  }
  const int n = (int)hs.size(), it = 3;
  std::vector<double> et((size_t)n * it), perf((size_t)n * it * 3), elbo((size_t)n * it * 10), times((size_t)n * it);
  int info[2];
  OK(bnmf_vb_run_many(hs.data(), n, it, et.data(), perf.data(), elbo.data(), times.data(), info));
  const int shared = info[0];
  OK(bnmf_vb_run_many(hs.data(), n, 2, nullptr, nullptr, nullptr, nullptr, nullptr));
  OK(bnmf_vb_run_many(hs.data(), 1, 2, et.data(), nullptr, nullptr, nullptr, info));
  const long live1 = hipstub_live_allocs();
  for (bnmtf_handle h : hs) OK(bnmtf_destroy(h));
  if (report && getenv("SAN_VERBOSE")) printf("vb_many: live allocations %ld before, %ld with five models, %ld after; %d models shared launches\n", live0, live1, hipstub_live_allocs(), shared);
}

static void tri_vb_set_state(bnmtf_handle h, const Data& d, int K, int L) {
  std::vector<double> F((size_t)d.I * K, 1.0), S((size_t)K * L, 1.0), G((size_t)d.J * L, 1.0);
  OK(bnmtf_vb_set_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
}

// several variational tri-factorisations in lock-step: models of different (K, L) -- one with K L >= 64, whose chain walks the
// permuted system: a site the others do not have -- and shapes; `wide`: also a model whose row sweep takes the 16-wave shape, which
// runs on its own.  Calls one behind the other (the first iteration of the first has sites the later ones do not), and one after a
// single model's state was set again (its first iteration then differs from the others').
static void tri_vb_many(const Data& d1, const Data& d2, bool wide, const char* report) {
  LaunchCount count(report);
  const Data dw = make_data(wide ? 6200 : 1, wide ? 90 : 1, 0.1, 35);
  struct Shape { const Data* d; int K, L; };
  std::vector<Shape> shapes = {{&d1, 4, 5}, {&d1, 6, 3}, {&d2, 9, 8}, {&d2, 4, 5}};
  if (wide) shapes.push_back({&dw, 5, 4});
  std::vector<bnmtf_handle> hs;
  for (const Shape& sh : shapes) {
    hs.push_back(create(*sh.d, sh.K, sh.L, 0, 1, nullptr));
    tri_vb_set_state(hs.back(), *sh.d, sh.K, sh.L);
  }
  const int n = (int)hs.size(), it = 3;
  std::vector<std::vector<int32_t>> orders;
  std::vector<const int32_t*> op;
  for (const Shape& sh : shapes) {
    const int per = sh.K * sh.L + sh.K + sh.L;
    orders.emplace_back((size_t)it * per);
    for (int t = 0; t < it; ++t) {
      int32_t* o = &orders.back()[(size_t)t * per];
      for (int a = 0; a < sh.K * sh.L; ++a) o[a] = (a + t) % (sh.K * sh.L);
      for (int k = 0; k < sh.K; ++k) o[sh.K * sh.L + k] = sh.K - 1 - k;
      for (int l = 0; l < sh.L; ++l) o[sh.K * sh.L + sh.K + l] = (l + t) % sh.L;
    }
  }
  for (auto& o : orders) op.push_back(o.data());
  std::vector<double> et((size_t)n * it), perf((size_t)n * it * 3), elbo((size_t)n * it * 10), times((size_t)n * it);
  int info[2];
  OK(bnmtf_vb_run_many(hs.data(), n, it, op.data(), et.data(), perf.data(), elbo.data(), times.data(), info));
  if (report && getenv("SAN_VERBOSE")) printf("%s: %d of %d models shared launches\n", report, info[0], n);
  OK(bnmtf_vb_run_many(hs.data(), n, 2, op.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
  tri_vb_set_state(hs[1], *shapes[1].d, shapes[1].K, shapes[1].L);
  OK(bnmtf_vb_run_many(hs.data(), n, 2, op.data(), et.data(), nullptr, nullptr, nullptr, info));
  OK(bnmtf_vb_run_many(hs.data(), 1, 2, op.data(), et.data(), nullptr, nullptr, nullptr, info));
  EXPECT_ERR(bnmtf_vb_run_many(hs.data(), n, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::vector<bnmtf_handle> dup = {hs[0], hs[1], hs[0]};
  EXPECT_ERR(bnmtf_vb_run_many(dup.data(), 3, 2, op.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
  for (bnmtf_handle h : hs) OK(bnmtf_destroy(h));
}

// NMF and NMTF models in lock-step: different ranks, so the S chains differ in length (the shorter ones have no record at the
// later passes) and NMF's two sweeps meet NMTF's; with and without outputs; a single model
static void np_many(const Data& d1, const Data& d2, const char* report) {
  LaunchCount count(report);
  struct Shape { const Data* d; int K, L; };
  const std::vector<Shape> shapes = {{&d1, 5, 0}, {&d1, 3, 4}, {&d2, 8, 0}, {&d2, 5, 6}, {&d1, 2, 2}};
  std::vector<bnmtf_handle> hs;
  for (const Shape& sh : shapes) {
    const Data& d = *sh.d;
    bnmtf_handle h = nullptr;
    OK(bnmtf_np_create(d.R.data(), d.M.data(), d.I, d.J, sh.K, sh.L, 0, &h));
    std::vector<double> F((size_t)d.I * sh.K, 1.0), S((size_t)sh.K * (sh.L ? sh.L : 1), 1.0), G((size_t)d.J * (sh.L ? sh.L : sh.K), 1.0);
    if (sh.L) OK(bnmtf_np_set_state(h, F.data(), S.data(), G.data()));
    else OK(bnmf_np_set_state(h, F.data(), G.data()));
    hs.push_back(h);
  }
  const int n = (int)hs.size(), it = 3;
  std::vector<double> perf((size_t)n * it * 3), idiv((size_t)n * it), times((size_t)n * it);
  int info[2];
  OK(bnmtf_np_run_many(hs.data(), n, it, perf.data(), idiv.data(), times.data(), info));
  if (report && getenv("SAN_VERBOSE")) printf("%s: %d of %d models shared launches\n", report, info[0], n);
  OK(bnmtf_np_run_many(hs.data(), n, 2, nullptr, nullptr, nullptr, nullptr));
  OK(bnmtf_np_run_many(hs.data() + 1, 1, 2, perf.data(), idiv.data(), times.data(), info));
  OK(bnmtf_np_run_many(hs.data(), 0, 2, nullptr, nullptr, nullptr, info));
  std::vector<bnmtf_handle> dup = {hs[0], hs[1], hs[0]};
  EXPECT_ERR(bnmtf_np_run_many(dup.data(), 3, 2, nullptr, nullptr, nullptr, nullptr));
  for (bnmtf_handle h : hs) OK(bnmtf_destroy(h));
}

// the variational tri-factorisation: set_state / run with shuffled orders / the direct exp_square_diff / single updates / get_state
static void tri_vb_round_trip(const Data& d, int K, int L, int iters) {
  bnmtf_handle h = create(d, K, L, 0, 1, nullptr);
  std::vector<double> F((size_t)d.I * K, 1.0), S((size_t)K * L, 1.0), G((size_t)d.J * L, 1.0);
  OK(bnmtf_vb_set_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
  const int per = K * L + K + L;
  std::vector<int32_t> orders((size_t)iters * per);
  for (int it = 0; it < iters; ++it) {
    int32_t* o = &orders[(size_t)it * per];
    for (int a = 0; a < K * L; ++a) o[a] = K * L - 1 - a;
    for (int k = 0; k < K; ++k) o[K * L + k] = (k + it) % K;
    for (int l = 0; l < L; ++l) o[K * L + K + l] = L - 1 - l;
  }
  std::vector<double> et(iters), perf((size_t)iters * 3), times(iters), elbo((size_t)iters * 10);
  OK(bnmtf_vb_run(h, iters, orders.data(), et.data(), perf.data(), elbo.data(), times.data()));
  double e = 0, sums[6];
  OK(bnmtf_vb_exp_square_diff(h, &e, sums));
  OK(bnmtf_vb_update(h, 0, K - 1, 0, 1));
  OK(bnmtf_vb_update(h, 1, K - 1, L - 1, 1));
  OK(bnmtf_vb_update(h, 2, 0, L - 1, 0));
  OK(bnmtf_vb_get_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data()));
  OK(bnmtf_destroy(h));
}

static void tri_round_trip(const Data& d, int K, int L, int iters) {
  bnmtf_handle h = create(d, K, L, 0, 1, nullptr);
  std::vector<double> F((size_t)d.I * K, 1.0), S((size_t)K * L, 1.0), G((size_t)d.J * L, 1.0);
  OK(bnmtf_set_state(h, F.data(), S.data(), G.data(), 1.0));
  std::vector<float> Fo((size_t)iters * d.I * K), So((size_t)iters * K * L), Go((size_t)iters * d.J * L);
  std::vector<double> tau(iters), perf((size_t)iters * 3);
  OK(bnmtf_gibbs_run(h, iters, BNMTF_UPDATE_DRAW, Fo.data(), So.data(), Go.data(), tau.data(), perf.data(), nullptr));
  double t;
  OK(bnmtf_get_state(h, F.data(), S.data(), G.data(), &t));
  OK(bnmtf_destroy(h));
}

// the one-launch path's batch entry points: models of different sizes, a duplicate handle (must be refused), a wrong-kind handle
static void batches() {
  std::vector<Data> ds;
  std::vector<bnmtf_handle> hs;
  for (int i = 0; i < 5; ++i) {
    ds.push_back(make_data(60 + 17 * i, 50 + 11 * i, 0.1, 100 + i));
  }
  for (int i = 0; i < 5; ++i) {
    hs.push_back(create(ds[i], 4 + i, 0, 0, 1, nullptr, 11 + i));
    std::vector<double> U((size_t)ds[i].I * (4 + i), 1.0), V((size_t)ds[i].J * (4 + i), 1.0);
    OK(bnmf_set_state(hs.back(), U.data(), V.data(), 1.0));
  }
  OK(bnmf_gibbs_run_many(hs.data(), (int)hs.size(), 6, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::vector<bnmtf_handle> dup = {hs[0], hs[1], hs[0]};
  (void)bnmf_gibbs_run_many(dup.data(), 3, 2, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);   // refused when both take the one-launch path
  Data dt = make_data(70, 60, 0.1, 5);
  bnmtf_handle tri = create(dt, 4, 3, 0, 1, nullptr);
  std::vector<double> F(70 * 4, 1.0), S(12, 1.0), G(60 * 3, 1.0);
  OK(bnmtf_set_state(tri, F.data(), S.data(), G.data(), 1.0));
  std::vector<bnmtf_handle> mixed = {hs[0], tri};
  EXPECT_ERR(bnmf_gibbs_run_many(mixed.data(), 2, 2, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  EXPECT_ERR(bnmtf_gibbs_run_many(mixed.data(), 2, 2, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::vector<bnmtf_handle> tris = {tri};
  OK(bnmtf_gibbs_run_many(tris.data(), 1, 3, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  OK(bnmtf_destroy(tri));
  for (auto h : hs) OK(bnmtf_destroy(h));
  // pooled arenas: create / destroy in a loop, as a model search does
  for (int i = 0; i < 6; ++i) {
    bnmtf_handle h = create(ds[i % 5], 5, 0, 0, 1, nullptr);
    OK(bnmtf_destroy(h));
  }
}

// a factorisation wider than 64 columns as two column blocks (bnmtf_amd/_blocked.py's call sequence)
static void column_blocks(const Data& d) {
  bnmtf_handle a = create(d, 64, 0, 0, 1, nullptr), b = create(d, 17, 0, 0, 1, nullptr);
  OK(bnmf_set_column_block(a, 0)); OK(bnmf_set_column_block(b, 64));
  std::vector<double> Ua((size_t)d.I * 64, 1.0), Va((size_t)d.J * 64, 1.0), Ub((size_t)d.I * 17, 1.0), Vb((size_t)d.J * 17, 1.0);
  OK(bnmf_set_state(a, Ua.data(), Va.data(), 1.0)); OK(bnmf_set_state(b, Ub.data(), Vb.data(), 1.0));
  for (int it = 0; it < 2; ++it)
    for (int which = 0; which < 2; ++which) {
      OK(bnmf_set_residual_data(a, &b, 1)); OK(bnmf_half_sweep(a, which, BNMTF_UPDATE_DRAW));
      OK(bnmf_set_residual_data(b, &a, 1)); OK(bnmf_half_sweep(b, which, BNMTF_UPDATE_MODE));
    }
  OK(bnmtf_set_tau(a, 0.5)); OK(bnmtf_set_iteration(a, 3));
  EXPECT_ERR(bnmf_set_residual_data(a, &a, 1));
  OK(bnmf_set_residual_data(a, nullptr, 0));
  std::vector<double> num(d.I), tp(d.I);
  OK(bnmf_cond_params(b, 0, 16, num.data(), tp.data()));
  OK(bnmf_vb_set_state(a, Ua.data(), Ua.data(), Ua.data(), Ua.data(), Va.data(), Va.data(), Va.data(), Va.data(), 1.0));
  OK(bnmf_vb_set_state(b, Ub.data(), Ub.data(), Ub.data(), Ub.data(), Vb.data(), Vb.data(), Vb.data(), Vb.data(), 1.0));
  OK(bnmf_set_residual_data(b, &a, 1)); OK(bnmf_vb_half_sweep(b, 0)); OK(bnmf_vb_half_sweep(b, 1));
  double t2[2];
  OK(bnmf_vb_esd_terms(b, t2));
  {   // the read-only hook on the column maxima of the masked product's grid: both factors, every pointer optional
    uint32_t posted[128], own[128];
    int was = -1;
    OK(bnmf_vb_column_maxima(b, 0, posted, own, &was)); OK(bnmf_vb_column_maxima(a, 1, posted, own, &was));
    OK(bnmf_vb_column_maxima(a, 0, nullptr, own, nullptr)); OK(bnmf_vb_column_maxima(a, 0, posted, nullptr, nullptr));
    EXPECT_ERR(bnmf_vb_column_maxima(b, 2, posted, own, &was));
  }
  OK(bnmtf_destroy(a)); OK(bnmtf_destroy(b));
}

// a block of the S of a wider tri-factorisation: a BNMTF handle on the data minus what two carriers (BNMF handles) explain
static void tri_blocks(const Data& d) {
  bnmtf_handle c0 = create(d, 40, 0, 0, 1, nullptr), c1 = create(d, 9, 0, 0, 1, nullptr), t = create(d, 33, 40, 0, 1, nullptr);
  OK(bnmf_set_column_block(c0, 0)); OK(bnmf_set_column_block(c1, 64));
  OK(bnmtf_set_s_block(t, 64, 0, 49));
  EXPECT_ERR(bnmtf_set_s_block(t, 0, 20, 49));                 // (the block would stick out of the wide S)
  EXPECT_ERR(bnmtf_set_s_block(c0, 0, 0, 40));                 // (a BNMF handle)
  std::vector<double> U0((size_t)d.I * 40, 0.5), V0((size_t)d.J * 40, 0.5), U1((size_t)d.I * 9, 0.5), V1((size_t)d.J * 9, 0.5);
  OK(bnmf_set_state(c0, U0.data(), V0.data(), 1.0)); OK(bnmf_set_state(c1, U1.data(), V1.data(), 1.0));
  std::vector<double> F((size_t)d.I * 33, 0.3), S((size_t)33 * 40, 0.3), G((size_t)d.J * 40, 0.3);
  OK(bnmtf_set_state(t, F.data(), S.data(), G.data(), 1.0));
  bnmtf_handle cs[2] = {c0, c1};
  OK(bnmf_set_residual_data(t, cs, 2));
  OK(bnmtf_set_iteration(t, 2));
  OK(bnmtf_s_rows(t, 0, 33, BNMTF_UPDATE_DRAW));
  OK(bnmtf_s_rows(t, 5, 6, BNMTF_UPDATE_ICM));
  EXPECT_ERR(bnmtf_s_rows(t, 3, 40, BNMTF_UPDATE_DRAW));
  EXPECT_ERR(bnmtf_s_rows(c0, 0, 1, BNMTF_UPDATE_DRAW));
  OK(bnmtf_get_state(t, nullptr, S.data(), nullptr, nullptr));
  double num, tp;
  OK(bnmtf_cond_params(t, 1, 32, 39, &num, &tp));
  OK(bnmtf_destroy(c0)); OK(bnmtf_destroy(c1)); OK(bnmtf_destroy(t));
}

// ---- the observed-entry layout (api_obs.inc, api_obs_tri.inc, api_obs_trivb.inc) ------------------------------------------------
// the mask's entries as the list the layout's calls take, in shuffled order
struct Entries { std::vector<int32_t> rows, cols; std::vector<float> vals; uint64_t n; };
static Entries entry_list(const Data& d, unsigned seed) {
  std::vector<size_t> at;
  for (size_t p = 0; p < d.M.size(); ++p) if (d.M[p]) at.push_back(p);
  std::mt19937 g(seed);
  std::shuffle(at.begin(), at.end(), g);
  Entries e;
  for (size_t p : at) { e.rows.push_back((int32_t)(p / d.J)); e.cols.push_back((int32_t)(p % d.J)); e.vals.push_back(d.R[p]); }
  e.n = at.size();
  return e;
}

// L = 0: bnmtf_obs_create, else bnmtf_otri_create; the status comes back, the handle in *h
static int obs_create(const Data& d, const Entries& e, int K, int L, bnmtf_handle* h) {
  std::vector<double> lr((size_t)d.I * K, 0.1), lc((size_t)d.J * (L ? L : K), 0.1), ls((size_t)K * (L ? L : 1), 0.1);
  if (L == 0) return bnmtf_obs_create(d.I, d.J, K, e.n, e.rows.data(), e.cols.data(), e.vals.data(), lr.data(), lc.data(), 1.0, 1.0, 7, 0, h);
  return bnmtf_otri_create(d.I, d.J, K, L, e.n, e.rows.data(), e.cols.data(), e.vals.data(), lr.data(), ls.data(), lc.data(), 1.0, 1.0, 7, 0, h);
}

// a create that must be refused, or fail, and leave nothing behind
static void obs_create_refused(const Data& d, const Entries& e, int K, int L) {
  const long live = hipstub_live_allocs();
  bnmtf_handle h = reinterpret_cast<bnmtf_handle>(&h);
  EXPECT_ERR(obs_create(d, e, K, L, &h));
  if (h != nullptr || hipstub_live_allocs() != live) { fprintf(stderr, "a refused create (K=%d L=%d) left a handle or %ld allocations\n", K, L, hipstub_live_allocs() - live); exit(2); }
}

// create .. destroy of one handle: the sampler's calls, the variational ones (whose first set_state allocates), the sampler's again
static void obs_walk(int I, int J, int K, int L, unsigned seed) {
  const Data d = make_data(I, J, 0.8, seed);
  const Entries e = entry_list(d, seed + 1);
  const bool tri = L > 0;
  const int Wc = tri ? L : K, iters = 3;
  const long live0 = hipstub_live_allocs();
  bnmtf_handle h = nullptr;
  OK(obs_create(d, e, K, L, &h));
  std::vector<double> F((size_t)I * K, 1.0), S((size_t)K * Wc, 1.0), G((size_t)J * Wc, 1.0), tau(iters), perf((size_t)iters * 3), times(iters);
  std::vector<float> Fo((size_t)iters * I * K), So((size_t)iters * K * Wc), Go((size_t)iters * J * Wc);
  std::vector<double> num(std::max(I, J)), tp(std::max(I, J));
  double t = 0, sums[6];
  auto set_state = [&] { if (tri) OK(bnmtf_otri_set_state(h, F.data(), S.data(), G.data(), 1.0)); else OK(bnmf_obs_set_state(h, F.data(), G.data(), 1.0)); };
  auto run = [&](int update, bool outputs) {
    float* fo = outputs ? Fo.data() : nullptr; float* so = outputs ? So.data() : nullptr; float* go = outputs ? Go.data() : nullptr;
    double* ta = outputs ? tau.data() : nullptr; double* pe = outputs ? perf.data() : nullptr; double* ti = outputs ? times.data() : nullptr;
    if (tri) OK(bnmtf_otri_run(h, iters, update, fo, so, go, ta, pe, ti)); else OK(bnmf_obs_run(h, iters, update, fo, go, ta, pe, ti));
  };
  // the variational calls ahead of their set_state
  const int per = K * Wc + K + Wc;
  std::vector<int32_t> orders((size_t)iters * per);
  for (int it = 0; it < iters; ++it) {
    int32_t* o = &orders[(size_t)it * per];
    for (int a = 0; a < K * Wc; ++a) o[a] = K * Wc - 1 - a;
    for (int k = 0; k < K; ++k) o[K * Wc + k] = (k + it) % K;
    for (int l = 0; l < Wc; ++l) o[K * Wc + K + l] = Wc - 1 - l;
  }
  if (tri) EXPECT_ERR(bnmtf_otvb_run(h, 1, orders.data(), nullptr, nullptr, nullptr, nullptr)); else EXPECT_ERR(bnmf_vbo_run(h, 1, nullptr, nullptr, nullptr, nullptr));
  set_state();
  run(BNMTF_UPDATE_DRAW, true); run(BNMTF_UPDATE_MODE, true); run(BNMTF_UPDATE_ICM, false);
  if (tri) {
    OK(bnmtf_otri_cond_params(h, 0, K - 1, 0, num.data(), tp.data()));
    OK(bnmtf_otri_cond_params(h, 1, K - 1, L - 1, num.data(), tp.data()));
    OK(bnmtf_otri_cond_params(h, 2, 0, L - 1, num.data(), tp.data()));
    EXPECT_ERR(bnmtf_otri_cond_params(h, 0, K, 0, num.data(), tp.data()));
    EXPECT_ERR(bnmtf_otri_cond_params(h, 2, 0, L, num.data(), tp.data()));
    EXPECT_ERR(bnmtf_otri_cond_params(h, 1, K, 0, num.data(), tp.data()));
  } else {
    OK(bnmf_obs_cond_params(h, 0, K - 1, num.data(), tp.data()));
    OK(bnmf_obs_cond_params(h, 1, 0, num.data(), tp.data()));
    EXPECT_ERR(bnmf_obs_cond_params(h, 0, K, num.data(), tp.data()));
  }
  // the metric sums: the training list, a short list of other entries, one outside the matrix
  const int32_t fr[3] = {I - 1, 0, I / 2}, fc[3] = {0, J - 1, J / 2}, outside[3] = {0, J, 0};
  const float fv[3] = {1.f, 2.f, 3.f};
  if (tri) {
    OK(bnmtf_otri_metric_sums(h, e.n, e.rows.data(), e.cols.data(), e.vals.data(), F.data(), S.data(), G.data(), sums));
    OK(bnmtf_otri_metric_sums(h, 3, fr, fc, fv, F.data(), S.data(), G.data(), sums));
    EXPECT_ERR(bnmtf_otri_metric_sums(h, 3, fr, outside, fv, F.data(), S.data(), G.data(), sums));
    OK(bnmtf_otri_get_state(h, F.data(), S.data(), G.data(), &t));
  } else {
    OK(bnmf_obs_metric_sums(h, e.n, e.rows.data(), e.cols.data(), e.vals.data(), F.data(), G.data(), sums));
    OK(bnmf_obs_metric_sums(h, 3, fr, fc, fv, F.data(), G.data(), sums));
    EXPECT_ERR(bnmf_obs_metric_sums(h, 3, fr, outside, fv, F.data(), G.data(), sums));
    OK(bnmf_obs_get_state(h, F.data(), G.data(), &t));
  }
  // the dense calls and the other kind's refuse the handle
  EXPECT_ERR(bnmf_set_state(h, F.data(), G.data(), 1.0));
  EXPECT_ERR(bnmf_gibbs_run(h, 1, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr));
  EXPECT_ERR(bnmtf_metric_sums(h, nullptr, F.data(), nullptr, G.data(), sums));
  if (tri) EXPECT_ERR(bnmf_obs_run(h, 1, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr));
  else EXPECT_ERR(bnmtf_otri_run(h, 1, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  if (tri) EXPECT_ERR(bnmf_vbo_set_state(h, F.data(), F.data(), F.data(), F.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
  else EXPECT_ERR(bnmtf_otvb_set_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
  // the variational model: the first set_state allocates, the second must not
  std::vector<double> et(iters), elbo((size_t)iters * 10);
  auto vb_set_state = [&] {
    if (tri) OK(bnmtf_otvb_set_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
    else OK(bnmf_vbo_set_state(h, F.data(), F.data(), F.data(), F.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
  };
  const long live1 = hipstub_live_allocs();
  vb_set_state();
  const long live2 = hipstub_live_allocs();
  vb_set_state();
  if (live2 <= live1 || hipstub_live_allocs() != live2) { fprintf(stderr, "variational buffers: %ld, %ld, %ld live allocations\n", live1, live2, hipstub_live_allocs()); exit(2); }
  if (tri) {
    EXPECT_ERR(bnmtf_otri_run(h, 1, BNMTF_UPDATE_DRAW, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));     // (a variational state)
    OK(bnmtf_otvb_run(h, iters, orders.data(), et.data(), perf.data(), elbo.data(), times.data()));
    EXPECT_ERR(bnmtf_otvb_run(h, 1, nullptr, nullptr, nullptr, nullptr, nullptr));
    for (int m = 0; m < 2; ++m) {
      OK(bnmtf_otvb_update(h, 0, K - 1, 0, m)); OK(bnmtf_otvb_update(h, 1, K - 1, L - 1, m)); OK(bnmtf_otvb_update(h, 2, 0, L - 1, m));
    }
    EXPECT_ERR(bnmtf_otvb_update(h, 0, K, 0, 1)); EXPECT_ERR(bnmtf_otvb_update(h, 2, 0, L, 1)); EXPECT_ERR(bnmtf_otvb_update(h, 3, 0, 0, 1));
    OK(bnmtf_otvb_exp_square_diff(h, &t));
    OK(bnmtf_otvb_get_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data()));
  } else {
    OK(bnmf_vbo_run(h, iters, et.data(), perf.data(), elbo.data(), times.data()));
    OK(bnmf_vbo_run(h, 1, nullptr, nullptr, nullptr, nullptr));
    for (int m = 0; m < 2; ++m) { OK(bnmf_vbo_update(h, 0, K - 1, m)); OK(bnmf_vbo_update(h, 1, 0, m)); }
    EXPECT_ERR(bnmf_vbo_update(h, 1, K, 1)); EXPECT_ERR(bnmf_vbo_update(h, 2, 0, 1));
    OK(bnmf_vbo_exp_square_diff(h, &t));
    OK(bnmf_vbo_get_state(h, F.data(), F.data(), F.data(), F.data(), G.data(), G.data(), G.data(), G.data()));
    OK(bnmf_obs_run(h, 1, BNMTF_UPDATE_MODE, nullptr, nullptr, nullptr, nullptr, nullptr));      // (two factors: the sampler runs on the expectations)
  }
  // the sampler's set_state ends the variational state
  set_state();
  run(BNMTF_UPDATE_DRAW, true);
  if (tri) EXPECT_ERR(bnmtf_otvb_exp_square_diff(h, &t)); else EXPECT_ERR(bnmf_vbo_exp_square_diff(h, &t));
  char buf[1024];
  OK(bnmtf_describe(h, buf, sizeof buf));
  OK(bnmtf_destroy(h));
  if (hipstub_live_allocs() != live0) { fprintf(stderr, "obs_walk(%d, %d, %d, %d): %ld allocations outlive the handle\n", I, J, K, L, hipstub_live_allocs() - live0); exit(2); }
}

// what the creates refuse, a create that fails midway, and the host builder of the lists on its own
static void obs_refusals() {
  const Data d = make_data(37, 23, 0.8, 51);
  const Entries e = entry_list(d, 52);
  for (int L : {0, 2}) {
    const int K = 3;
    Entries bad = e; bad.cols[5] = d.J;                                   // an entry outside the matrix
    obs_create_refused(d, bad, K, L);
    bad = e; bad.rows[7] = bad.rows[3]; bad.cols[7] = bad.cols[3];        // an entry twice
    obs_create_refused(d, bad, K, L);
    bad = Entries();                                                      // row 4 without entries
    for (uint64_t q = 0; q < e.n; ++q) if (e.rows[q] != 4) { bad.rows.push_back(e.rows[q]); bad.cols.push_back(e.cols[q]); bad.vals.push_back(e.vals[q]); }
    bad.n = bad.rows.size();
    obs_create_refused(d, bad, K, L);
    bad = e; bad.n = 0;
    obs_create_refused(d, bad, K, L);
    obs_create_refused(d, e, L ? 33 : 257, L);
    if (L) obs_create_refused(d, e, K, 33);
    for (long at : {3L, 7L}) {                                            // a host exception inside the first and the second direction's build (four uploads each)
      hipstub_throw_at_sync(at);
      obs_create_refused(d, e, K, L);
      hipstub_throw_at_sync(0);
    }
  }
  std::vector<uint32_t> rptr(d.I + 1), ridx(e.n), cptr(d.J + 1), cidx(e.n);
  std::vector<float> rval(e.n), cval(e.n);
  OK(bnmtf_obs_build_lists(d.I, d.J, e.n, e.rows.data(), e.cols.data(), e.vals.data(), rptr.data(), ridx.data(), rval.data(), cptr.data(), cidx.data(), cval.data()));
  OK(bnmtf_obs_build_lists(d.I, d.J, e.n, e.rows.data(), e.cols.data(), e.vals.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  if (rptr[d.I] != e.n || cptr[d.J] != e.n) { fprintf(stderr, "bnmtf_obs_build_lists: %u / %u of %llu entries\n", rptr[d.I], cptr[d.J], (unsigned long long)e.n); exit(2); }
  EXPECT_ERR(bnmtf_obs_build_lists(d.I, d.J, 0, e.rows.data(), e.cols.data(), e.vals.data(), rptr.data(), ridx.data(), rval.data(), cptr.data(), cidx.data(), cval.data()));
}

// `world` ranks of this process, one thread each, joined by the in-process transport (communicator id "BNMTFLOC...")
static void sharded(const Data& d, int K, int L, int world, const char* token, int iters) {
  uint8_t cid[128];
  memset(cid, 0, sizeof cid);
  snprintf(reinterpret_cast<char*>(cid), sizeof cid, "BNMTFLOC%s", token);
  std::vector<std::thread> ts;
  std::vector<int> rc(world, 0);
  for (int r = 0; r < world; ++r)
    ts.emplace_back([&, r] {
      bnmtf_handle h = create(d, K, L, r, world, cid);
      if (L == 0) {
        std::vector<double> U((size_t)d.I * K, 1.0), V((size_t)d.J * K, 1.0);
        OK(bnmf_set_state(h, U.data(), V.data(), 1.0));
        std::vector<float> Uo((size_t)iters * d.I * K), Vo((size_t)iters * d.J * K);
        OK(bnmf_gibbs_run(h, iters, BNMTF_UPDATE_DRAW, Uo.data(), Vo.data(), nullptr, nullptr, nullptr));
        OK(bnmf_vb_set_state(h, U.data(), U.data(), U.data(), U.data(), V.data(), V.data(), V.data(), V.data(), 1.0));
        OK(bnmf_vb_run(h, 2, nullptr, nullptr, nullptr, nullptr));
      } else {
        std::vector<double> F((size_t)d.I * K, 1.0), S((size_t)K * L, 1.0), G((size_t)d.J * L, 1.0);
        OK(bnmtf_set_state(h, F.data(), S.data(), G.data(), 1.0));
        OK(bnmtf_gibbs_run(h, iters, BNMTF_UPDATE_MODE, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        // ... and the variational tri-factorisation over the same ranks (round 6)
        OK(bnmtf_vb_set_state(h, F.data(), F.data(), F.data(), F.data(), S.data(), S.data(), S.data(), S.data(), G.data(), G.data(), G.data(), G.data(), 1.0));
        const int per = K * L + K + L;
        std::vector<int32_t> orders((size_t)2 * per);
        for (int it = 0; it < 2; ++it) {
          int32_t* o = &orders[(size_t)it * per];
          for (int a = 0; a < K * L; ++a) o[a] = (a + it) % (K * L);
          for (int k = 0; k < K; ++k) o[K * L + k] = K - 1 - k;
          for (int l = 0; l < L; ++l) o[K * L + K + l] = l;
        }
        OK(bnmtf_vb_run(h, 2, orders.data(), nullptr, nullptr, nullptr, nullptr));
        EXPECT_ERR(bnmtf_vb_update(h, 0, 0, 0, 1));          // (single updates are single-GPU hooks)
      }
      OK(bnmtf_destroy(h));
      rc[r] = 1;
    });
  for (auto& t : ts) t.join();
  for (int r = 0; r < world; ++r) if (!rc[r]) { fprintf(stderr, "rank %d did not finish\n", r); exit(2); }
}

int main(int argc, char** argv) {
  const bool quick = argc > 1 && !strcmp(argv[1], "quick");
  int n = 0;
  OK(bnmtf_device_count(&n));
  int64_t first, count;
  for (int w = 1; w <= 8; ++w) for (int r = 0; r < w; ++r) OK(bnmtf_shard_range(1000 + w, r, w, &first, &count));
  EXPECT_ERR(bnmtf_shard_range(10, 3, 2, &first, &count));

  // small models (the one-launch path's arena), then shapes that take the multi-launch structures: the 8-wave and -- with
  // enough units -- the 16-wave slot layout, the two-chunk inner extent, a mask with rows the on-chip kernels refuse
  bnmf_round_trip(make_data(100, 80, 0.1, 1), 10, 6, true);
  bnmf_round_trip(make_data(640, 512, 0.12, 2), 24, 9, true);            // sample ring: more iterations than its depth
  bnmf_round_trip(make_data(1, 40, 0.0, 3), 3, 3, true);
  bnmf_round_trip(make_data(40, 1, 0.0, 4), 1, 3, false);
  bnmf_round_trip(make_data(300, 200, 0.9, 5), 8, 3, true);              // 90 % missing
  vb_round_trip(make_data(515, 389, 0.12, 6), 40);
  tri_round_trip(make_data(100, 80, 0.1, 7), 5, 5, 4);
  tri_round_trip(make_data(400, 300, 0.1, 8), 32, 17, 3);
  tri_vb_round_trip(make_data(90, 70, 0.1, 15), 4, 5, 3);
  tri_vb_round_trip(make_data(1200, 1100, 0.1, 16), 12, 9, 2);         // the on-chip F / G sweeps' host side, the blocked chain's (K L >= 64)
  batches();
  slot_layout_walk(37, 77, 32, 0.3, 41);
  slot_layout_walk(900, 700, 64, 0.3, 42);                               // enough units for the helper threads of the layout passes
  exception_stays_inside(make_data(515, 389, 0.12, 27), 24);
  vb_many(make_data(300, 120, 0.15, 21), make_data(210, 150, 0.1, 22), 12, "vb_many");
  tri_vb_many(make_data(300, 120, 0.15, 31), make_data(210, 150, 0.1, 32), true, "tri_vb_many");
  np_many(make_data(300, 120, 0.15, 33), make_data(210, 150, 0.1, 34), "np_many");
  {   // two host threads, a list of models each (the recorder is thread-local)
    const Data da = make_data(280, 110, 0.15, 23), db = make_data(190, 160, 0.1, 24), dc = make_data(260, 100, 0.2, 25), dd = make_data(150, 170, 0.1, 26);
    LaunchCount count("two threads of vb_many, tri_vb_many, np_many");
    std::thread t1([&] { vb_many(da, db, 10, nullptr); tri_vb_many(da, db, false, nullptr); np_many(da, db, nullptr); });
    std::thread t2([&] { vb_many(dc, dd, 14, nullptr); tri_vb_many(dc, dd, false, nullptr); np_many(dc, dd, nullptr); });
    t1.join(); t2.join();
  }
  column_blocks(make_data(150, 120, 0.15, 21));
  column_blocks(make_data(70, 60, 0.1, 22));             // (blocks that qualify for the one-launch arena)
  tri_blocks(make_data(130, 110, 0.12, 23));
  tri_blocks(make_data(60, 50, 0.1, 24));
  obs_walk(37, 23, 5, 0, 61);                            // row stride 8: padded
  obs_walk(19, 21, 64, 0, 62);                           // row stride = K
  obs_walk(37, 23, 3, 2, 63);
  obs_walk(33, 31, 32, 32, 64);                          // row stride = W
  obs_refusals();
  sharded(make_data(640, 512, 0.12, 9), 24, 0, 2, "a2", 5);
  sharded(make_data(515, 389, 0.12, 10), 40, 0, 3, "a3", 5);
  sharded(make_data(300, 260, 0.1, 11), 8, 6, 2, "t2", 3);
  if (!quick) {
    bnmf_round_trip(make_data(6200, 6144, 0.1, 12), 64, 3, false);       // >= 192 blocks of 32 units: the 16-wave layout + hand-over tables
    bnmf_round_trip(make_data(700, 12288, 0.1, 13), 16, 2, false);       // inner extent of two LDS panels for the rows direction
    sharded(make_data(2048, 2048, 0.1, 14), 64, 0, 8, "a8", 2);
  }
  printf("sanitize driver: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
