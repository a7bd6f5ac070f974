// Test infrastructure (CPU box only): bnmtf_fold_in (csrc/api_foldin.inc: new rows or columns folded into a fitted model) walked on
// the library's HOST side under AddressSanitizer + UBSan (`make asan_foldin`), linked against hip_stub.cpp instead of the HIP runtime
// as driver_top.cpp is.  Kernels do not run, so no number that comes back means anything; what is checked is the host code the call
// goes through -- the checks of the list, the units' offsets, the two fp32 copies of the fixed factor (row stride rounded up to
// four; transposed with a zero word behind every column), every upload's and download's extent (the arrays are exactly as long as
// the call may read or write, so one element too many is a heap overflow the sanitizer sees), both forms, ids null and given,
// samples null and given --, every refusal, a call that fails midway, and that nothing outlives a call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "driver_common.h"

struct Case {
  int n_units, m, W, T;
  std::vector<double> other, lambda, init;
  std::vector<int32_t> unit, idx;
  std::vector<float> values;
  std::vector<uint32_t> ids;
  std::vector<double> first, sd, sd2;
  std::vector<float> samples;
};
// unit u gets counts[u % 4] of {1, 3, m, m / 2 + 1} entries (at most m), ascending indices from a shuffle
static Case make(int n_units, int m, int W, int T, unsigned seed) {
  std::mt19937 g(seed);
  Case c; c.n_units = n_units; c.m = m; c.W = W; c.T = T;
  c.other.assign((size_t)m * W, 1.0); c.lambda.assign((size_t)n_units * W, 1.0); c.init.assign((size_t)n_units * W, 1.0);
  std::vector<int32_t> all(m);
  for (int u = 0; u < n_units; ++u) {
    const int want[4] = {1, 3, m, m / 2 + 1};
    const int cnt = want[u % 4] < m ? want[u % 4] : m;
    for (int j = 0; j < m; ++j) all[j] = j;
    for (int j = m - 1; j > 0; --j) std::swap(all[j], all[g() % (j + 1)]);
    std::vector<int32_t> pick(all.begin(), all.begin() + cnt);
    for (size_t x = 0; x < pick.size(); ++x)
      for (size_t y = x + 1; y < pick.size(); ++y)
        if (pick[y] < pick[x]) std::swap(pick[x], pick[y]);
    for (int32_t j : pick) { c.unit.push_back(u); c.idx.push_back(j); c.values.push_back(1.5f); }
    c.ids.push_back(1000u + (uint32_t)u);
  }
  return c;
}
static int call(Case& c, bool with_ids, bool with_samples, int form, int update = 0, int discard = 0, int keep_every = 1) {
  const size_t nW = (size_t)c.n_units * c.W;
  c.first.assign(nW, 7.0); c.sd.assign(nW, 7.0); c.sd2.assign(nW, 7.0); c.samples.assign(with_samples ? (size_t)c.T * nW : 0, 7.f);
  return bnmtf_fold_in(0, c.n_units, c.m, c.W, c.other.data(), c.unit.size(), c.unit.data(), c.idx.data(), c.values.data(), c.lambda.data(), 2.0,
                       c.init.data(), with_ids ? c.ids.data() : nullptr, 17u, c.T, 3, discard, keep_every, update, 0.0, form,
                       c.first.data(), c.sd.data(), c.sd2.data(), with_samples ? c.samples.data() : nullptr);
}

static void walk(int n_units, int m, int W, int T, unsigned seed) {
  Case c = make(n_units, m, W, T, seed);
  for (int form = 0; form < 2; ++form)
    for (int with_ids = 0; with_ids < 2; ++with_ids)
      for (int with_samples = 0; with_samples < 2; ++with_samples)
        for (int update = 0; update < 2; ++update) {
          const long before = hipstub_launches();
          OK(call(c, with_ids != 0, with_samples != 0, form, update, update ? 0 : T / 2, update ? 1 : 2));
          if (hipstub_launches() - before != 1) { fprintf(stderr, "form %d: %ld launches\n", form, hipstub_launches() - before); exit(2); }
          if (hipstub_live_allocs() != 0) { fprintf(stderr, "walk(%d, %d, %d): %ld allocations outlive the call\n", n_units, m, W, hipstub_live_allocs()); exit(2); }
          for (size_t t = 0; t < c.first.size(); ++t)       // (the stub's device memory is zeroed and no kernel ran: every output was written)
            if (c.first[t] != 0.0 || c.sd[t] != 0.0 || c.sd2[t] != 0.0) { fprintf(stderr, "statistic %zu was not written\n", t); exit(2); }
          for (size_t t = 0; t < c.samples.size(); ++t)
            if (c.samples[t] != 0.f) { fprintf(stderr, "sample %zu was not written\n", t); exit(2); }
        }
  // a call that fails at its synchronisation frees what it made and comes back as a status
  hipstub_throw_at_sync(1);
  EXPECT_ERR(call(c, true, true, 0), "injected by the stub");
  hipstub_throw_at_sync(0);
  double up = -1.0, kn = -1.0;
  OK(call(c, false, false, 0));
  OK(bnmtf_fold_in_times(&up, &kn));
  if (!(up >= 0.0) || !(kn >= 0.0)) { fprintf(stderr, "times %g %g\n", up, kn); exit(2); }
}

static void refusals() {
  Case c = make(5, 9, 3, 4, 9);
  call(c, true, true, 0);
  const long before = hipstub_launches();
  double* const O = c.other.data(); double* const L = c.lambda.data(); double* const X = c.init.data();
  int32_t* const un = c.unit.data(); int32_t* const ix = c.idx.data(); float* const v = c.values.data(); uint32_t* const id = c.ids.data();
  const uint64_t n = c.unit.size();
  double* const o0 = c.first.data(); double* const o1 = c.sd.data(); double* const o2 = c.sd2.data(); float* const os = c.samples.data();
#define CALL(nu, m, W, O, n, un, ix, v, L, tau, X, T, it0, dis, ke, upd, mn, form, o0, o1, o2) \
  bnmtf_fold_in(0, nu, m, W, O, n, un, ix, v, L, tau, X, id, 17u, T, it0, dis, ke, upd, mn, form, o0, o1, o2, os)
  EXPECT_ERR(CALL(5, 9, 3, nullptr, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, nullptr, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, nullptr, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, nullptr, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, nullptr, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, nullptr, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, nullptr, o1, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, nullptr, o2), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, nullptr), "bnmtf_fold_in: null argument");
  EXPECT_ERR(CALL(0, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: unsupported shape");
  EXPECT_ERR(CALL(5, 0, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "unsupported shape");
  EXPECT_ERR(CALL(5, (1 << 30) + 1, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "unsupported shape");
  EXPECT_ERR(CALL(5, 9, 0, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "unsupported shape");
  EXPECT_ERR(CALL(5, 9, 257, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "BNMTF_FOLDIN_MAX_RANK");
  EXPECT_ERR(CALL(5, 9, 3, O, 0, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: 1 <= n < 2^31");
  EXPECT_ERR(CALL(5, 9, 3, O, (uint64_t)1 << 31, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "1 <= n < 2^31");
  EXPECT_ERR(CALL(5, 9, 3, O, 4, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: every unit needs an entry");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 0, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: iterations >= 1");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, -1, 0, 1, 0, 0.0, 0, o0, o1, o2), "first_iteration >= 0");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0x7ffffffe, 0, 1, 0, 0.0, 0, o0, o1, o2), "below 2^31");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 2, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: update is 0 (draw) or 1 (mode)");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 0, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: keep_every >= 1");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 4, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: 0 <= discard < iterations");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, -1, 1, 0, 0.0, 0, o0, o1, o2), "0 <= discard < iterations");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 1, 1, 1, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: a mode chain has one answer");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 2, 1, 0.0, 0, o0, o1, o2), "a mode chain has one answer");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 2, o0, o1, o2), "bnmtf_fold_in: form is 0");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 0.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: tau is positive and finite");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, std::numeric_limits<double>::infinity(), X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "tau is positive and finite");
  EXPECT_ERR(CALL(5, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 1, -1.0, 0, o0, o1, o2), "bnmtf_fold_in: min_x is finite and not negative");
  Case bad = c; bad.unit[2] = 5;
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: entry 2 (5,");
  bad = c; bad.idx[0] = 9;
  EXPECT_ERR(call(bad, true, true, 0), "lies outside the 5 units x 9 indices");
  bad = c; bad.idx[2] = bad.idx[1];
  EXPECT_ERR(call(bad, true, true, 0), "is given twice");
  bad = c; std::swap(bad.idx[1], bad.idx[2]);
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: the list is sorted by (unit, index)");
  EXPECT_ERR(CALL(6, 9, 3, O, n, un, ix, v, L, 2.0, X, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2), "bnmtf_fold_in: unit 5 has no entry");
  bad = c; bad.values[3] = std::numeric_limits<float>::quiet_NaN();
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: the value of entry 3");
  bad = c; bad.other[5] = std::numeric_limits<double>::infinity();
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: the fixed factor holds a value that is not finite");
  bad = c; bad.other[5] = 1e300;
  EXPECT_ERR(call(bad, true, true, 0), "not finite in fp32");
  bad = c; bad.lambda[4] = -1.0;
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: the prior rates are finite and not negative");
  bad = c; bad.init[4] = std::numeric_limits<double>::quiet_NaN();
  EXPECT_ERR(call(bad, true, true, 0), "bnmtf_fold_in: the start holds a value that is not finite");
  EXPECT_ERR(bnmtf_fold_in(5, 5, 9, 3, O, n, un, ix, v, L, 2.0, X, id, 17u, 4, 0, 0, 1, 0, 0.0, 0, o0, o1, o2, os), "hipSetDevice");
  EXPECT_ERR(bnmtf_fold_in_times(nullptr, o0), "bnmtf_fold_in_times: null argument");
#undef CALL
  if (hipstub_launches() != before) { fprintf(stderr, "a refused call launched\n"); exit(2); }
}

int main() {
  walk(1, 1, 1, 1, 1);                    // the smallest call
  walk(7, 23, 3, 5, 2);                   // an odd width: the padded rows of the fixed factor
  walk(9, 700, 4, 3, 3);                  // units beyond 512 entries: the long form's residual array in form 0 as well
  walk(5, 65, 256, 2, 4);
  walk(1100, 7, 2, 2, 5);
  walk(3, 64, 255, 4, 6);
  refusals();
  if (hipstub_live_allocs() != 0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs()); return 2; }
  printf("sanitize driver foldin: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
