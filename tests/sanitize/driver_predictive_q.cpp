// Test infrastructure (CPU box only): bnmtf_predictive_moments and bnmtf_predictive_moments_times (csrc/api_predictive_q.inc: the
// closed-form predictive mean and variance of a variational model over an entry list) walked on the library's HOST side under
// AddressSanitizer + UBSan (`make asan_predictive_q`), linked against hip_stub.cpp instead of the HIP runtime as
// driver_predictive.cpp is.  Kernels do not run, so no number that comes back means anything; what is checked is the host code the
// call goes through -- the checks of the moments, the sort of the list and the scatter back through its permutation, every
// upload's extent (the arrays are exactly as long as the call may read, so one double too many is a heap overflow the sanitizer
// sees), both forms, each variance null in turn, duplicates --, every refusal, a call that fails midway, and that nothing outlives
// a call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "driver_common.h"

struct Case {
  int I, J, K, L; uint64_t n;
  std::vector<int32_t> rows, cols;
  std::vector<double> EA, VA, ES, VS, EB, VB, mean, var;
};
// a shuffled list with an empty row, the far corner and three entries given twice
static Case make(int I, int J, int K, int L, unsigned seed) {
  std::mt19937 g(seed);
  Case c; c.I = I; c.J = J; c.K = K; c.L = L;
  std::uniform_int_distribution<int> ri(0, I - 1), rj(0, J - 1);
  for (int e = 0; e < 5 * I + 7; ++e) { int i = ri(g); if (i == 1 && I > 2) i = 0; c.rows.push_back(i); c.cols.push_back(rj(g)); }
  c.rows.push_back(I - 1); c.cols.push_back(J - 1);
  for (int d = 0; d < 3; ++d) { c.rows.push_back(c.rows[d]); c.cols.push_back(c.cols[d]); }
  for (size_t e = c.rows.size() - 1; e > 0; --e) { const size_t o = g() % (e + 1); std::swap(c.rows[e], c.rows[o]); std::swap(c.cols[e], c.cols[o]); }
  c.n = c.rows.size();
  const int W = L > 0 ? L : K;
  c.EA.assign((size_t)I * K, 1.0); c.VA.assign((size_t)I * K, 0.5);
  c.EB.assign((size_t)J * W, 1.0); c.VB.assign((size_t)J * W, 0.0);
  if (L > 0) { c.ES.assign((size_t)K * L, 2.0); c.VS.assign((size_t)K * L, 0.25); }
  c.mean.assign(c.n, -1.0); c.var.assign(c.n, -1.0);
  return c;
}
// nulls: bit 0 VA, bit 1 VS, bit 2 VB
static int call(Case& c, int nulls = 0, int device = 0) {
  return bnmtf_predictive_moments(device, c.I, c.J, c.K, c.L, c.n, c.rows.data(), c.cols.data(), c.EA.data(), (nulls & 1) ? nullptr : c.VA.data(),
                                  c.L > 0 ? c.ES.data() : nullptr, (c.L > 0 && !(nulls & 2)) ? c.VS.data() : nullptr, c.EB.data(),
                                  (nulls & 4) ? nullptr : c.VB.data(), c.mean.data(), c.var.data());
}

static void walk(int I, int J, int K, int L, unsigned seed) {
  Case c = make(I, J, K, L, seed);
  for (int nulls = 0; nulls < 8; ++nulls) {
    const long before = hipstub_launches();
    OK(call(c, nulls));
    if (hipstub_launches() - before != (L > 0 ? 2 : 1)) { fprintf(stderr, "walk(%d, %d, %d, %d): %ld launches\n", I, J, K, L, hipstub_launches() - before); exit(2); }
    if (hipstub_live_allocs() != 0) { fprintf(stderr, "walk(%d, %d, %d, %d) nulls %d: %ld allocations outlive the call\n", I, J, K, L, nulls, hipstub_live_allocs()); exit(2); }
    c.mean.assign(c.n, -1.0); c.var.assign(c.n, -1.0);
  }
  // a call that fails at its synchronisation frees what it made and comes back as a status
  hipstub_throw_at_sync(1);
  EXPECT_ERR(call(c), "injected by the stub");
  hipstub_throw_at_sync(0);
  double up = -1.0, kn = -1.0;
  OK(call(c));
  OK(bnmtf_predictive_moments_times(&up, &kn));
  if (!(up >= 0.0) || !(kn >= 0.0)) { fprintf(stderr, "times %g %g\n", up, kn); exit(2); }
}

static void refusals() {
  Case c = make(7, 5, 3, 0, 9);
  Case t = make(7, 5, 3, 2, 9);
  const long before = hipstub_launches();
  int32_t* const r = c.rows.data(); int32_t* const q = c.cols.data();
  double* const EA = c.EA.data(); double* const VA = c.VA.data(); double* const EB = c.EB.data(); double* const VB = c.VB.data();
  double* const ES = t.ES.data(); double* const VS = t.VS.data();
  double* const o = c.mean.data();
#define CALL(I, J, K, L, n, r, q, EA, VA, ES, VS, EB, VB, o0, o1) bnmtf_predictive_moments(0, I, J, K, L, n, r, q, EA, VA, ES, VS, EB, VB, o0, o1)
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, nullptr, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, nullptr, EA, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, nullptr, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, EA, VA, nullptr, nullptr, nullptr, VB, o, o), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, nullptr, o), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, nullptr), "bnmtf_predictive_moments: null argument");
  EXPECT_ERR(CALL(0, 5, 3, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: unsupported shape");
  EXPECT_ERR(CALL(7, 0, 3, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 0, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 257, 0, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, -1, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 257, c.n, r, q, EA, VA, ES, VS, EB, VB, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 2, c.n, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: ES is required when L >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 2, c.n, r, q, EA, VA, nullptr, VS, EB, VB, o, o), "ES is required when L >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, EA, VA, ES, nullptr, EB, VB, o, o), "null when L = 0");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, EA, VA, nullptr, VS, EB, VB, o, o), "null when L = 0");
  EXPECT_ERR(CALL(7, 5, 3, 0, 0, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "bnmtf_predictive_moments: 1 <= n < 2^31");
  EXPECT_ERR(CALL(7, 5, 3, 0, (uint64_t)1 << 31, r, q, EA, VA, nullptr, nullptr, EB, VB, o, o), "1 <= n < 2^31");
#undef CALL
  Case bad = c; bad.rows[4] = 7;
  EXPECT_ERR(call(bad), "bnmtf_predictive_moments: entry 4 (7,");
  bad = c; bad.cols[2] = -1;
  EXPECT_ERR(call(bad), "lies outside the 7 x 5 matrix");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  bad = c; bad.VA.back() = -1e-300;
  EXPECT_ERR(call(bad), "the rows factor holds a variance that is negative or not finite");
  OK(call(bad, 1));                                   // (a variance that is not passed is not read)
  bad = c; bad.VB[0] = inf;
  EXPECT_ERR(call(bad), "the columns factor holds a variance that is negative or not finite");
  bad = c; bad.VB.back() = nan;
  EXPECT_ERR(call(bad), "variance that is negative or not finite");
  bad = t; bad.VS[1] = -2.0;
  EXPECT_ERR(call(bad), "the middle factor holds a variance that is negative or not finite");
  OK(call(bad, 2));
  bad = c; bad.EA[3] = nan;
  EXPECT_ERR(call(bad), "the rows factor holds a mean that is not finite");
  bad = t; bad.ES.back() = inf;
  EXPECT_ERR(call(bad), "the middle factor holds a mean that is not finite");
  bad = t; bad.EB.back() = -inf;
  EXPECT_ERR(call(bad), "the columns factor holds a mean that is not finite");
  EXPECT_ERR(call(c, 0, 5), "hipSetDevice");
  EXPECT_ERR(bnmtf_predictive_moments_times(nullptr, o), "bnmtf_predictive_moments_times: null argument");
  EXPECT_ERR(bnmtf_predictive_moments_times(o, nullptr), "bnmtf_predictive_moments_times: null argument");
  if (hipstub_launches() != before + 3) { fprintf(stderr, "a refused call launched\n"); exit(2); }      // (the two calls above that were taken: 1 + 2 launches)
}

int main() {
  const long start = hipstub_live_allocs();
  walk(37, 23, 3, 0, 1);
  walk(37, 23, 4, 0, 2);
  walk(5, 700, 5, 0, 3);
  walk(1100, 7, 3, 0, 4);
  walk(40, 37, 256, 0, 5);
  walk(37, 23, 3, 5, 6);            // the tri-factorisation
  walk(37, 23, 5, 4, 7);
  walk(11, 9, 256, 2, 8);
  walk(11, 9, 2, 256, 9);
  walk(1, 1, 1, 1, 10);
  refusals();
  if (hipstub_live_allocs() != start) { fprintf(stderr, "%ld allocations outlive the run (%ld at its start)\n", hipstub_live_allocs(), start); return 2; }
  printf("sanitize driver predictive_q: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
