// Test infrastructure (CPU box only): bnmtf_log_predictive_samples (csrc/api_log_predictive.inc: the log predictive density of known
// values under stored samples over an entry list) walked on the library's HOST side under AddressSanitizer + UBSan (`make
// asan_log_predictive`), linked against hip_stub.cpp instead of the HIP runtime as driver_predictive.cpp is.  Kernels do not run,
// so no number that comes back means anything; what is checked is the host code the call goes through -- the sort of the list, the
// values carried through its permutation and the five outputs scattered back through it, the chunking and every upload's extent
// (the sample arrays, c and h are exactly as long as the call may read, so one element too many is a heap overflow the sanitizer
// sees), both forms, strided samples, duplicates --, every refusal, a call that fails midway, and that nothing outlives a call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "driver_common.h"

struct Case {
  int I, J, K, L, T; uint64_t first, step, n;
  std::vector<int32_t> rows, cols;
  std::vector<double> values, c, h;
  std::vector<float> A, S, B;
  std::vector<double> out[5];
};
// a shuffled list with an empty row, the far corner and three entries given twice; sample arrays that end with the call's last sample
static Case make(int I, int J, int K, int L, int T, uint64_t first, uint64_t step, unsigned seed) {
  std::mt19937 g(seed);
  Case c; c.I = I; c.J = J; c.K = K; c.L = L; c.T = T; c.first = first; c.step = step;
  std::uniform_int_distribution<int> ri(0, I - 1), rj(0, J - 1);
  for (int e = 0; e < 5 * I + 7; ++e) { int i = ri(g); if (i == 1 && I > 2) i = 0; c.rows.push_back(i); c.cols.push_back(rj(g)); }
  c.rows.push_back(I - 1); c.cols.push_back(J - 1);
  for (int d = 0; d < 3; ++d) { c.rows.push_back(c.rows[d]); c.cols.push_back(c.cols[d]); }
  for (size_t e = c.rows.size() - 1; e > 0; --e) { const size_t o = g() % (e + 1); std::swap(c.rows[e], c.rows[o]); std::swap(c.cols[e], c.cols[o]); }
  c.n = c.rows.size();
  c.values.assign(c.n, 1.5);
  c.c.assign(T, -0.25); c.h.assign(T, 0.5);
  const size_t stored = first + (uint64_t)(T - 1) * step + 1;
  const int W = L > 0 ? L : K;
  c.A.assign(stored * I * K, 1.f); c.B.assign(stored * J * W, 1.f);
  if (L > 0) c.S.assign(stored * K * L, 1.f);
  for (auto& o : c.out) o.assign(c.n, -1.0);
  return c;
}
static int call(Case& c, int chunk) {
  return bnmtf_log_predictive_samples(0, c.I, c.J, c.K, c.L, c.n, c.rows.data(), c.cols.data(), c.values.data(), c.A.data(),
                                      c.L > 0 ? c.S.data() : nullptr, c.B.data(), c.first, c.step, c.T, chunk, c.c.data(), c.h.data(),
                                      c.out[0].data(), c.out[1].data(), c.out[2].data(), c.out[3].data(), c.out[4].data());
}

static void walk(int I, int J, int K, int L, int T, uint64_t first, uint64_t step, unsigned seed) {
  Case c = make(I, J, K, L, T, first, step, seed);
  for (int chunk : {0, 1, 2, 5, T, T + 3}) {
    const long before = hipstub_launches();
    OK(call(c, chunk));
    const int eff = chunk == 0 || chunk > T ? T : chunk;
    if (hipstub_launches() - before != (T + eff - 1) / eff) { fprintf(stderr, "chunk %d of %d samples: %ld launches\n", chunk, T, hipstub_launches() - before); exit(2); }
    if (hipstub_live_allocs() != 0) { fprintf(stderr, "walk(%d, %d, %d, %d) chunk %d: %ld allocations outlive the call\n", I, J, K, L, chunk, hipstub_live_allocs()); exit(2); }
    for (auto& o : c.out) {                   // (the stub's device memory is zeroed and no kernel ran: every output was written, through the permutation)
      for (uint64_t e = 0; e < c.n; ++e) if (o[e] != 0.0) { fprintf(stderr, "entry %llu was not written\n", (unsigned long long)e); exit(2); }
      o.assign(c.n, -1.0);
    }
  }
  // a call that fails at its synchronisation frees what it made and comes back as a status
  hipstub_throw_at_sync(1);
  EXPECT_ERR(call(c, 2), "injected by the stub");
  hipstub_throw_at_sync(0);
  double up = -1.0, kn = -1.0;
  OK(call(c, 0));
  OK(bnmtf_log_predictive_times(&up, &kn));
  if (!(up >= 0.0) || !(kn >= 0.0)) { fprintf(stderr, "times %g %g\n", up, kn); exit(2); }
}

static void refusals() {
  Case c = make(7, 5, 3, 0, 2, 0, 1, 9);
  Case t = make(7, 5, 3, 2, 2, 0, 1, 9);
  const long before = hipstub_launches();
  int32_t* const r = c.rows.data(); int32_t* const q = c.cols.data();
  double* const v = c.values.data(); double* const cc = c.c.data(); double* const hh = c.h.data();
  float* const A = c.A.data(); float* const B = c.B.data();
  double* const o = c.out[0].data();
#define CALL(I, J, K, L, n, r, q, v, A, S, B, first, step, T, chunk, cc, hh, o0, o1, o2, o3, o4) \
  bnmtf_log_predictive_samples(0, I, J, K, L, n, r, q, v, A, S, B, first, step, T, chunk, cc, hh, o0, o1, o2, o3, o4)
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, nullptr, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, nullptr, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, nullptr, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, nullptr, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, nullptr, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, nullptr, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, nullptr, o, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, nullptr, o, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, nullptr, o, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, nullptr, o, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, nullptr, o), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, nullptr), "bnmtf_log_predictive_samples: null argument");
  EXPECT_ERR(CALL(0, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: unsupported shape");
  EXPECT_ERR(CALL(7, 0, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 0, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 257, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, -1, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 257, c.n, r, q, v, A, t.S.data(), B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 2, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: S is required when L >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, t.S.data(), B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "null when L = 0");
  EXPECT_ERR(CALL(7, 5, 3, 0, 0, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: 1 <= n < 2^31");
  EXPECT_ERR(CALL(7, 5, 3, 0, (uint64_t)1 << 31, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "1 <= n < 2^31");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 0, 0, cc, hh, o, o, o, o, o), "bnmtf_log_predictive_samples: T >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 0, 2, 0, cc, hh, o, o, o, o, o), "step >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, -1, cc, hh, o, o, o, o, o), "chunk_samples >= 0");
#undef CALL
  Case bad = c; bad.rows[4] = 7;
  EXPECT_ERR(call(bad, 0), "bnmtf_log_predictive_samples: entry 4 (7,");
  bad = c; bad.cols[2] = -1;
  EXPECT_ERR(call(bad, 0), "lies outside the 7 x 5 matrix");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  bad = c; bad.values[3] = nan;
  EXPECT_ERR(call(bad, 0), "bnmtf_log_predictive_samples: values: the value of entry 3 (");
  bad = c; bad.values[c.n - 1] = -inf;
  EXPECT_ERR(call(bad, 0), "is not finite");
  bad = c; bad.c[1] = inf;
  EXPECT_ERR(call(bad, 0), "bnmtf_log_predictive_samples: c[1] is not finite");
  bad = c; bad.c[0] = nan;
  EXPECT_ERR(call(bad, 0), "c[0] is not finite");
  bad = c; bad.h[1] = 0.0;
  EXPECT_ERR(call(bad, 0), "bnmtf_log_predictive_samples: h[1] is not finite and positive");
  bad = c; bad.h[0] = -0.5;
  EXPECT_ERR(call(bad, 0), "h[0] is not finite and positive");
  bad = c; bad.h[1] = inf;
  EXPECT_ERR(call(bad, 0), "h[1] is not finite and positive");
  bad = c; bad.h[0] = nan;
  EXPECT_ERR(call(bad, 0), "h[0] is not finite and positive");
  EXPECT_ERR(bnmtf_log_predictive_samples(5, 7, 5, 3, 0, c.n, r, q, v, A, nullptr, B, 0, 1, 2, 0, cc, hh, o, o, o, o, o), "hipSetDevice");
  EXPECT_ERR(bnmtf_log_predictive_times(nullptr, o), "bnmtf_log_predictive_times: null argument");
  if (hipstub_launches() != before) { fprintf(stderr, "a refused call launched\n"); exit(2); }
}

int main() {
  walk(37, 23, 3, 0, 7, 2, 3, 1);           // strided samples: a copy per sample
  walk(37, 23, 5, 0, 7, 0, 1, 2);           // consecutive samples: a copy per chunk
  walk(5, 700, 4, 0, 4, 1, 1, 3);
  walk(1100, 7, 3, 0, 5, 2, 3, 4);
  walk(40, 37, 256, 0, 3, 0, 2, 5);
  walk(37, 23, 3, 5, 7, 2, 3, 6);           // the tri-factorisation
  walk(37, 23, 5, 3, 7, 0, 1, 7);
  walk(11, 9, 256, 2, 3, 1, 1, 8);
  walk(11, 9, 2, 256, 3, 0, 4, 9);
  refusals();
  if (hipstub_live_allocs() != 0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs()); return 2; }
  printf("sanitize driver log_predictive: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
