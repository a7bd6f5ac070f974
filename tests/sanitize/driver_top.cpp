// Test infrastructure (CPU box only): bnmtf_top_entries (csrc/api_top.inc: the n best predicted entries per row) walked on the
// library's HOST side under AddressSanitizer + UBSan (`make asan_top`), linked against hip_stub.cpp instead of the HIP runtime as
// driver_predictive.cpp is.  Kernels do not run, so no number that comes back means anything; what is checked is the host code the
// call goes through -- the gather of the rows asked for, the counting sort and the deduplication of the exclusion list, the padded
// copy of an odd-width B, every upload's extent (the arrays are exactly as long as the call may read, so one element too many is a
// heap overflow the sanitizer sees), both forms, rows null and given, splits from 1 to more than there are column steps --, every
// refusal, a call that fails midway, and that nothing outlives a call.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "driver_common.h"

struct Case {
  int I, J, K, L, n;
  std::vector<double> A, S, B;
  std::vector<int32_t> rows, ex_rows, ex_cols;
  std::vector<int32_t> cols; std::vector<double> scores; std::vector<int32_t> counts;
};
// a shuffled exclusion list with an empty row, a full row, the far corner and three entries given twice; `rows` a shuffled half of
// the rows; output arrays exactly as long as the call may write
static Case make(int I, int J, int K, int L, int n, unsigned seed) {
  std::mt19937 g(seed);
  Case c; c.I = I; c.J = J; c.K = K; c.L = L; c.n = n;
  const int W = L > 0 ? L : K;
  c.A.assign((size_t)I * K, 1.0); c.B.assign((size_t)J * W, 1.0);
  if (L > 0) c.S.assign((size_t)K * L, 1.0);
  std::uniform_int_distribution<int> ri(0, I - 1), rj(0, J - 1);
  for (int e = 0; e < 3 * I + 7; ++e) { int i = ri(g); if (i == 1 && I > 2) i = 0; c.ex_rows.push_back(i); c.ex_cols.push_back(rj(g)); }
  for (int j = 0; j < J; ++j) { c.ex_rows.push_back(I - 1); c.ex_cols.push_back(j); }
  for (int d = 0; d < 3; ++d) { c.ex_rows.push_back(c.ex_rows[d]); c.ex_cols.push_back(c.ex_cols[d]); }
  for (size_t e = c.ex_rows.size() - 1; e > 0; --e) { const size_t o = g() % (e + 1); std::swap(c.ex_rows[e], c.ex_rows[o]); std::swap(c.ex_cols[e], c.ex_cols[o]); }
  std::vector<int32_t> all(I);
  for (int i = 0; i < I; ++i) all[i] = i;
  for (int i = I - 1; i > 0; --i) std::swap(all[i], all[g() % (i + 1)]);
  c.rows.assign(all.begin(), all.begin() + (I + 1) / 2);
  return c;
}
static int call(Case& c, bool with_rows, int split, int largest = 1) {
  const size_t r = with_rows ? c.rows.size() : (size_t)c.I;
  c.cols.assign(r * c.n, 7); c.scores.assign(r * c.n, 7.0); c.counts.assign(r, 7);
  return bnmtf_top_entries(0, c.I, c.J, c.K, c.L, c.A.data(), c.L > 0 ? c.S.data() : nullptr, c.B.data(), with_rows ? c.rows.size() : 0,
                           with_rows ? c.rows.data() : nullptr, c.ex_rows.size(), c.ex_rows.data(), c.ex_cols.data(), c.n, largest, split,
                           c.cols.data(), c.scores.data(), c.counts.data());
}

static void walk(int I, int J, int K, int L, int n, unsigned seed) {
  Case c = make(I, J, K, L, n, seed);
  const int steps = (J + 63) / 64;
  for (int with_rows = 0; with_rows < 2; ++with_rows)
    for (int split : {0, 1, 2, 3, steps, steps + 5}) {
      const long before = hipstub_launches();
      OK(call(c, with_rows != 0, split, split & 1));
      if (hipstub_launches() - before != (L > 0 ? 3 : 2)) { fprintf(stderr, "split %d: %ld launches\n", split, hipstub_launches() - before); exit(2); }
      if (hipstub_live_allocs() != 0) { fprintf(stderr, "walk(%d, %d, %d, %d) split %d: %ld allocations outlive the call\n", I, J, K, L, split, hipstub_live_allocs()); exit(2); }
      for (size_t t = 0; t < c.cols.size(); ++t)       // (the stub's device memory is zeroed and no kernel ran: every output was written)
        if (c.cols[t] != 0 || c.scores[t] != 0.0) { fprintf(stderr, "slot %zu was not written\n", t); exit(2); }
      for (size_t t = 0; t < c.counts.size(); ++t)
        if (c.counts[t] != 0) { fprintf(stderr, "count %zu was not written\n", t); exit(2); }
    }
  // no exclusion list at all: null lists with n_excl = 0
  {
    std::vector<int32_t> cols((size_t)I * n); std::vector<double> scores((size_t)I * n); std::vector<int32_t> counts(I);
    OK(bnmtf_top_entries(0, I, J, K, L, c.A.data(), L > 0 ? c.S.data() : nullptr, c.B.data(), 0, nullptr, 0, nullptr, nullptr, n, 1, 0,
                         cols.data(), scores.data(), counts.data()));
  }
  // a call that fails at its synchronisation frees what it made and comes back as a status
  hipstub_throw_at_sync(1);
  EXPECT_ERR(call(c, true, 2), "injected by the stub");
  hipstub_throw_at_sync(0);
  double up = -1.0, kn = -1.0;
  OK(call(c, false, 0));
  OK(bnmtf_top_entries_times(&up, &kn));
  if (!(up >= 0.0) || !(kn >= 0.0)) { fprintf(stderr, "times %g %g\n", up, kn); exit(2); }
}

static void refusals() {
  Case c = make(7, 5, 3, 0, 4, 9);
  Case t = make(7, 5, 3, 2, 4, 9);
  call(c, true, 0);
  const long before = hipstub_launches();
  double* const A = c.A.data(); double* const B = c.B.data(); double* const S = t.S.data();
  int32_t* const r = c.rows.data(); const uint64_t nr = c.rows.size();
  int32_t* const er = c.ex_rows.data(); int32_t* const ec = c.ex_cols.data(); const uint64_t ne = c.ex_rows.size();
  int32_t* const oc = c.cols.data(); double* const os = c.scores.data(); int32_t* const on = c.counts.data();
#define CALL(I, J, K, L, A, S, B, nr, r, ne, er, ec, n, lg, sp, oc, os, on) bnmtf_top_entries(0, I, J, K, L, A, S, B, nr, r, ne, er, ec, n, lg, sp, oc, os, on)
  EXPECT_ERR(CALL(7, 5, 3, 0, nullptr, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, nullptr, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, nullptr, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, nullptr, 4, 1, 0, oc, os, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, nullptr, os, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, nullptr, on), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, nullptr), "bnmtf_top_entries: null argument");
  EXPECT_ERR(CALL(0, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: unsupported shape");
  EXPECT_ERR(CALL(7, 0, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, (1 << 30) + 1, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 0, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 257, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, -1, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 257, A, S, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "unsupported shape");
  EXPECT_ERR(CALL(7, 5, 3, 2, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: S is required when L >= 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, S, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "null when L = 0");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 0, 1, 0, oc, os, on), "bnmtf_top_entries: 1 <= n <= 128");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 129, 1, 0, oc, os, on), "1 <= n <= 128");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 2, 0, oc, os, on), "bnmtf_top_entries: largest is 0 or 1");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, -1, oc, os, on), "bnmtf_top_entries: 0 <= split <= 1024");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 1025, oc, os, on), "0 <= split <= 1024");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, 0, r, ne, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: 1 <= n_rows <= I");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, 8, r, ne, er, ec, 4, 1, 0, oc, os, on), "1 <= n_rows <= I");
  EXPECT_ERR(CALL(7, 5, 3, 0, A, nullptr, B, nr, r, (uint64_t)1 << 32, er, ec, 4, 1, 0, oc, os, on), "bnmtf_top_entries: n_excl < 2^32");
  Case bad = c; bad.rows[1] = 7;
  EXPECT_ERR(call(bad, true, 0), "bnmtf_top_entries: rows[1] = 7 lies outside the 7 rows");
  bad = c; bad.rows[2] = bad.rows[0];
  EXPECT_ERR(call(bad, true, 0), "occurs twice");
  bad = c; bad.ex_rows[4] = 7;
  EXPECT_ERR(call(bad, true, 0), "bnmtf_top_entries: excluded entry 4 (7,");
  bad = c; bad.ex_cols[2] = -1;
  EXPECT_ERR(call(bad, false, 0), "lies outside the 7 x 5 matrix");
  bad = c; bad.A[5] = std::numeric_limits<double>::quiet_NaN();
  EXPECT_ERR(call(bad, false, 0), "bnmtf_top_entries: a factor holds a value that is not finite");
  bad = c; bad.B[14] = std::numeric_limits<double>::infinity();
  EXPECT_ERR(call(bad, true, 0), "not finite");
  bad = t; bad.S[5] = -std::numeric_limits<double>::infinity();
  EXPECT_ERR(call(bad, true, 0), "not finite");
  EXPECT_ERR(bnmtf_top_entries(5, 7, 5, 3, 0, A, nullptr, B, nr, r, ne, er, ec, 4, 1, 0, oc, os, on), "hipSetDevice");
  EXPECT_ERR(bnmtf_top_entries_times(nullptr, os), "bnmtf_top_entries_times: null argument");
#undef CALL
  if (hipstub_launches() != before) { fprintf(stderr, "a refused call launched\n"); exit(2); }
}

int main() {
  walk(37, 23, 3, 0, 5, 1);               // an odd width: the padded copy of B
  walk(37, 200, 4, 0, 128, 2);            // four column steps
  walk(5, 700, 5, 0, 1, 3);
  walk(1100, 7, 2, 0, 10, 4);
  walk(9, 65, 256, 0, 64, 5);
  walk(37, 23, 3, 5, 5, 6);               // the tri-factorisation
  walk(11, 130, 256, 2, 7, 7);
  walk(11, 9, 2, 255, 3, 8);
  refusals();
  if (hipstub_live_allocs() != 0) { fprintf(stderr, "%ld allocations outlive the run\n", hipstub_live_allocs()); return 2; }
  printf("sanitize driver top: ok (%ld stub launches, %ld live stub allocations)\n", hipstub_launches(), hipstub_live_allocs());
  return 0;
}
