// Closed-form predictive mean and variance of a variational model (C ABI part 13: bnmtf_amd.variational_predictive,
// bnmtf_amd/predictive_q.py; DESIGN.md section 2.8a) -- included in api.hip beside api_top.inc and api_foldin.inc, on which it does
// not depend.
// bnmtf_predictive_moments takes no handle: the entry list and the host's fp64 means and variances of q.  It checks everything and
// sorts the list by row (a stable counting sort; the permutation scatters the outputs back) before its first device call, makes a
// stream, three events, the two list arrays, the operands, the table H [J][K] of the tri-factorisation and the two outputs [n] on
// the device, uploads once and launches once (kernel_predictive_q.hip).  Everything is owned by objects of this function: whichever
// way it leaves, nothing stays.  Nothing of size I x J is made on either side.

namespace bnmtf {

// what is wrong with a factor's moments: 0 nothing, 1 a mean that is not finite, 2 a variance that is negative or not finite
static int predictive_q_bad(const double* mean, const double* var, size_t count) {
  for (size_t q = 0; q < count; ++q) if (!std::isfinite(mean[q])) return 1;
  if (var) for (size_t q = 0; q < count; ++q) if (!(var[q] >= 0.0) || !std::isfinite(var[q])) return 2;
  return 0;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_predictive_moments(int device, int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols,
                             const double* EA, const double* VA, const double* ES, const double* VS, const double* EB, const double* VB,
                             double* mean_out, double* var_out) try {
  if (!rows || !cols || !EA || !EB || !mean_out || !var_out) { set_error("bnmtf_predictive_moments: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > kObsMaxRank || L < 0 || L > kObsMaxRank) {
    set_error("bnmtf_predictive_moments: unsupported shape I=%d J=%d K=%d L=%d (1 <= K <= %d, 0 <= L <= %d)", I, J, K, L, kObsMaxRank, kObsMaxRank);
    return BNMTF_EINVAL;
  }
  if ((L > 0) != (ES != nullptr) || (L == 0 && VS)) {
    set_error("bnmtf_predictive_moments: ES is required when L >= 1, ES and VS are null when L = 0 (L=%d)", L);
    return BNMTF_EINVAL;
  }
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("bnmtf_predictive_moments: 1 <= n < 2^31 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= I || cols[e] < 0 || cols[e] >= J) {
      set_error("bnmtf_predictive_moments: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], I, J);
      return BNMTF_EINVAL;
    }
  const int W = L > 0 ? L : K;
  const size_t nA = (size_t)I * K, nS = (size_t)K * L, nB = (size_t)J * W;
  {
    const char* const names[3] = {"rows", "middle", "columns"};
    const double* const means[3] = {EA, ES, EB};
    const double* const vars[3] = {VA, VS, VB};
    const size_t counts[3] = {nA, nS, nB};
    for (int m = 0; m < 3; ++m) {
      if (!means[m]) continue;
      const int bad = predictive_q_bad(means[m], vars[m], counts[m]);
      if (bad) {
        set_error(bad == 1 ? "bnmtf_predictive_moments: the %s factor holds a mean that is not finite"
                           : "bnmtf_predictive_moments: the %s factor holds a variance that is negative or not finite", names[m]);
        return BNMTF_EINVAL;
      }
    }
  }

  // ---- the list by row, in the given order within a row
  std::vector<uint32_t> rowptr, col, perm;
  sort_entries_by_row(I, n, rows, cols, rowptr, col, perm);

  // ---- the device's side: all of it owned here
  CallScope cs;
  DevBuf<uint32_t> d_rowptr, d_col;
  DevBuf<double> dEA, dVA, dES, dVS, dEB, dVB, dH, d_mean, d_var;
  const int hstride = (K + 1) & ~1;
  CHK(cs.open(device));
  CHK(d_rowptr.alloc(rowptr.size())); CHK(d_col.alloc(n));
  CHK(dEA.alloc(nA)); CHK(dEB.alloc(nB));
  if (VA) CHK(dVA.alloc(nA));
  if (VB) CHK(dVB.alloc(nB));
  if (L > 0) { CHK(dES.alloc(nS)); CHK(dH.alloc((size_t)J * hstride)); }
  if (VS) CHK(dVS.alloc(nS));
  CHK(d_mean.alloc(n)); CHK(d_var.alloc(n));

  CHK(cs.mark(0));
  HIPCHK(hipMemcpyAsync(d_rowptr.p, rowptr.data(), rowptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_col.p, col.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(dEA.p, EA, nA * sizeof(double), hipMemcpyHostToDevice, cs.s));
  if (VA) HIPCHK(hipMemcpyAsync(dVA.p, VA, nA * sizeof(double), hipMemcpyHostToDevice, cs.s));
  if (L > 0) HIPCHK(hipMemcpyAsync(dES.p, ES, nS * sizeof(double), hipMemcpyHostToDevice, cs.s));
  if (VS) HIPCHK(hipMemcpyAsync(dVS.p, VS, nS * sizeof(double), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(dEB.p, EB, nB * sizeof(double), hipMemcpyHostToDevice, cs.s));
  if (VB) HIPCHK(hipMemcpyAsync(dVB.p, VB, nB * sizeof(double), hipMemcpyHostToDevice, cs.s));
  CHK(cs.mark(1));

  PredictiveQArgs a; memset(&a, 0, sizeof(a));
  a.rowptr = d_rowptr.p; a.col = d_col.p;
  a.EA = dEA.p; a.VA = VA ? dVA.p : nullptr;
  a.ES = L > 0 ? dES.p : nullptr; a.VS = VS ? dVS.p : nullptr;
  a.EB = dEB.p; a.VB = VB ? dVB.p : nullptr;
  a.H = L > 0 ? dH.p : nullptr;
  a.I = I; a.J = J; a.K = K; a.L = L; a.hstride = hstride;
  a.mean = d_mean.p; a.var = d_var.p;
  launch_predictive_q(a, cs.s);
  HIPCHK(hipGetLastError());
  CHK(cs.mark(2));
  HIPCHK(hipStreamSynchronize(cs.s));
  HIPCHK(hipGetLastError());
  double up = 0.0, kn = 0.0;
  CHK(cs.elapsed(&up, &kn));

  // ---- back, from list order to the given order
  std::vector<double> sorted(n);
  double* const outs[2] = {mean_out, var_out};
  const double* const devs[2] = {d_mean.p, d_var.p};
  for (int m = 0; m < 2; ++m) {
    HIPCHK(hipMemcpy(sorted.data(), devs[m], (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t q = 0; q < n; ++q) outs[m][perm[q]] = sorted[q];
  }
  g_call_ms[kCallPredictiveQ][0] = up; g_call_ms[kCallPredictiveQ][1] = kn;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_predictive_moments_times(double* upload_ms, double* kernel_ms) try {
  return call_times("bnmtf_predictive_moments_times", kCallPredictiveQ, upload_ms, kernel_ms);
} BNMTF_ABI_GUARD

}  // extern "C"
