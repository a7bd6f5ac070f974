// Posterior predictive statistics of stored samples (C ABI part 10: bnmtf_amd.posterior_predictive, bnmtf_amd/predictive.py) --
// included behind api_many.inc at the end of api.hip.
// bnmtf_predictive_samples takes no handle: the entry list, the host's sample arrays and where in them the call's samples lie.  It
// checks everything and sorts the list by row (a stable counting sort; the permutation scatters the outputs back) before its first
// device call, makes a stream, three events, the two list arrays, one staging buffer per factor and the three accumulators [n] on
// the device, and walks the samples in chunks: upload of the chunk (one copy per factor when step = 1, else one per sample), one
// launch of predictive_kernel (kernel_predictive.hip), which read-modify-writes the accumulators.  Everything is owned by objects
// of this function: whichever way it leaves, nothing stays.  One stream: the upload of a chunk follows the kernel of the one
// before (DESIGN.md section 2.8 has the measured split that decided against a second stream).  The row sort, the chunk size and
// the upload of a chunk are api.hip's (sort_entries_by_row, sample_chunk, upload_samples): api_log_predictive.inc walks the same way.

extern "C" {

int bnmtf_predictive_samples(int device, int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols,
                             const float* A, const float* S, const float* B, uint64_t first, uint64_t step, int T, int chunk_samples,
                             double* p_first, double* sum_d, double* sum_d2) try {
  if (!rows || !cols || !A || !B || !p_first || !sum_d || !sum_d2) { set_error("bnmtf_predictive_samples: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > kObsMaxRank || L < 0 || L > kObsMaxRank) {
    set_error("bnmtf_predictive_samples: unsupported shape I=%d J=%d K=%d L=%d (1 <= K <= %d, 0 <= L <= %d)", I, J, K, L, kObsMaxRank, kObsMaxRank);
    return BNMTF_EINVAL;
  }
  if ((L > 0) != (S != nullptr)) { set_error("bnmtf_predictive_samples: S is required when L >= 1 and null when L = 0 (L=%d)", L); return BNMTF_EINVAL; }
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("bnmtf_predictive_samples: 1 <= n < 2^31 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  if (T < 1 || step < 1 || chunk_samples < 0) {
    set_error("bnmtf_predictive_samples: T >= 1, step >= 1, chunk_samples >= 0 (T=%d step=%llu chunk_samples=%d)", T, (unsigned long long)step, chunk_samples);
    return BNMTF_EINVAL;
  }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= I || cols[e] < 0 || cols[e] >= J) {
      set_error("bnmtf_predictive_samples: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], I, J);
      return BNMTF_EINVAL;
    }

  // ---- the list by row, in the given order within a row
  std::vector<uint32_t> rowptr, col, perm;
  sort_entries_by_row(I, n, rows, cols, rowptr, col, perm);

  const int W = L > 0 ? L : K;
  const size_t perA = (size_t)I * K, perS = (size_t)K * L, perB = (size_t)J * W;
  const int chunk = sample_chunk(chunk_samples, T, perA + perS + perB);

  // ---- the device's side: all of it owned here
  CallScope cs;
  DevBuf<uint32_t> d_rowptr, d_col;
  DevBuf<float> dA, dS, dB;
  DevBuf<double> d_first, d_sum, d_sum2;
  CHK(cs.open(device));
  CHK(d_rowptr.alloc(rowptr.size())); CHK(d_col.alloc(n));
  CHK(dA.alloc((size_t)chunk * perA)); CHK(dB.alloc((size_t)chunk * perB));
  if (L > 0) CHK(dS.alloc((size_t)chunk * perS));
  CHK(d_first.alloc(n, true)); CHK(d_sum.alloc(n, true)); CHK(d_sum2.alloc(n, true));
  HIPCHK(hipMemcpyAsync(d_rowptr.p, rowptr.data(), rowptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_col.p, col.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));

  PredictiveArgs a; memset(&a, 0, sizeof(a));
  a.rowptr = d_rowptr.p; a.col = d_col.p;
  a.A = dA.p; a.S = L > 0 ? dS.p : nullptr; a.B = dB.p;
  a.I = I; a.J = J; a.K = K; a.L = L;
  a.p_first = d_first.p; a.sum_d = d_sum.p; a.sum_d2 = d_sum2.p;
  double upload_ms = 0.0, kernel_ms = 0.0;
  for (int t0 = 0; t0 < T; t0 += chunk) {
    const int c = T - t0 < chunk ? T - t0 : chunk;
    CHK(cs.mark(0));
    CHK(upload_samples(dA.p, A, perA, first, step, t0, c, cs.s));
    if (L > 0) CHK(upload_samples(dS.p, S, perS, first, step, t0, c, cs.s));
    CHK(upload_samples(dB.p, B, perB, first, step, t0, c, cs.s));
    CHK(cs.mark(1));
    a.C = c; a.first = t0 == 0 ? 1 : 0;
    launch_predictive(a, cs.s);
    HIPCHK(hipGetLastError());
    CHK(cs.mark(2));
    HIPCHK(hipEventSynchronize(cs.ev[2]));         // (the staging buffers are the next chunk's; the stream orders that by itself)
    double up = 0.0, kn = 0.0;
    CHK(cs.elapsed(&up, &kn));
    upload_ms += up; kernel_ms += kn;
  }
  HIPCHK(hipStreamSynchronize(cs.s));
  HIPCHK(hipGetLastError());

  // ---- back, from list order to the given order
  std::vector<double> sorted(n);
  double* const outs[3] = {p_first, sum_d, sum_d2};
  const double* const devs[3] = {d_first.p, d_sum.p, d_sum2.p};
  for (int m = 0; m < 3; ++m) {
    HIPCHK(hipMemcpy(sorted.data(), devs[m], (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t q = 0; q < n; ++q) outs[m][perm[q]] = sorted[q];
  }
  g_call_ms[kCallPredictive][0] = upload_ms; g_call_ms[kCallPredictive][1] = kernel_ms;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_predictive_times(double* upload_ms, double* kernel_ms) try {
  return call_times("bnmtf_predictive_times", kCallPredictive, upload_ms, kernel_ms);
} BNMTF_ABI_GUARD

}  // extern "C"
