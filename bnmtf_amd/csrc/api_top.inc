// The n best predicted entries per row (C ABI part 11: bnmtf_amd.top_entries, bnmtf_amd/top_entries.py; DESIGN.md section 2.9) --
// included in api.hip beside api_predictive.inc, on which it does not depend.
// bnmtf_top_entries takes no handle: fp64 factors as the host holds them, the rows asked for and a list of excluded entries.
// Before its first device call it checks everything, gathers the selected rows of A and builds the exclusion list by selected row
// (a counting sort by row; columns sorted and deduplicated within a row; entries of rows not asked for are dropped).  Then it makes
// a stream, three events and its buffers on the device, uploads, and launches launch_top (kernel_top.hip): (F S) of the selected
// rows for the tri-factorisation, a wave per (row, column segment) pair, and the merge of a row's segments.  Everything is owned
// by objects of this function: whichever way it leaves, nothing stays.  Nothing of size I x J is made on either side.

namespace bnmtf {

constexpr int kTopMaxDim = 1 << 30;                  // I and J: column indices and their 64-column steps stay inside an int
constexpr long long kTopFillPairs = 256 * 8;         // split = 0: (row, segment) pairs that fill 256 CUs with eight waves each

static bool top_all_finite(const double* p, size_t count) {
  for (size_t t = 0; t < count; ++t)
    if (!std::isfinite(p[t])) return false;
  return true;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_top_entries(int device, int I, int J, int K, int L, const double* A, const double* S, const double* B,
                      uint64_t n_rows, const int32_t* rows, uint64_t n_excl, const int32_t* ex_rows, const int32_t* ex_cols,
                      int n, int largest, int split, int32_t* cols_out, double* scores_out, int32_t* counts_out) try {
  if (!A || !B || !cols_out || !scores_out || !counts_out || (n_excl > 0 && (!ex_rows || !ex_cols))) {
    set_error("bnmtf_top_entries: null argument");
    return BNMTF_EINVAL;
  }
  if (I < 1 || J < 1 || I > kTopMaxDim || J > kTopMaxDim || K < 1 || K > kObsMaxRank || L < 0 || L > kObsMaxRank) {
    set_error("bnmtf_top_entries: unsupported shape I=%d J=%d K=%d L=%d (1 <= I, J <= 2^30, 1 <= K <= %d, 0 <= L <= %d)", I, J, K, L, kObsMaxRank, kObsMaxRank);
    return BNMTF_EINVAL;
  }
  if ((L > 0) != (S != nullptr)) { set_error("bnmtf_top_entries: S is required when L >= 1 and null when L = 0 (L=%d)", L); return BNMTF_EINVAL; }
  if (n < 1 || n > kTopMaxN) { set_error("bnmtf_top_entries: 1 <= n <= %d (BNMTF_TOP_MAX_N; n=%d)", kTopMaxN, n); return BNMTF_EINVAL; }
  if (largest != 0 && largest != 1) { set_error("bnmtf_top_entries: largest is 0 or 1 (largest=%d)", largest); return BNMTF_EINVAL; }
  if (split < 0 || split > kTopMaxSplit) { set_error("bnmtf_top_entries: 0 <= split <= %d (0: the library chooses; split=%d)", kTopMaxSplit, split); return BNMTF_EINVAL; }
  if (rows && (n_rows < 1 || n_rows > (uint64_t)I)) {
    set_error("bnmtf_top_entries: 1 <= n_rows <= I distinct rows (n_rows=%llu, I=%d)", (unsigned long long)n_rows, I);
    return BNMTF_EINVAL;
  }
  if (n_excl >= ((uint64_t)1 << 32)) { set_error("bnmtf_top_entries: n_excl < 2^32 excluded entries (n_excl=%llu)", (unsigned long long)n_excl); return BNMTF_EINVAL; }
  const int r = rows ? (int)n_rows : I;
  const int W = L > 0 ? L : K;

  // ---- the rows asked for: where each row of the matrix stands among them (-1: not asked for)
  std::vector<int32_t> slot_of;
  if (rows) {
    slot_of.assign((size_t)I, -1);
    for (int q = 0; q < r; ++q) {
      if (rows[q] < 0 || rows[q] >= I) { set_error("bnmtf_top_entries: rows[%d] = %d lies outside the %d rows", q, rows[q], I); return BNMTF_EINVAL; }
      if (slot_of[rows[q]] >= 0) { set_error("bnmtf_top_entries: rows[%d] = %d occurs twice (rows[%d])", q, rows[q], slot_of[rows[q]]); return BNMTF_EINVAL; }
      slot_of[rows[q]] = q;
    }
  }
  for (uint64_t e = 0; e < n_excl; ++e)
    if (ex_rows[e] < 0 || ex_rows[e] >= I || ex_cols[e] < 0 || ex_cols[e] >= J) {
      set_error("bnmtf_top_entries: excluded entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, ex_rows[e], ex_cols[e], I, J);
      return BNMTF_EINVAL;
    }

  // ---- the selected rows of A, and finite values everywhere (the total order needs finite scores)
  std::vector<double> Asel;
  if (rows) {
    Asel.resize((size_t)r * K);
    for (int q = 0; q < r; ++q) memcpy(Asel.data() + (size_t)q * K, A + (size_t)rows[q] * K, (size_t)K * sizeof(double));
  }
  const double* const Ause = rows ? Asel.data() : A;
  if (!top_all_finite(Ause, (size_t)r * K) || (L > 0 && !top_all_finite(S, (size_t)K * L)) || !top_all_finite(B, (size_t)J * W)) {
    set_error("bnmtf_top_entries: a factor holds a value that is not finite (the order needs finite scores)");
    return BNMTF_EINVAL;
  }
  // B with an even row stride: a row begins on a 16-byte boundary
  const int stride = (W + 1) & ~1;
  std::vector<double> Bpad;
  if (stride != W) {
    Bpad.assign((size_t)J * stride, 0.0);
    for (int j = 0; j < J; ++j) memcpy(Bpad.data() + (size_t)j * stride, B + (size_t)j * W, (size_t)W * sizeof(double));
  }
  const double* const Buse = stride != W ? Bpad.data() : B;

  // ---- the exclusion list by selected row: counting sort, then ascending and distinct within a row
  std::vector<uint32_t> exptr((size_t)r + 1, 0u), excol;
  {
    std::vector<uint32_t> ptr((size_t)r + 1, 0u);
    for (uint64_t e = 0; e < n_excl; ++e) {
      const int32_t q = rows ? slot_of[ex_rows[e]] : ex_rows[e];
      if (q >= 0) ptr[(size_t)q + 1]++;
    }
    for (int q = 0; q < r; ++q) ptr[(size_t)q + 1] += ptr[q];
    std::vector<uint32_t> col(ptr[r]), at(ptr.begin(), ptr.end() - 1);
    for (uint64_t e = 0; e < n_excl; ++e) {
      const int32_t q = rows ? slot_of[ex_rows[e]] : ex_rows[e];
      if (q >= 0) col[at[q]++] = (uint32_t)ex_cols[e];
    }
    excol.reserve(col.size());
    for (int q = 0; q < r; ++q) {
      std::sort(col.begin() + ptr[q], col.begin() + ptr[(size_t)q + 1]);
      for (uint32_t t = ptr[q]; t < ptr[(size_t)q + 1]; ++t)
        if (t == ptr[q] || col[t] != col[t - 1]) excol.push_back(col[t]);
      exptr[(size_t)q + 1] = (uint32_t)excol.size();
    }
  }

  // ---- the column split: whole 64-column steps per segment
  const int steps = (J + kTopStep - 1) / kTopStep;
  int use_split = split;
  if (use_split == 0) {
    const long long want = (kTopFillPairs + r - 1) / r;
    use_split = (int)(want < 1 ? 1 : want > steps ? steps : want);
    if (use_split > kTopMaxSplit) use_split = kTopMaxSplit;
  }
  const int seg_steps = (steps + use_split - 1) / use_split;
  const long long pairs = (long long)r * use_split;
  if ((pairs + kTopRows - 1) / kTopRows > 0x7fffffffLL) {
    set_error("bnmtf_top_entries: %d rows in %d segments are more (row, segment) pairs than one launch takes", r, use_split);
    return BNMTF_EINVAL;
  }

  // ---- the device's side: all of it owned here
  CallScope cs;
  DevBuf<double> dA, dS, dFS, dB, d_key, d_scores;
  DevBuf<uint32_t> d_exptr, d_excol;
  DevBuf<int32_t> d_pcol, d_pcnt, d_cols, d_counts;
  CHK(cs.open(device));
  const size_t nA = (size_t)r * K, nB = (size_t)J * stride, nout = (size_t)r * n, npart = (size_t)pairs * n;
  CHK(dA.alloc(nA)); CHK(dB.alloc(nB));
  if (L > 0) { CHK(dS.alloc((size_t)K * L)); CHK(dFS.alloc((size_t)r * L)); }
  CHK(d_exptr.alloc(exptr.size())); CHK(d_excol.alloc(excol.size() ? excol.size() : 1));
  CHK(d_key.alloc(npart)); CHK(d_pcol.alloc(npart)); CHK(d_pcnt.alloc((size_t)pairs));
  CHK(d_cols.alloc(nout)); CHK(d_scores.alloc(nout)); CHK(d_counts.alloc((size_t)r));

  CHK(cs.mark(0));
  HIPCHK(hipMemcpyAsync(dA.p, Ause, nA * sizeof(double), hipMemcpyHostToDevice, cs.s));
  if (L > 0) HIPCHK(hipMemcpyAsync(dS.p, S, (size_t)K * L * sizeof(double), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(dB.p, Buse, nB * sizeof(double), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_exptr.p, exptr.data(), exptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  if (!excol.empty()) HIPCHK(hipMemcpyAsync(d_excol.p, excol.data(), excol.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  CHK(cs.mark(1));

  TopArgs a; memset(&a, 0, sizeof(a));
  a.A = dA.p; a.S = L > 0 ? dS.p : nullptr; a.FS = L > 0 ? dFS.p : nullptr; a.B = dB.p;
  a.r = r; a.J = J; a.K = K; a.L = L; a.stride = stride;
  a.exptr = d_exptr.p; a.excol = d_excol.p;
  a.n = n; a.largest = largest; a.split = use_split; a.seg_steps = seg_steps;
  a.part_key = d_key.p; a.part_col = d_pcol.p; a.part_cnt = d_pcnt.p;
  a.cols = d_cols.p; a.scores = d_scores.p; a.counts = d_counts.p;
  launch_top(a, cs.s);
  HIPCHK(hipGetLastError());
  CHK(cs.mark(2));
  HIPCHK(hipStreamSynchronize(cs.s));
  HIPCHK(hipGetLastError());
  double up = 0.0, kn = 0.0;
  CHK(cs.elapsed(&up, &kn));

  HIPCHK(hipMemcpy(cols_out, d_cols.p, nout * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(scores_out, d_scores.p, nout * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(counts_out, d_counts.p, (size_t)r * sizeof(int32_t), hipMemcpyDeviceToHost));
  g_call_ms[kCallTop][0] = up; g_call_ms[kCallTop][1] = kn;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_top_entries_times(double* upload_ms, double* kernel_ms) try {
  return call_times("bnmtf_top_entries_times", kCallTop, upload_ms, kernel_ms);
} BNMTF_ABI_GUARD

}  // extern "C"
