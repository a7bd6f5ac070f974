// Observed-entry layout of the two-factor Gibbs / ICM models (C ABI part 6, layout='observed') -- included at the end of api.hip.
// A handle of bnmtf_obs_create holds, in ObsState, the observed entries as a row list and a column list, both factors row major
// and transposed in fp32, the prior rates, the long form's residual scratch and the V half sweep's partial sums: memory
// proportional to the number of observed entries.  None of the samplers' layouts, no dense operand, no copy of R or M.  The
// iteration is two launches of obs_sweep_kernel and obs_finish_kernel (kernel_obs.hip) on the handle's stream; the samples leave
// through the SampleSink like bnmf_gibbs_run's, written into their slots by the sweeps themselves.  One GPU.
// The variational model on the same handle (bnmf_vbo_*, at the end of this file): its q parameters, the transposed S2 and the
// half sweeps' partial sums are allocated by the first bnmf_vbo_set_state, so a Gibbs / ICM handle holds none of them.

namespace bnmtf {

struct ObsList {                 // one direction: units, their entries' inner indices and values
  uint32_t* ptr = nullptr; uint32_t* idx = nullptr; float* val = nullptr;
  float* X = nullptr; float* XT = nullptr; int n = 0, ldT = 0;     // the direction's factor [n][KP] and [K][ldT]
  float* lambda = nullptr;                                         // [n][KP]
  double* numer = nullptr; double* taup = nullptr;                 // cond-params scratch [n]
  uint32_t longest = 0; size_t long_units = 0;                     // most entries of a unit; units beyond the register form
  // variational state (bnmf_vbo_set_state): q's mu, tau, var [n][KP] beside the expectation in X / XT; S2 = var + X^2 transposed
  // [K][ldT] with XT's zero word behind every column; the half sweep's partial sums [obs_sweep_blocks(n)][6]
  float* mu = nullptr; float* tauq = nullptr; float* var = nullptr; float* S2T = nullptr;
  double* vstat = nullptr;
};
struct ObsState {
  ObsList rows, cols;
  size_t n = 0; int KP = 0;
  float* escratch = nullptr;       // [n]
  double* part = nullptr;          // [obs_sweep_blocks(J)][4]
  double* scal = nullptr;          // tau_d, tau_f and out8 of the metric sums (one allocation)
  double* out8 = nullptr;
  bool force_long = false;
  bool vb_alloc = false, vb_state = false;   // the variational buffers exist; they hold the state of the last bnmf_vbo_set_state / run
  double* esd_part = nullptr;      // [obs_vb_esd_blocks(I)] exp_square_diff's partial sums
};

static void obs_free(bnmtf_model* h) {
  ObsState* s = h->obs;
  if (!s) return;
  for (ObsList* d : {&s->rows, &s->cols}) {
    dfree(d->ptr); dfree(d->idx); dfree(d->val); dfree(d->X); dfree(d->XT); dfree(d->lambda); dfree(d->numer); dfree(d->taup);
    dfree(d->mu); dfree(d->tauq); dfree(d->var); dfree(d->S2T); dfree(d->vstat);
  }
  dfree(s->escratch); dfree(s->part); dfree(s->scal); dfree(s->esd_part);
  h->tau_d = nullptr; h->tau_f = nullptr;
  delete s;
  h->obs = nullptr;
}

static int obs_check(bnmtf_model* h, bool need_state) {
  if (!h || !h->obs) { set_error("not a handle of bnmtf_obs_create"); return BNMTF_EINVAL; }
  if (need_state && !h->have_state) { set_error("bnmf_obs_set_state has not been called"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

// The entries sorted by (major, minor) with two stable counting sorts: ptr [nmajor + 1], the minor indices ascending within a
// unit, the values beside them.  Returns the position of an entry that occurs twice, or -1.
static long long obs_sort(uint64_t n, const int32_t* major, const int32_t* minor, const float* values, int nmajor, int nminor,
                          std::vector<uint32_t>& ptr, std::vector<uint32_t>& idx, std::vector<float>& val) {
  std::vector<uint32_t> by_minor(n), cnt((size_t)nminor + 1, 0);
  for (uint64_t e = 0; e < n; ++e) cnt[(size_t)minor[e] + 1]++;
  for (int m = 0; m < nminor; ++m) cnt[m + 1] += cnt[m];
  for (uint64_t e = 0; e < n; ++e) by_minor[cnt[minor[e]]++] = (uint32_t)e;
  ptr.assign((size_t)nmajor + 1, 0);
  for (uint64_t e = 0; e < n; ++e) ptr[(size_t)major[e] + 1]++;
  for (int u = 0; u < nmajor; ++u) ptr[u + 1] += ptr[u];
  std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
  idx.resize(n); val.resize(n);
  for (uint64_t q = 0; q < n; ++q) {
    const uint32_t e = by_minor[q];
    const uint32_t pos = at[major[e]]++;
    idx[pos] = (uint32_t)minor[e]; val[pos] = values[e];
  }
  for (int u = 0; u < nmajor; ++u)
    for (uint32_t p = ptr[u] + 1; p < ptr[u + 1]; ++p)
      if (idx[p] == idx[p - 1]) return (long long)p;
  return -1;
}

// What bnmtf_obs_create holds of the entries, built on the host before any device call (and handed out by
// bnmtf_obs_build_lists): the checked entries as a row list and a column list, and the sums of R over them.  Refuses an entry
// outside the matrix, an entry that occurs twice and a row or column without entries.
struct ObsLists {
  std::vector<uint32_t> rptr, ridx, cptr, cidx;
  std::vector<float> rval, cval;
  double sumR = 0, sumR2 = 0;
};
static int obs_lists(int I, int J, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values, ObsLists& ls) {
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("between 1 and 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e) {
    if (rows[e] < 0 || rows[e] >= I || cols[e] < 0 || cols[e] >= J) {
      set_error("entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], I, J);
      return BNMTF_EINVAL;
    }
    const double r = values[e]; ls.sumR += r; ls.sumR2 += r * r;
  }
  const long long dup = obs_sort(n, rows, cols, values, I, J, ls.rptr, ls.ridx, ls.rval);
  if (dup >= 0) {
    const int i = (int)(std::upper_bound(ls.rptr.begin(), ls.rptr.end(), (uint32_t)dup) - ls.rptr.begin()) - 1;
    set_error("the entry (%d, %u) occurs twice", i, ls.ridx[(size_t)dup]);
    return BNMTF_EINVAL;
  }
  (void)obs_sort(n, cols, rows, values, J, I, ls.cptr, ls.cidx, ls.cval);
  for (int i = 0; i < I; ++i) if (ls.rptr[i + 1] == ls.rptr[i]) { set_error("Fully unobserved row in R, row %d.", i); return BNMTF_EINVAL; }
  for (int j = 0; j < J; ++j) if (ls.cptr[j + 1] == ls.cptr[j]) { set_error("Fully unobserved column in R, column %d.", j); return BNMTF_EINVAL; }
  return BNMTF_OK;
}

static int obs_build_dir(bnmtf_model* h, ObsList& d, int n, const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& idx,
                         const std::vector<float>& val, const double* lambda) {
  ObsState* s = h->obs;
  const int K = h->K, KP = s->KP;
  d.n = n; d.ldT = round_up(n + 1, 64);          // (a zero behind every column of XT: the sweep's empty slots gather it)
  CHK(upload(&d.ptr, ptr, h->stream));
  CHK(upload(&d.idx, idx, h->stream));
  CHK(upload(&d.val, val, h->stream));
  std::vector<float> lam((size_t)n * KP, 0.f);
  for (int u = 0; u < n; ++u)
    for (int k = 0; k < K; ++k) lam[(size_t)u * KP + k] = (float)lambda[(size_t)u * K + k];
  CHK(upload(&d.lambda, lam, h->stream));
  CHK(dalloc(&d.X, (size_t)n * KP));
  CHK(dalloc(&d.XT, (size_t)K * d.ldT));
  CHK(dalloc(&d.numer, (size_t)n, false));
  CHK(dalloc(&d.taup, (size_t)n, false));
  for (int u = 0; u < n; ++u) {
    const uint32_t c = ptr[u + 1] - ptr[u];
    d.longest = std::max(d.longest, c);
    if (c > (uint32_t)kObsMaxSlots * 64u) d.long_units++;
  }
  return BNMTF_OK;
}

// fp64 host [n][K] -> fp32 device [n][KP] and [K][ldT]
static int obs_put(bnmtf_model* h, ObsList& d, const double* src) {
  const int K = h->K, KP = h->obs->KP;
  std::vector<float> x((size_t)d.n * KP, 0.f), xt((size_t)K * d.ldT, 0.f);
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < K; ++k) {
      const float v = (float)src[(size_t)u * K + k];
      x[(size_t)u * KP + k] = v; xt[(size_t)k * d.ldT + u] = v;
    }
  HIPCHK(hipMemcpyAsync(d.X, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.XT, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

static ObsSweepArgs obs_sweep_args(bnmtf_model* h, bool rows, int mode) {
  ObsState* s = h->obs;
  ObsList& d = rows ? s->rows : s->cols;
  ObsList& o = rows ? s->cols : s->rows;
  ObsSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = o.n; a.K = h->K; a.KP = s->KP;
  a.mode = mode; a.cond_k = -1; a.force_long = s->force_long ? 1 : 0; a.min_x = h->cur_min_x;
  a.lambda = d.lambda;
  a.X = d.X; a.XT = d.XT; a.ldT = d.ldT;
  a.Xo = o.X; a.XoT = o.XT; a.ldT_o = o.ldT;
  a.escratch = s->escratch;
  a.tau = h->tau_f;
  a.key0 = (uint32_t)h->seed; a.key1 = (uint32_t)(h->seed >> 32); a.it = (uint32_t)h->iteration;
  a.stream = rows ? kStreamRows : kStreamCols;
  return a;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_obs_create(int I, int J, int K, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                     const double* lambda_rows, const double* lambda_cols, double alpha, double beta, uint64_t seed, int device,
                     bnmtf_handle* out) try {
  if (!out) { set_error("bnmtf_obs_create: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!rows || !cols || !values || !lambda_rows || !lambda_cols) { set_error("bnmtf_obs_create: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > BNMTF_OBS_MAX_RANK) {
    set_error("bnmtf_obs_create: unsupported shape I=%d J=%d K=%d (1 <= K <= %d)", I, J, K, BNMTF_OBS_MAX_RANK);
    return BNMTF_EINVAL;
  }
  ObsLists ls;
  CHK(obs_lists(I, J, n, rows, cols, values, ls));
  HIPCHK(hipSetDevice(device));
  bnmtf_model* h = new bnmtf_model();
  h->I = I; h->J = J; h->K = K; h->L = 0; h->device = device;
  h->alpha = alpha; h->beta = beta; h->seed = seed;
  h->n_obs = (double)n; h->sumR = ls.sumR; h->sumR2 = ls.sumR2;
  h->rows.nglob = I; h->rows.m = J; h->rows.W = K; h->cols.nglob = J; h->cols.m = I; h->cols.W = K;
  h->std_built = false;
  struct Guard { bnmtf_model* h; ~Guard() { if (h) bnmtf_destroy(h); } } guard{h};      // every way out but the last, an exception included, destroys the handle
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; set_error("hipStreamCreate failed"); return BNMTF_EHIP; }
  h->obs = new ObsState();
  ObsState* s = h->obs;
  s->n = (size_t)n; s->KP = round_up(K, 4);
  const char* fl = getenv("BNMTF_OBS_LONG");
  s->force_long = fl && fl[0] == '1';
  int rcode;
  if ((rcode = obs_build_dir(h, s->rows, I, ls.rptr, ls.ridx, ls.rval, lambda_rows)) || (rcode = obs_build_dir(h, s->cols, J, ls.cptr, ls.cidx, ls.cval, lambda_cols)) ||
      (rcode = dalloc(&s->escratch, (size_t)n, false)) || (rcode = dalloc(&s->part, (size_t)obs_sweep_blocks(J) * 4, false)) ||
      (rcode = dalloc(&s->scal, 16)))
    return rcode;
  h->tau_d = s->scal; h->tau_f = reinterpret_cast<float*>(s->scal + 1); s->out8 = s->scal + 8;
  char buf[512];
  snprintf(buf, sizeof(buf), "bnmf layout=observed I=%d J=%d K=%d entries=%llu (%.3g %% of the matrix) longest_row=%u longest_column=%u "
           "long_form_units=%zu/%zu force_long=%d", I, J, K, (unsigned long long)n, 100.0 * (double)n / ((double)I * (double)J),
           s->rows.longest, s->cols.longest, s->rows.long_units, s->cols.long_units, (int)s->force_long);
  h->description = buf;
  guard.h = nullptr;
  *out = h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_obs_build_lists(int I, int J, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                          uint32_t* row_ptr, uint32_t* row_col, float* row_val, uint32_t* col_ptr, uint32_t* col_row, float* col_val) try {
  if (!rows || !cols || !values) { set_error("bnmtf_obs_build_lists: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1) { set_error("bnmtf_obs_build_lists: unsupported shape I=%d J=%d", I, J); return BNMTF_EINVAL; }
  ObsLists ls;
  CHK(obs_lists(I, J, n, rows, cols, values, ls));
  if (row_ptr) memcpy(row_ptr, ls.rptr.data(), ls.rptr.size() * sizeof(uint32_t));
  if (row_col) memcpy(row_col, ls.ridx.data(), ls.ridx.size() * sizeof(uint32_t));
  if (row_val) memcpy(row_val, ls.rval.data(), ls.rval.size() * sizeof(float));
  if (col_ptr) memcpy(col_ptr, ls.cptr.data(), ls.cptr.size() * sizeof(uint32_t));
  if (col_row) memcpy(col_row, ls.cidx.data(), ls.cidx.size() * sizeof(uint32_t));
  if (col_val) memcpy(col_val, ls.cval.data(), ls.cval.size() * sizeof(float));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_set_state(bnmtf_handle h, const double* U, const double* V, double tau) try {
  CHK(obs_check(h, false));
  if (!U || !V) { set_error("bnmf_obs_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(obs_put(h, h->obs->rows, U));
  CHK(obs_put(h, h->obs->cols, V));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->obs->vb_state = false;          // (the expectations were replaced: a variational state ends here)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_get_state(bnmtf_handle h, double* U, double* V, double* tau) try {
  CHK(obs_check(h, true));
  ObsState* s = h->obs;
  if (U) CHK(download_matrix(h, s->rows.X, h->I, h->K, s->KP, U));
  if (V) CHK(download_matrix(h, s->cols.X, h->J, h->K, s->KP, V));
  if (tau) {
    HIPCHK(hipMemcpyAsync(tau, h->tau_d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_run(bnmtf_handle h, int n_iter, int update, float* U_out, float* V_out, double* tau_out, double* perf_out,
                 double* times_out) try {
  CHK(obs_check(h, true));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsState* s = h->obs;
  CHK(ensure_rec(h, (size_t)n_iter));
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  if (mode == kSweepDraw) CHK(stage_gamma_variates(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  SampleSink sink;
  sink.add(s->rows.X, h->I, h->K, s->KP, U_out);
  sink.add(s->cols.X, h->J, h->K, s->KP, V_out);
  CHK(sink.begin(h, n_iter));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    ObsSweepArgs a = obs_sweep_args(h, true, mode);
    a.snap = sink.slot_for(it, s->rows.X);
    launch_obs_sweep(a, h->stream);
    a = obs_sweep_args(h, false, mode);
    a.snap = sink.slot_for(it, s->cols.X);
    a.part = s->part;
    launch_obs_sweep(a, h->stream);
    ObsFinishArgs f; memset(&f, 0, sizeof(f));
    f.part = s->part; f.nb = obs_sweep_blocks(h->J);
    f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
    f.update = update; f.gunit = mode == kSweepDraw ? h->gunit + it : nullptr;
    f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->rec + (size_t)it * 5;
    launch_obs_finish(f, h->stream);
    CHK(sink.close_slot(it));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sink.finish());
  HIPCHK(hipGetLastError());
  std::vector<double> rec((size_t)n_iter * 5);
  HIPCHK(hipMemcpy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int it = 0; it < n_iter; ++it) {
    if (tau_out) tau_out[it] = rec[(size_t)it * 5];
    if (perf_out) for (int m = 0; m < 3; ++m) perf_out[(size_t)it * 3 + m] = rec[(size_t)it * 5 + 1 + m];
  }
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_cond_params(bnmtf_handle h, int which, int k, double* numer_out, double* tau_out) try {
  CHK(obs_check(h, true));
  if (which != 0 && which != 1) { set_error("bnmf_obs_cond_params: which is 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  if (k < 0 || k >= h->K) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  if (!numer_out || !tau_out) { set_error("bnmf_obs_cond_params: null argument"); return BNMTF_EINVAL; }
  ObsList& d = which == 0 ? h->obs->rows : h->obs->cols;
  ObsSweepArgs a = obs_sweep_args(h, which == 0, kSweepDraw);
  a.cond_k = k; a.numer_out = d.numer; a.tau_out = d.taup;
  launch_obs_sweep(a, h->stream);
  HIPCHK(hipMemcpyAsync(numer_out, d.numer, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tau_out, d.taup, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                         const double* A, const double* B, double sums_out[6]) try {
  CHK(obs_check(h, false));
  if (!rows || !cols || !values || !A || !B || !sums_out) { set_error("bnmf_obs_metric_sums: null argument"); return BNMTF_EINVAL; }
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("bnmf_obs_metric_sums: between 1 and 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= h->I || cols[e] < 0 || cols[e] >= h->J) {
      set_error("bnmf_obs_metric_sums: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], h->I, h->J);
      return BNMTF_EINVAL;
    }
  DevBuf<uint32_t> dr, dc; DevBuf<float> dv; DevBuf<double> dA, dB, part;
  CHK(dr.alloc(n)); CHK(dc.alloc(n)); CHK(dv.alloc(n));
  CHK(dA.alloc((size_t)h->I * h->K)); CHK(dB.alloc((size_t)h->J * h->K)); CHK(part.alloc((size_t)obs_metric_blocks(n) * 8));
  HIPCHK(hipMemcpyAsync(dr.p, rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));      // (checked non-negative: the same bits as uint32)
  HIPCHK(hipMemcpyAsync(dc.p, cols, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dv.p, values, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dA.p, A, (size_t)h->I * h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dB.p, B, (size_t)h->J * h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ObsMetricArgs a; memset(&a, 0, sizeof(a));
  a.row = dr.p; a.col = dc.p; a.val = dv.p; a.n = (size_t)n; a.A = dA.p; a.B = dB.p; a.K = h->K; a.part = part.p;
  launch_obs_metric(a, h->obs->out8, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  double out8[8];
  HIPCHK(hipMemcpy(out8, h->obs->out8, sizeof(out8), hipMemcpyDeviceToHost));
  for (int m = 0; m < 6; ++m) sums_out[m] = out8[m];
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"

// ---- the variational two-factor model on the handle's lists (kernel_obs_vb.hip; DESIGN.md section 2.7) -----------------------
namespace bnmtf {

static int vbo_check(bnmtf_model* h, bool need_state) {
  if (!h || !h->obs) { set_error("not a handle of bnmtf_obs_create"); return BNMTF_EINVAL; }
  if (need_state && !(h->obs->vb_state && h->have_state)) { set_error("bnmf_vbo_set_state has not been called"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

static int vbo_alloc(bnmtf_model* h) {
  ObsState* s = h->obs;
  if (s->vb_alloc) return BNMTF_OK;
  for (ObsList* d : {&s->rows, &s->cols}) {
    if (!d->mu) CHK(dalloc(&d->mu, (size_t)d->n * s->KP));
    if (!d->tauq) CHK(dalloc(&d->tauq, (size_t)d->n * s->KP));
    if (!d->var) CHK(dalloc(&d->var, (size_t)d->n * s->KP));
    if (!d->S2T) CHK(dalloc(&d->S2T, (size_t)h->K * d->ldT));
    if (!d->vstat) CHK(dalloc(&d->vstat, (size_t)obs_sweep_blocks(d->n) * 6));
  }
  if (!s->esd_part) CHK(dalloc(&s->esd_part, (size_t)obs_vb_esd_blocks(h->I)));
  s->vb_alloc = true;
  return BNMTF_OK;
}

// fp64 host [n][K] x 4 -> the direction's fp32 q: mu, tau, var [n][KP]; the expectation in X / XT; S2 = var + exp^2 in S2T
static int vbo_put(bnmtf_model* h, ObsList& d, const double* mu, const double* tau, const double* ex, const double* var) {
  const int K = h->K, KP = h->obs->KP;
  const size_t nk = (size_t)d.n * KP;
  std::vector<float> m(nk, 0.f), t(nk, 0.f), v(nk, 0.f), s2((size_t)K * d.ldT, 0.f);
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < K; ++k) {
      const size_t src = (size_t)u * K + k, at = (size_t)u * KP + k;
      m[at] = (float)mu[src]; t[at] = (float)tau[src]; v[at] = (float)var[src];
      const float e = (float)ex[src];
      s2[(size_t)k * d.ldT + u] = fmaf(e, e, v[at]);              // (as the sweep forms it)
    }
  CHK(obs_put(h, d, ex));
  HIPCHK(hipMemcpyAsync(d.mu, m.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.tauq, t.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.var, v.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.S2T, s2.data(), s2.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

static ObsVbSweepArgs vbo_sweep_args(bnmtf_model* h, bool rows) {
  ObsState* s = h->obs;
  ObsList& d = rows ? s->rows : s->cols;
  ObsList& o = rows ? s->cols : s->rows;
  ObsVbSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = o.n; a.K = h->K; a.KP = s->KP;
  a.only_k = -1; a.moments = 1; a.force_long = s->force_long ? 1 : 0;
  a.lambda = d.lambda;
  a.X = d.X; a.XT = d.XT; a.S2T = d.S2T; a.ldT = d.ldT;
  a.mu = d.mu; a.tauq = d.tauq; a.var = d.var;
  a.Xo = o.X; a.XoT = o.XT; a.S2oT = o.S2T; a.ldT_o = o.ldT;
  a.escratch = s->escratch;
  a.tau = h->tau_f;
  return a;
}

}  // namespace bnmtf

extern "C" {

int bnmf_vbo_set_state(bnmtf_handle h, const double* muU, const double* tauU, const double* expU, const double* varU,
                       const double* muV, const double* tauV, const double* expV, const double* varV, double exptau) try {
  CHK(vbo_check(h, false));
  if (!muU || !tauU || !expU || !varU || !muV || !tauV || !expV || !varV) { set_error("bnmf_vbo_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(vbo_alloc(h));
  h->obs->vb_state = false;
  CHK(vbo_put(h, h->obs->rows, muU, tauU, expU, varU));
  CHK(vbo_put(h, h->obs->cols, muV, tauV, expV, varV));
  CHK(set_tau(h, exptau));
  h->have_state = true;
  h->obs->vb_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_get_state(bnmtf_handle h, double* muU, double* tauU, double* expU, double* varU,
                       double* muV, double* tauV, double* expV, double* varV) try {
  CHK(vbo_check(h, true));
  ObsState* s = h->obs;
  ObsList& r = s->rows; ObsList& c = s->cols;
  if (muU) CHK(download_matrix(h, r.mu, h->I, h->K, s->KP, muU));
  if (tauU) CHK(download_matrix(h, r.tauq, h->I, h->K, s->KP, tauU));
  if (expU) CHK(download_matrix(h, r.X, h->I, h->K, s->KP, expU));
  if (varU) CHK(download_matrix(h, r.var, h->I, h->K, s->KP, varU));
  if (muV) CHK(download_matrix(h, c.mu, h->J, h->K, s->KP, muV));
  if (tauV) CHK(download_matrix(h, c.tauq, h->J, h->K, s->KP, tauV));
  if (expV) CHK(download_matrix(h, c.X, h->J, h->K, s->KP, expV));
  if (varV) CHK(download_matrix(h, c.var, h->J, h->K, s->KP, varV));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_run(bnmtf_handle h, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out) try {
  CHK(vbo_check(h, true));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsState* s = h->obs;
  CHK(vb_reserve_rec(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    ObsVbSweepArgs a = vbo_sweep_args(h, true);
    a.stat = s->rows.vstat;
    launch_obs_vb_sweep(a, h->stream);
    a = vbo_sweep_args(h, false);
    a.stat = s->cols.vstat; a.part = s->part;
    launch_obs_vb_sweep(a, h->stream);
    ObsVbFinishArgs f; memset(&f, 0, sizeof(f));
    f.stat_r = s->rows.vstat; f.nb_r = obs_sweep_blocks(h->I);
    f.stat_c = s->cols.vstat; f.part = s->part; f.nb_c = obs_sweep_blocks(h->J);
    f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
    f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->vb_rec + (size_t)it * 16;
    launch_obs_vb_finish(f, h->stream);
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  std::vector<double> rec((size_t)n_iter * 16);
  HIPCHK(hipMemcpy(rec.data(), h->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_vb_rec(rec.data(), n_iter, exptau_out, perf_out, elbo_terms_out);
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_update(bnmtf_handle h, int which, int k, int moments) try {
  CHK(vbo_check(h, true));
  if (which != 0 && which != 1) { set_error("bnmf_vbo_update: which is 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  if (k < 0 || k >= h->K) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  ObsVbSweepArgs a = vbo_sweep_args(h, which == 0);
  a.only_k = k; a.moments = moments ? 1 : 0;
  launch_obs_vb_sweep(a, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_exp_square_diff(bnmtf_handle h, double* out) try {
  CHK(vbo_check(h, true));
  if (!out) { set_error("bnmf_vbo_exp_square_diff: null argument"); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  ObsVbEsdArgs a; memset(&a, 0, sizeof(a));
  a.ptr = s->rows.ptr; a.idx = s->rows.idx; a.val = s->rows.val; a.n = h->I; a.K = h->K; a.KP = s->KP;
  a.X = s->rows.X; a.var = s->rows.var; a.Xo = s->cols.X; a.varo = s->cols.var; a.part = s->esd_part;
  launch_obs_vb_esd(a, s->out8, h->stream);
  HIPCHK(hipMemcpyAsync(out, s->out8, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
