// The non-probabilistic models on the observed-entry layout (C ABI part 9: nmf_np.NMF / nmtf_np.NMTF with layout='observed') --
// included behind api_obs_trivb.inc at the end of api.hip.
// A handle of bnmtf_onp_create holds the ObsState of api_obs.inc with its marker set: the two lists, U and V (or F and G) row major
// and transposed in fp32 at strides of K (and L) rounded up to 4, P's scratch and, for NMTF (L > 0), S, the S step's output and
// block partials and the two effective factors G S^T [J][K] and F S [I][L] in both forms.  No prior rates, no seed, no tau, nothing
// of size I x J.  obs_free owns all of it.  The iteration (DESIGN.md section 2.7): NMF is two launches of onp_sweep_kernel and the
// fold; NMTF is the S step -- K L + 1 dependent passes of onp_s_pass_kernel --, then the F sweep against G S^T and the G sweep
// against F S (kernel_obs_np.hip).  One GPU, the handle's stream.

namespace bnmtf {

static int onp_check(bnmtf_model* h, bool need_state) {
  if (!h || !h->obs || !h->obs->np) { set_error("not a handle of bnmtf_onp_create"); return BNMTF_EINVAL; }
  if (need_state && !h->have_state) { set_error("bnmtf_onp_set_state has not been called"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

// NMTF's effective factor of a half sweep for the current state: rows (the F sweep): G S^T; else (the G sweep): F S
static void onp_enqueue_eff(bnmtf_model* h, bool rows) {
  ObsState* s = h->obs;
  OnpEffArgs e; memset(&e, 0, sizeof(e));
  e.S = s->npS; e.K = h->K; e.L = h->L;
  if (rows) { e.X = s->cols.X; e.n = h->J; e.ldX = s->cols.stride; e.transposeS = 1; e.out = s->ceffX; e.ldo = s->rows.stride; e.outT = s->ceffXT; e.ldT = s->cols.ldT; }
  else      { e.X = s->rows.X; e.n = h->I; e.ldX = s->rows.stride; e.transposeS = 0; e.out = s->reffX; e.ldo = s->cols.stride; e.outT = s->reffXT; e.ldT = s->rows.ldT; }
  launch_onp_eff(e, h->stream);
}

// the half sweep of a direction (rows: U or F) over the columns [k0, k1); NMTF: against the effective factor, rebuilt first.
// resume / keep: the single-column calls' hand-over of P (ObsState::np_next_*).
static void onp_enqueue_sweep(bnmtf_model* h, bool rows, int k0, int k1, bool resume, bool keep, double* rec) {
  ObsState* s = h->obs;
  ObsList& d = rows ? s->rows : s->cols;
  ObsOther o = obs_other(h, rows);
  if (h->L > 0) {
    onp_enqueue_eff(h, rows);
    o = rows ? ObsOther{s->ceffX, s->ceffXT, nullptr, s->cols.ldT, h->J} : ObsOther{s->reffX, s->reffXT, nullptr, s->rows.ldT, h->I};
  }
  OnpSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = o.m; a.K = d.W; a.KP = d.stride;
  a.k0 = k0; a.k1 = k1; a.force_long = s->force_long ? 1 : 0; a.resume = resume ? 1 : 0; a.keep = keep ? 1 : 0;
  a.X = d.X; a.XT = d.XT; a.ldT = d.ldT;
  a.Xo = o.X; a.XoT = o.XT; a.ldT_o = o.ldT;
  a.escratch = s->escratch;
  a.part = rec ? s->np_part : nullptr;
  launch_onp_sweep(a, h->stream);
  if (rec) launch_onp_fold(s->np_part, obs_sweep_blocks(d.n), rec, h->stream);
}

// S entries [e0, e1) in row-major order (nmtf_np.py:127-129 for the whole range): one pass per entry and one that finishes the
// last; npS2 receives the new values and becomes npS.  resume: escratch holds the P entry e0 continues from (no build);
// keep: the finishing pass moves P by the last entry's change too, for the call that continues.
static int onp_s_step(bnmtf_model* h, int e0, int e1, bool resume, bool keep) {
  ObsState* s = h->obs;
  const int nb = onp_s_blocks(h->I);
  if (!resume) onp_enqueue_eff(h, true);
  HIPCHK(hipMemcpyAsync(s->npS2, s->npS, (size_t)h->K * h->L * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  OnpSPassArgs a; memset(&a, 0, sizeof(a));
  a.ptr = s->rows.ptr; a.idx = s->rows.idx; a.val = s->rows.val; a.I = h->I;
  a.F = s->rows.X; a.ldF = s->rows.stride; a.GT = s->cols.XT; a.ldGT = s->cols.ldT; a.Xo = s->ceffX;
  a.P = s->escratch; a.S_in = s->npS; a.S_out = s->npS2; a.K = h->K; a.L = h->L; a.nb = nb;
  for (int e = e0; e <= e1; ++e) {
    a.prev = e > e0 ? e - 1 : -1;
    a.cur = e < e1 ? e : -1;
    a.build = (e == e0 && !resume) ? 1 : 0;
    a.apply = (e == e1 && keep) ? 1 : 0;
    a.part_prev = s->np_spart + (size_t)((e + 1) & 1) * nb * 2;
    a.part_cur = s->np_spart + (size_t)(e & 1) * nb * 2;
    launch_onp_s_pass(a, h->stream);
  }
  std::swap(s->npS, s->npS2);
  return BNMTF_OK;
}

static int onp_iteration(bnmtf_model* h, double* rec) {
  if (h->L == 0) {                                              // nmf_np.py:95-98
    onp_enqueue_sweep(h, true, 0, h->K, false, false, nullptr);
    onp_enqueue_sweep(h, false, 0, h->K, false, false, rec);
  } else {                                                      // nmtf_np.py:127-135
    CHK(onp_s_step(h, 0, h->K * h->L, false, false));
    onp_enqueue_sweep(h, true, 0, h->K, false, false, nullptr);
    onp_enqueue_sweep(h, false, 0, h->L, false, false, rec);
  }
  h->iteration++;
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_onp_create(int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                     int device, bnmtf_handle* out) try {
  if (!out) { set_error("bnmtf_onp_create: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!rows || !cols || !values) { set_error("bnmtf_onp_create: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > BNMTF_ONP_MAX_RANK || L < 0 || L > BNMTF_ONP_MAX_RANK) {
    set_error("bnmtf_onp_create: unsupported shape I=%d J=%d K=%d L=%d (1 <= K <= %d; L = 0: two factors, or 1 <= L <= %d)", I, J, K, L,
              BNMTF_ONP_MAX_RANK, BNMTF_ONP_MAX_RANK);
    return BNMTF_EINVAL;
  }
  const int sK = round_up(K, 4), sL = L > 0 ? round_up(L, 4) : sK;
  ObsCreateGuard guard;
  CHK(obs_create_common(guard, I, J, K, L, sK, n, rows, cols, values, nullptr, nullptr, 0.0, 0.0, 0, device, true, sL));
  bnmtf_model* h = guard.h;
  ObsState* s = h->obs;
  CHK(dalloc(&s->np_part, (size_t)obs_sweep_blocks(J) * 8, false));
  CHK(dalloc(&s->np_mpart, (size_t)1024 * 8, false));
  if (L > 0) {
    CHK(dalloc(&s->npS, (size_t)K * L)); CHK(dalloc(&s->npS2, (size_t)K * L));
    CHK(dalloc(&s->np_spart, (size_t)2 * onp_s_blocks(I) * 2));
    CHK(dalloc(&s->ceffX, (size_t)J * sK)); CHK(dalloc(&s->ceffXT, (size_t)K * s->cols.ldT));
    CHK(dalloc(&s->reffX, (size_t)I * sL)); CHK(dalloc(&s->reffXT, (size_t)L * s->rows.ldT));
  }
  char buf[512];
  snprintf(buf, sizeof(buf), "%s layout=observed I=%d J=%d K=%d L=%d entries=%llu (%.3g %% of the matrix) longest_row=%u longest_column=%u "
           "long_form_units=%zu/%zu force_long=%d", L > 0 ? "nmtf_np" : "nmf_np", I, J, K, L, (unsigned long long)n,
           100.0 * (double)n / ((double)I * (double)J), s->rows.longest, s->cols.longest, s->rows.long_units, s->cols.long_units, (int)s->force_long);
  h->description = buf;
  *out = guard.release();
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_onp_set_state(bnmtf_handle h, const double* A, const double* S, const double* B) try {
  CHK(onp_check(h, false));
  if (!A || !B || ((h->L > 0) != (S != nullptr))) { set_error("bnmtf_onp_set_state: null argument (S: given for NMTF, null for NMF)"); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  s->np_next_which = -1;
  CHK(obs_put(h, s->rows, A));
  CHK(obs_put(h, s->cols, B));
  if (S) {
    std::vector<float> sf((size_t)h->K * h->L);
    for (size_t t = 0; t < sf.size(); ++t) sf[t] = (float)S[t];
    HIPCHK(hipMemcpyAsync(s->npS, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  h->have_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_onp_get_state(bnmtf_handle h, double* A, double* S, double* B) try {
  CHK(onp_check(h, true));
  ObsState* s = h->obs;
  if (A) CHK(download_matrix(h, s->rows.X, h->I, s->rows.W, s->rows.stride, A));
  if (B) CHK(download_matrix(h, s->cols.X, h->J, s->cols.W, s->cols.stride, B));
  if (S) {
    if (h->L == 0) { set_error("bnmtf_onp_get_state: an NMF handle has no S"); return BNMTF_EINVAL; }
    CHK(download_matrix(h, s->npS, h->K, h->L, h->L, S));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_onp_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out) try {
  CHK(onp_check(h, true));
  if (n_iter < 0) { set_error("run: negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsState* s = h->obs;
  s->np_next_which = -1;
  if ((size_t)n_iter > s->np_rec_cap) {
    dfree(s->np_rec); s->np_rec_cap = 0;
    CHK(dalloc(&s->np_rec, (size_t)n_iter * 8, false));
    s->np_rec_cap = (size_t)n_iter;
  }
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(onp_iteration(h, s->np_rec + (size_t)it * 8));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  std::vector<double> rec((size_t)n_iter * 8);
  HIPCHK(hipMemcpy(rec.data(), s->np_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_np_rec(rec.data(), n_iter, perf_out, idiv_out);
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_onp_update(bnmtf_handle h, int which, int k, int l) try {
  CHK(onp_check(h, true));
  const bool tri = h->L > 0;
  const bool ok = (which == 0 && k >= 0 && k < h->K) || (which == 1 && tri && k >= 0 && k < h->K && l >= 0 && l < h->L) ||
                  (which == 2 && l >= 0 && l < (tri ? h->L : h->K));
  if (!ok) { set_error("bnmtf_onp_update: which %d / entry (%d, %d) out of range (0: rows, column k; 1: S, NMTF only; 2: columns, column l)", which, k, l); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  // the columns (or S entries) of a direction one after the other are its half sweep (its S step): the call that continues the
  // last one takes P as that one left it in escratch, every other one rebuilds it, as the half sweep's first column does
  const int col = which == 0 ? k : which == 1 ? k * h->L + l : l;
  const int last = which == 0 ? h->K : which == 1 ? h->K * h->L : (tri ? h->L : h->K);
  const bool resume = col > 0 && s->np_next_which == which && s->np_next_col == col;
  s->np_next_which = -1;
  if (which == 1) CHK(onp_s_step(h, col, col + 1, resume, true));
  else onp_enqueue_sweep(h, which == 0, col, col + 1, resume, true, nullptr);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if (col + 1 < last) { s->np_next_which = which; s->np_next_col = col + 1; }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_onp_metrics(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values, double* out8) try {
  CHK(onp_check(h, true));
  if (!out8 || (n > 0 && (!rows || !cols || !values))) { set_error("bnmtf_onp_metrics: null argument"); return BNMTF_EINVAL; }
  if (n >= ((uint64_t)1 << 31)) { set_error("bnmtf_onp_metrics: at most 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= h->I || cols[e] < 0 || cols[e] >= h->J) {
      set_error("bnmtf_onp_metrics: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], h->I, h->J);
      return BNMTF_EINVAL;
    }
  ObsState* s = h->obs;
  s->np_next_which = -1;               // (nothing here writes escratch; a metric call between two columns still ends the hand-over: one rule)
  OnpMetricArgs a; memset(&a, 0, sizeof(a));
  a.I = h->I; a.A = s->rows.X; a.ldA = s->rows.stride; a.B = s->cols.X; a.ldB = s->cols.stride;
  a.S = h->L > 0 ? s->npS : nullptr; a.K = h->K; a.L = h->L; a.part = s->np_mpart;
  DevBuf<uint32_t> dr, dc; DevBuf<float> dv;
  if (n == 0) {                        // the training entries: the row list itself
    a.row = nullptr; a.ptr = s->rows.ptr; a.col = s->rows.idx; a.val = s->rows.val; a.n = s->n;
  } else {
    CHK(dr.alloc(n)); CHK(dc.alloc(n)); CHK(dv.alloc(n));
    HIPCHK(hipMemcpyAsync(dr.p, rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));      // (checked non-negative: the same bits as uint32)
    HIPCHK(hipMemcpyAsync(dc.p, cols, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dv.p, values, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    a.row = dr.p; a.col = dc.p; a.val = dv.p; a.n = (size_t)n;
  }
  launch_onp_metric(a, s->out8, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out8, s->out8, 8 * sizeof(double), hipMemcpyDeviceToHost));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
