// The tri-factorisation on the observed-entry layout (C ABI part 7: bnmtf_gibbs_optimised / nmtf_icm with layout='observed') --
// included behind api_obs.inc at the end of api.hip.
// A handle of bnmtf_otri_create holds, in ObsTriState, the entry lists of bnmtf_obs_create (ObsLists / ObsList), F [I][32] and
// G [J][32] row major and transposed in fp32, the two effective factors G S^T [J][32] and F S [I][32] in the same two forms, the prior
// rates, Pv = R~^T F [J][32], the long form's residual scratch and the G half sweep's partial sums; and in the model itself S, its
// prior rates and the buffers of the dense S system (the ones bnmtf_alloc_extras gives a dense handle).  Nothing of size I x J.  A
// row stride of 32 is what kernel_ssys.hip's launchers read (SColGramArgs::F, GammaPackArgs::G, SSysBArgs::slabs), hence K, L <= 32.
// The iteration (DESIGN.md section 2.7): the F and G half sweeps are obs_sweep_kernel against an effective factor
// (obs_tri_eff_kernel), the S step is kernel_ssys.hip's system with its per-column inputs from the column list
// (obs_tri_gram_kernel); everything on the handle's stream, the samples through the SampleSink.

namespace bnmtf {

struct ObsTriState {
  ObsList rows, cols;              // F's and G's direction: lists, factor (X [n][32], XT [W][ldT]), prior rates, cond-params scratch
  float* ceffX = nullptr; float* ceffXT = nullptr;    // G S^T: [J][32] and [K][cols.ldT]
  float* reffX = nullptr; float* reffXT = nullptr;    // F S:   [I][32] and [L][rows.ldT]
  float* Pv = nullptr;             // [J][32]
  size_t n = 0;
  float* escratch = nullptr;       // [n]
  double* part = nullptr;          // [obs_sweep_blocks(J)][4]
  double* scal = nullptr;          // tau_d, tau_f and out8 of the metric sums (one allocation)
  double* out8 = nullptr;
  bool force_long = false;
  // the variational model on this handle (api_obs_trivb.inc): allocated by the first bnmtf_otvb_set_state.  q(F), q(G) live in
  // rows / cols {mu, tauq, var} beside the expectation X; q(S) in the model's muS, tauS, varS beside S
  bool vb_alloc = false, vb_state = false;   // the variational buffers exist; the handle holds the state of a bnmtf_otvb_set_state / run
  float* ceffS2 = nullptr; float* ceffS2T = nullptr;    // second moment of G S^T: [J][32] and [K][cols.ldT]
  float* reffS2 = nullptr; float* reffS2T = nullptr;    // second moment of F S:   [I][32] and [L][rows.ldT]
  double* esd_part = nullptr;      // [obs_vb_esd_blocks(I)]
};

static void otri_free(bnmtf_model* h) {
  ObsTriState* s = h->otri;
  if (!s) return;
  for (ObsList* d : {&s->rows, &s->cols}) {
    dfree(d->ptr); dfree(d->idx); dfree(d->val); dfree(d->X); dfree(d->XT); dfree(d->lambda); dfree(d->numer); dfree(d->taup);
    dfree(d->mu); dfree(d->tauq); dfree(d->var); dfree(d->vstat);
  }
  dfree(s->ceffS2); dfree(s->ceffS2T); dfree(s->reffS2); dfree(s->reffS2T); dfree(s->esd_part);
  dfree(s->ceffX); dfree(s->ceffXT); dfree(s->reffX); dfree(s->reffXT); dfree(s->Pv);
  dfree(s->escratch); dfree(s->part); dfree(s->scal);
  h->tau_d = nullptr; h->tau_f = nullptr;
  delete s;
  h->otri = nullptr;             // (S, lambdaS and the S system's buffers are the model's own: bnmtf_destroy frees them)
}

static int otri_check(bnmtf_model* h, bool need_state) {
  if (!h || !h->otri) { set_error("not a handle of bnmtf_otri_create"); return BNMTF_EINVAL; }
  if (need_state && !h->have_state) { set_error("bnmtf_otri_set_state has not been called"); return BNMTF_ESTATE; }
  if (need_state && h->otri->vb_state) {
    set_error("the handle holds a variational state (bnmtf_otvb_set_state): it runs the bnmtf_otvb_* calls until bnmtf_otri_set_state replaces it");
    return BNMTF_ESTATE;
  }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

// one direction: the list, the prior rates [n][32], the factor in both forms (W columns) and the hooks' scratch
static int otri_build_dir(bnmtf_model* h, ObsList& d, int n, int W, const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& idx,
                          const std::vector<float>& val, const double* lambda) {
  d.n = n; d.ldT = round_up(n + 1, 64);          // (a zero behind every column of the transposed forms: the sweep's empty slots gather it)
  CHK(upload(&d.ptr, ptr, h->stream));
  CHK(upload(&d.idx, idx, h->stream));
  CHK(upload(&d.val, val, h->stream));
  std::vector<float> lam((size_t)n * kObsTriStride, 0.f);
  for (int u = 0; u < n; ++u)
    for (int k = 0; k < W; ++k) lam[(size_t)u * kObsTriStride + k] = (float)lambda[(size_t)u * W + k];
  CHK(upload(&d.lambda, lam, h->stream));
  CHK(dalloc(&d.X, (size_t)n * kObsTriStride));
  CHK(dalloc(&d.XT, (size_t)W * d.ldT));
  CHK(dalloc(&d.numer, (size_t)n, false));
  CHK(dalloc(&d.taup, (size_t)n, false));
  for (int u = 0; u < n; ++u) {
    const uint32_t c = ptr[u + 1] - ptr[u];
    d.longest = std::max(d.longest, c);
    if (c > (uint32_t)kObsMaxSlots * 64u) d.long_units++;
  }
  return BNMTF_OK;
}

// fp64 host [n][W] -> fp32 device [n][32] and [W][ldT]
static int otri_put(bnmtf_model* h, ObsList& d, int W, const double* src) {
  std::vector<float> x((size_t)d.n * kObsTriStride, 0.f), xt((size_t)W * d.ldT, 0.f);
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < W; ++k) {
      const float v = (float)src[(size_t)u * W + k];
      x[(size_t)u * kObsTriStride + k] = v; xt[(size_t)k * d.ldT + u] = v;
    }
  HIPCHK(hipMemcpyAsync(d.X, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.XT, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

// the effective factor of a half sweep for the current state: rows (the F sweep): G S^T; else (the G sweep): F S
static void otri_enqueue_eff(bnmtf_model* h, bool rows) {
  ObsTriState* s = h->otri;
  ObsTriEffArgs e; memset(&e, 0, sizeof(e));
  e.S = h->S; e.K = h->K; e.L = h->L;
  if (rows) { e.X = s->cols.X; e.n = h->J; e.transposeS = 1; e.out = s->ceffX; e.outT = s->ceffXT; e.ldT = s->cols.ldT; }
  else      { e.X = s->rows.X; e.n = h->I; e.transposeS = 0; e.out = s->reffX; e.outT = s->reffXT; e.ldT = s->rows.ldT; }
  launch_obs_tri_eff(e, h->stream);
}

// the half sweep of F (rows) or G against its effective factor: a two-factor half sweep of rank K or L
static ObsSweepArgs otri_sweep_args(bnmtf_model* h, bool rows, int mode) {
  ObsTriState* s = h->otri;
  ObsList& d = rows ? s->rows : s->cols;
  ObsSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = rows ? h->J : h->I; a.K = rows ? h->K : h->L; a.KP = kObsTriStride;
  a.mode = mode; a.cond_k = -1; a.force_long = s->force_long ? 1 : 0; a.min_x = h->cur_min_x;
  a.lambda = d.lambda;
  a.X = d.X; a.XT = d.XT; a.ldT = d.ldT;
  a.Xo = rows ? s->ceffX : s->reffX; a.XoT = rows ? s->ceffXT : s->reffXT; a.ldT_o = rows ? s->cols.ldT : s->rows.ldT;
  a.escratch = s->escratch;
  a.tau = h->tau_f;
  a.key0 = (uint32_t)h->seed; a.key1 = (uint32_t)(h->seed >> 32); a.it = (uint32_t)h->iteration;
  a.stream = rows ? kStreamRows : kStreamCols;
  return a;
}

// (A, b) of the S system for the current F, G and the residual r = b - A S with the chain's candidates and triangular inverses:
// enqueue_ssys_build's sequence with the per-column inputs from the column list
static void otri_enqueue_ssys_build(bnmtf_model* h) {
  ObsTriState* s = h->otri;
  const int K = h->K, L = h->L, J = h->J, n2 = K * L;
  ObsTriGramArgs w; memset(&w, 0, sizeof(w));
  w.ptr = s->cols.ptr; w.idx = s->cols.idx; w.val = s->cols.val; w.n = J; w.K = K; w.F = s->rows.X; w.Wc = h->ss_Wc; w.Pv = s->Pv;
  launch_obs_tri_gram(w, h->stream);
  GammaPackArgs gp;
  gp.n = J; gp.n0 = 0; gp.L = L; gp.G = s->cols.X; gp.varG = nullptr; gp.Gc = h->ss_Gc;
  launch_gamma_pack(gp, h->stream);
  SSysBArgs b;
  b.n = J; b.n0 = 0; b.K = K; b.L = L; b.slabs = s->Pv; b.split = 1; b.n_pad = J; b.G = s->cols.X; b.b = h->ss_bpart;
  launch_ssys_b(b, h->stream);
  SSysGemmArgs g;
  g.n = J; g.K = K; g.L = L; g.nsplit = h->ss_nsplit; g.Wc = h->ss_Wc; g.Gc = h->ss_Gc; g.slabs = h->ss_slabs;
  launch_ssys_gemm(g, h->stream);
  launch_ssys_reduce(h->ss_slabs, h->ss_nsplit, K, L, h->ss_AB, h->stream);
  launch_ssys_residual(h->ss_AB, h->ss_AB + (size_t)n2 * n2, h->ss_bpart, ssys_b_blocks(J), h->S, n2, h->ss_r, h->stream,
                       h->ss_cands, (uint32_t)h->iteration, (uint32_t)h->seed, (uint32_t)(h->seed >> 32),
                       h->ss_tinv, K, L, h->tau_f, h->ss_rec, h->ss_rec + (size_t)1024 * 8, h->ss_rec + (size_t)1024 * 24);
}

}  // namespace bnmtf

extern "C" {

int bnmtf_otri_create(int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                      const double* lambda_F, const double* lambda_S, const double* lambda_G, double alpha, double beta,
                      uint64_t seed, int device, bnmtf_handle* out) try {
  if (!out) { set_error("bnmtf_otri_create: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!rows || !cols || !values || !lambda_F || !lambda_S || !lambda_G) { set_error("bnmtf_otri_create: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > BNMTF_OTRI_MAX_RANK || L < 1 || L > BNMTF_OTRI_MAX_RANK) {
    set_error("bnmtf_otri_create: unsupported shape I=%d J=%d K=%d L=%d (1 <= K, L <= %d)", I, J, K, L, BNMTF_OTRI_MAX_RANK);
    return BNMTF_EINVAL;
  }
  ObsLists ls;
  CHK(obs_lists(I, J, n, rows, cols, values, ls));
  HIPCHK(hipSetDevice(device));
  bnmtf_model* h = new bnmtf_model();
  h->I = I; h->J = J; h->K = K; h->L = L; h->device = device;
  h->alpha = alpha; h->beta = beta; h->seed = seed;
  h->n_obs = (double)n; h->sumR = ls.sumR; h->sumR2 = ls.sumR2;
  h->rows.nglob = I; h->rows.m = J; h->rows.W = K; h->cols.nglob = J; h->cols.m = I; h->cols.W = L;
  h->std_built = false;
  struct Guard { bnmtf_model* h; ~Guard() { if (h) bnmtf_destroy(h); } } guard{h};      // every way out but the last, an exception included, destroys the handle
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; set_error("hipStreamCreate failed"); return BNMTF_EHIP; }
  h->otri = new ObsTriState();
  ObsTriState* s = h->otri;
  s->n = (size_t)n;
  const char* fl = getenv("BNMTF_OBS_LONG");
  s->force_long = fl && fl[0] == '1';
  CHK(otri_build_dir(h, s->rows, I, K, ls.rptr, ls.ridx, ls.rval, lambda_F));
  CHK(otri_build_dir(h, s->cols, J, L, ls.cptr, ls.cidx, ls.cval, lambda_G));
  CHK(dalloc(&s->ceffX, (size_t)J * kObsTriStride)); CHK(dalloc(&s->ceffXT, (size_t)K * s->cols.ldT));
  CHK(dalloc(&s->reffX, (size_t)I * kObsTriStride)); CHK(dalloc(&s->reffXT, (size_t)L * s->rows.ldT));
  CHK(dalloc(&s->Pv, (size_t)J * kObsTriStride));
  CHK(dalloc(&s->escratch, (size_t)n, false));
  CHK(dalloc(&s->part, (size_t)obs_sweep_blocks(J) * 4, false));
  CHK(dalloc(&s->scal, 16));
  h->tau_d = s->scal; h->tau_f = reinterpret_cast<float*>(s->scal + 1); s->out8 = s->scal + 8;
  // S, its prior rates and the dense S system's buffers: what bnmtf_alloc_extras gives h->ssys, sized by its rules
  const size_t n2 = (size_t)K * L;
  CHK(dalloc(&h->S, n2));
  {
    std::vector<float> lsf(n2);
    for (size_t t = 0; t < n2; ++t) lsf[t] = (float)lambda_S[t];
    CHK(upload(&h->lambdaS, lsf, h->stream));
  }
  CHK(dalloc(&h->s_numer, 1)); CHK(dalloc(&h->s_taup, 1));
  h->ssys = true;
  const int wtiles = ssys_gemm_wave_tiles(K, L);
  h->ss_nsplit = std::max(1, std::min({512 / std::max((wtiles + 3) / 4, 1), std::max(J / 64, 1), 32}));
  const size_t nc = (size_t)J + 2;                                 // + 2 zero rows: what a column range reads past its end
  CHK(dalloc(&h->ss_Wc, nc * tri_padded(K)));                      // (dalloc zero-fills: the pads and the extra rows are never written)
  CHK(dalloc(&h->ss_Gc, nc * tri_padded(L)));
  CHK(dalloc(&h->ss_slabs, (size_t)h->ss_nsplit * tri_padded(K) * tri_padded(L)));
  CHK(dalloc(&h->ss_AB, n2 * n2 + n2));
  CHK(dalloc(&h->ss_r, n2));
  CHK(dalloc(&h->ss_cands, n2 * 16));
  CHK(dalloc(&h->ss_rec, (size_t)1024 * 25));
  CHK(dalloc(&h->ss_tinv, (size_t)K * 1024));
  CHK(dalloc(&h->ss_bpart, (size_t)ssys_b_blocks(J) * n2));
  char buf[640];
  snprintf(buf, sizeof(buf), "bnmtf layout=observed I=%d J=%d K=%d L=%d entries=%llu (%.3g %% of the matrix) longest_row=%u longest_column=%u "
           "long_form_units=%zu/%zu force_long=%d ssys[nsplit=%d range=%d bblocks=%d]", I, J, K, L, (unsigned long long)n,
           100.0 * (double)n / ((double)I * (double)J), s->rows.longest, s->cols.longest, s->rows.long_units, s->cols.long_units,
           (int)s->force_long, h->ss_nsplit, ssys_gemm_range(J, h->ss_nsplit), ssys_b_blocks(J));
  h->description = buf;
  guard.h = nullptr;
  *out = h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_set_state(bnmtf_handle h, const double* F, const double* S, const double* G, double tau) try {
  CHK(otri_check(h, false));
  if (!F || !S || !G) { set_error("bnmtf_otri_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(otri_put(h, h->otri->rows, h->K, F));
  CHK(otri_put(h, h->otri->cols, h->L, G));
  std::vector<float> sf((size_t)h->K * h->L);
  for (size_t t = 0; t < sf.size(); ++t) sf[t] = (float)S[t];
  HIPCHK(hipMemcpyAsync(h->S, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->otri->vb_state = false;          // (the factors were replaced: a variational state ends here)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_get_state(bnmtf_handle h, double* F, double* S, double* G, double* tau) try {
  CHK(otri_check(h, true));
  ObsTriState* s = h->otri;
  if (F) CHK(download_matrix(h, s->rows.X, h->I, h->K, kObsTriStride, F));
  if (G) CHK(download_matrix(h, s->cols.X, h->J, h->L, kObsTriStride, G));
  if (S) CHK(download_matrix(h, h->S, h->K, h->L, h->L, S));
  if (tau) {
    HIPCHK(hipMemcpyAsync(tau, h->tau_d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_run(bnmtf_handle h, int n_iter, int update, float* F_out, float* S_out, float* G_out, double* tau_out,
                   double* perf_out, double* times_out) try {
  CHK(otri_check(h, true));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsTriState* s = h->otri;
  CHK(ensure_rec(h, (size_t)n_iter));
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  if (mode == kSweepDraw) CHK(stage_gamma_variates(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  SampleSink sink;
  sink.add(s->rows.X, h->I, h->K, kObsTriStride, F_out);
  sink.add(h->S, h->K, h->L, h->L, S_out);
  sink.add(s->cols.X, h->J, h->L, kObsTriStride, G_out);
  CHK(sink.begin(h, n_iter));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    // ---- F columns: other = G S^T
    otri_enqueue_eff(h, true);
    ObsSweepArgs a = otri_sweep_args(h, true, mode);
    a.snap = sink.slot_for(it, s->rows.X);
    launch_obs_sweep(a, h->stream);
    // ---- S entries, row-major: the dense system of the new F and the old G
    otri_enqueue_ssys_build(h);
    enqueue_ssys_chain(h, update, -1);
    sink.snapshot(it, h->S);
    // ---- G columns: other = F S
    otri_enqueue_eff(h, false);
    a = otri_sweep_args(h, false, mode);
    a.snap = sink.slot_for(it, s->cols.X);
    a.part = s->part;
    launch_obs_sweep(a, h->stream);
    // ---- tau and the record, from the G sweep's final residual
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

int bnmtf_otri_cond_params(bnmtf_handle h, int which, int k, int l, double* numer_out, double* tau_out) try {
  CHK(otri_check(h, true));
  if (which < 0 || which > 2) { set_error("bnmtf_otri_cond_params: which is 0 (F), 1 (S) or 2 (G)"); return BNMTF_EINVAL; }
  if (!numer_out || !tau_out) { set_error("bnmtf_otri_cond_params: null argument"); return BNMTF_EINVAL; }
  if (which == 1) {
    if (k < 0 || k >= h->K || l < 0 || l >= h->L) { set_error("S index out of range"); return BNMTF_EINVAL; }
    otri_enqueue_ssys_build(h);
    enqueue_ssys_chain(h, BNMTF_UPDATE_DRAW, k * h->L + l);
    HIPCHK(hipMemcpyAsync(numer_out, h->s_numer, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(tau_out, h->s_taup, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return BNMTF_OK;
  }
  const bool rows = which == 0;
  const int col = rows ? k : l, W = rows ? h->K : h->L;
  if (col < 0 || col >= W) { set_error("column %d out of range", col); return BNMTF_EINVAL; }
  ObsList& d = rows ? h->otri->rows : h->otri->cols;
  otri_enqueue_eff(h, rows);
  ObsSweepArgs a = otri_sweep_args(h, rows, kSweepDraw);
  a.cond_k = col; a.numer_out = d.numer; a.tau_out = d.taup;
  launch_obs_sweep(a, h->stream);
  HIPCHK(hipMemcpyAsync(numer_out, d.numer, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tau_out, d.taup, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                           const double* F, const double* S, const double* G, double sums_out[6]) try {
  CHK(otri_check(h, false));
  if (!rows || !cols || !values || !F || !S || !G || !sums_out) { set_error("bnmtf_otri_metric_sums: null argument"); return BNMTF_EINVAL; }
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("bnmtf_otri_metric_sums: between 1 and 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= h->I || cols[e] < 0 || cols[e] >= h->J) {
      set_error("bnmtf_otri_metric_sums: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], h->I, h->J);
      return BNMTF_EINVAL;
    }
  const int I = h->I, J = h->J, K = h->K, L = h->L;
  std::vector<double> FS((size_t)I * L, 0.0);          // F S in fp64, summed in k order (metric_sums_impl's rule)
  for (int i = 0; i < I; ++i)
    for (int k = 0; k < K; ++k) {
      const double fik = F[(size_t)i * K + k];
      for (int l = 0; l < L; ++l) FS[(size_t)i * L + l] += fik * S[(size_t)k * L + l];
    }
  DevBuf<uint32_t> dr, dc; DevBuf<float> dv; DevBuf<double> dA, dB, part;
  CHK(dr.alloc(n)); CHK(dc.alloc(n)); CHK(dv.alloc(n));
  CHK(dA.alloc((size_t)I * L)); CHK(dB.alloc((size_t)J * L)); CHK(part.alloc((size_t)obs_metric_blocks(n) * 8));
  HIPCHK(hipMemcpyAsync(dr.p, rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));      // (checked non-negative: the same bits as uint32)
  HIPCHK(hipMemcpyAsync(dc.p, cols, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dv.p, values, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dA.p, FS.data(), (size_t)I * L * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dB.p, G, (size_t)J * L * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ObsMetricArgs a; memset(&a, 0, sizeof(a));
  a.row = dr.p; a.col = dc.p; a.val = dv.p; a.n = (size_t)n; a.A = dA.p; a.B = dB.p; a.K = L; a.part = part.p;
  launch_obs_metric(a, h->otri->out8, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  double out8[8];
  HIPCHK(hipMemcpy(out8, h->otri->out8, sizeof(out8), hipMemcpyDeviceToHost));
  for (int m = 0; m < 6; ++m) sums_out[m] = out8[m];
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
