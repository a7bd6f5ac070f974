// The tri-factorisation on the observed-entry layout (C ABI part 7: bnmtf_gibbs_optimised / nmtf_icm with layout='observed') --
// included behind api_obs.inc at the end of api.hip.
// A handle of bnmtf_otri_create holds the ObsState of api_obs.inc with its tri-factorisation parts: F [I][32] and G [J][32] as the
// two directions' factors (row major and transposed in fp32), the two effective factors G S^T [J][32] and F S [I][32] in the same
// two forms and Pv = R~^T F [J][32]; and in the model itself S, its prior rates and the buffers of the dense S system (the ones
// bnmtf_alloc_extras gives a dense handle).  Nothing of size I x J.  A row stride of 32 is what kernel_ssys.hip's launchers read
// (SColGramArgs::F, GammaPackArgs::G, SSysBArgs::slabs), hence K, L <= 32.
// The iteration (DESIGN.md section 2.7): the F and G half sweeps are obs_sweep_kernel against an effective factor
// (obs_tri_eff_kernel), the S step is kernel_ssys.hip's system with its per-column inputs from the column list
// (obs_tri_gram_kernel); everything on the handle's stream, the samples through the SampleSink.

namespace bnmtf {

// the effective factor of a half sweep for the current state: rows (the F sweep): G S^T; else (the G sweep): F S
static void otri_enqueue_eff(bnmtf_model* h, bool rows) {
  ObsState* s = h->obs;
  ObsTriEffArgs e; memset(&e, 0, sizeof(e));
  e.S = h->S; e.K = h->K; e.L = h->L;
  if (rows) { e.X = s->cols.X; e.n = h->J; e.transposeS = 1; e.out = s->ceffX; e.outT = s->ceffXT; e.ldT = s->cols.ldT; }
  else      { e.X = s->rows.X; e.n = h->I; e.transposeS = 0; e.out = s->reffX; e.outT = s->reffXT; e.ldT = s->rows.ldT; }
  launch_obs_tri_eff(e, h->stream);
}

// what the half sweep of F (rows) or G reads of its effective factor: G S^T over the column units, F S over the row units
static ObsOther otri_other(bnmtf_model* h, bool rows) {
  const ObsState* s = h->obs;
  if (rows) return ObsOther{s->ceffX, s->ceffXT, s->ceffS2T, s->cols.ldT, h->J};
  return ObsOther{s->reffX, s->reffXT, s->reffS2T, s->rows.ldT, h->I};
}

// (A, b) of the S system for the current F, G and the residual r = b - A S with the chain's candidates and triangular inverses:
// enqueue_ssys_build's sequence with the per-column inputs from the column list
static void otri_enqueue_ssys_build(bnmtf_model* h) {
  ObsState* s = h->obs;
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
  ObsCreateGuard guard;
  CHK(obs_create_common(guard, I, J, K, L, kObsTriStride, n, rows, cols, values, lambda_F, lambda_G, alpha, beta, seed, device));
  bnmtf_model* h = guard.h;
  ObsState* s = h->obs;
  CHK(dalloc(&s->ceffX, (size_t)J * kObsTriStride)); CHK(dalloc(&s->ceffXT, (size_t)K * s->cols.ldT));
  CHK(dalloc(&s->reffX, (size_t)I * kObsTriStride)); CHK(dalloc(&s->reffXT, (size_t)L * s->rows.ldT));
  CHK(dalloc(&s->Pv, (size_t)J * kObsTriStride));
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
  *out = guard.release();
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_set_state(bnmtf_handle h, const double* F, const double* S, const double* G, double tau) try {
  CHK(obs_check(h, true, kObsNoState));
  if (!F || !S || !G) { set_error("bnmtf_otri_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(obs_put(h, h->obs->rows, F));
  CHK(obs_put(h, h->obs->cols, G));
  std::vector<float> sf((size_t)h->K * h->L);
  for (size_t t = 0; t < sf.size(); ++t) sf[t] = (float)S[t];
  HIPCHK(hipMemcpyAsync(h->S, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->obs->vb_state = false;          // (the factors were replaced: a variational state ends here)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_get_state(bnmtf_handle h, double* F, double* S, double* G, double* tau) try {
  CHK(obs_check(h, true, kObsSamplerState));
  ObsState* s = h->obs;
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
  CHK(obs_check(h, true, kObsSamplerState));
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
  sink.add(s->rows.X, h->I, h->K, kObsTriStride, F_out);
  sink.add(h->S, h->K, h->L, h->L, S_out);
  sink.add(s->cols.X, h->J, h->L, kObsTriStride, G_out);
  CHK(sink.begin(h, n_iter));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    // ---- F columns: other = G S^T
    otri_enqueue_eff(h, true);
    ObsSweepArgs a = obs_sweep_args(h, true, otri_other(h, true), mode);
    a.snap = sink.slot_for(it, s->rows.X);
    launch_obs_sweep(a, h->stream);
    // ---- S entries, row-major: the dense system of the new F and the old G
    otri_enqueue_ssys_build(h);
    enqueue_ssys_chain(h, update, -1);
    sink.snapshot(it, h->S);
    // ---- G columns: other = F S
    otri_enqueue_eff(h, false);
    a = obs_sweep_args(h, false, otri_other(h, false), mode);
    a.snap = sink.slot_for(it, s->cols.X);
    a.part = s->part;
    launch_obs_sweep(a, h->stream);
    // ---- tau and the record, from the G sweep's final residual
    launch_obs_finish(obs_finish_args(h, update, it), h->stream);
    CHK(sink.close_slot(it));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sink.finish());
  HIPCHK(hipGetLastError());
  CHK(obs_fetch_rec(h, n_iter, tau_out, perf_out));
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otri_cond_params(bnmtf_handle h, int which, int k, int l, double* numer_out, double* tau_out) try {
  CHK(obs_check(h, true, kObsSamplerState));
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
  otri_enqueue_eff(h, rows);
  return obs_cond_params_dir(h, rows ? h->obs->rows : h->obs->cols, obs_sweep_args(h, rows, otri_other(h, rows), kSweepDraw), col, numer_out, tau_out);
} BNMTF_ABI_GUARD

int bnmtf_otri_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                           const double* F, const double* S, const double* G, double sums_out[6]) try {
  CHK(obs_check(h, true, kObsNoState));
  if (!rows || !cols || !values || !F || !S || !G || !sums_out) { set_error("bnmtf_otri_metric_sums: null argument"); return BNMTF_EINVAL; }
  const int I = h->I, K = h->K, L = h->L;
  std::vector<double> FS((size_t)I * L, 0.0);          // F S in fp64, summed in k order (metric_sums_impl's rule)
  for (int i = 0; i < I; ++i)
    for (int k = 0; k < K; ++k) {
      const double fik = F[(size_t)i * K + k];
      for (int l = 0; l < L; ++l) FS[(size_t)i * L + l] += fik * S[(size_t)k * L + l];
    }
  return obs_list_metric(h, "bnmtf_otri_metric_sums", n, rows, cols, values, FS.data(), G, L, sums_out);
} BNMTF_ABI_GUARD

}  // extern "C"
