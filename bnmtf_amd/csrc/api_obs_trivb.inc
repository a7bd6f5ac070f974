// The variational tri-factorisation on the observed-entry layout (C ABI part 8: bnmtf_vb_observed) -- included behind
// api_obs_tri.inc at the end of api.hip.  Five entry points on the handle of bnmtf_otri_create; the first bnmtf_otvb_set_state
// allocates what the variational model holds beyond the sampler's -- the variational parts of api_obs.inc's ObsState: q's mu, tau
// and variance of F and G [.][32] beside the expectations in rows.X / cols.X (obs_alloc_q, obs_put_q: the two-factor model's,
// without an S2T), the second moments of the two effective factors --, and in the model q(S) in muS, tauS, varS beside S,
// the masked variance sums mv_rows [I][32] / mv_cols [J][32], the chain's permuted system, the half sweeps' partial sums.  Nothing
// of size I x J.  The iteration (DESIGN.md section 2.7; bnmtf_vb_optimised.py:172-192 restated on the observed entries): the S
// entries on the second-moment system of kernel_ssys.hip with its per-column inputs from obs_tri_gram_vb_kernel, the F and G half
// sweeps on obs_trivb_sweep_kernel against the effective factors of obs_trivb_eff_kernel, everything on the handle's stream.  A
// variational state and a sampler's state exclude each other: each set_state ends the other's.

namespace bnmtf {

static int otvb_alloc(bnmtf_model* h) {
  ObsState* s = h->obs;
  if (s->vb_alloc) return BNMTF_OK;
  CHK(obs_alloc_q(h, s->rows, false));          // (no S2T: the half sweeps gather the effective factors' second moments)
  CHK(obs_alloc_q(h, s->cols, false));
  if (!s->ceffS2) CHK(dalloc(&s->ceffS2, (size_t)h->J * kObsTriStride));
  if (!s->ceffS2T) CHK(dalloc(&s->ceffS2T, (size_t)h->K * s->cols.ldT));
  if (!s->reffS2) CHK(dalloc(&s->reffS2, (size_t)h->I * kObsTriStride));
  if (!s->reffS2T) CHK(dalloc(&s->reffS2T, (size_t)h->L * s->rows.ldT));
  if (!s->esd_part) CHK(dalloc(&s->esd_part, (size_t)obs_vb_esd_blocks(h->I)));
  const size_t n2 = (size_t)h->K * h->L;
  if (!h->muS) CHK(dalloc(&h->muS, n2));
  if (!h->tauS) CHK(dalloc(&h->tauS, n2));
  if (!h->varS) CHK(dalloc(&h->varS, n2));
  if (!h->mv_rows) CHK(dalloc(&h->mv_rows, (size_t)h->I * kObsTriStride));
  if (!h->mv_cols) CHK(dalloc(&h->mv_cols, (size_t)h->J * kObsTriStride));
  if (!h->tri_third) CHK(dalloc(&h->tri_third, (size_t)std::max(tri_third_blocks(h->J), 1)));
  if (!h->ss_Aperm) CHK(dalloc(&h->ss_Aperm, n2 * n2));
  s->vb_alloc = true;
  return BNMTF_OK;
}

// W~_j (packed, with the variance sums on the diagonal), Pv_j and mv_cols of the current q(F): one pass over the column list
static void otvb_enqueue_gram(bnmtf_model* h) {
  ObsState* s = h->obs;
  ObsTriGramArgs w; memset(&w, 0, sizeof(w));
  w.ptr = s->cols.ptr; w.idx = s->cols.idx; w.val = s->cols.val; w.n = h->J; w.K = h->K; w.F = s->rows.X; w.Wc = h->ss_Wc; w.Pv = s->Pv;
  ObsTriGramVbArgs v; v.varF = s->rows.var; v.mv = h->mv_cols;
  launch_obs_tri_gram_vb(w, v, h->stream);
}

// (A~, b) of the second-moment S system for the current q(F), q(G) and r = b - A~ E[S]: enqueue_tri_ssys's sequence with the
// per-column inputs from the column list (gram_current: they are there, formed behind the F sweep)
static void otvb_enqueue_ssys(bnmtf_model* h, bool gram_current) {
  ObsState* s = h->obs;
  const int K = h->K, L = h->L, J = h->J, n2 = K * L;
  if (!gram_current) otvb_enqueue_gram(h);
  GammaPackArgs gp; memset(&gp, 0, sizeof(gp));
  gp.n = J; gp.n0 = 0; gp.L = L; gp.G = s->cols.X; gp.varG = s->cols.var; gp.Gc = h->ss_Gc;
  launch_gamma_pack(gp, h->stream);
  SSysGemmArgs g; memset(&g, 0, sizeof(g));
  g.n = J; g.K = K; g.L = L; g.nsplit = h->ss_nsplit; g.Wc = h->ss_Wc; g.Gc = h->ss_Gc; g.slabs = h->ss_slabs;
  launch_ssys_gemm(g, h->stream);
  launch_ssys_reduce(h->ss_slabs, h->ss_nsplit, K, L, h->ss_AB, h->stream);
  SSysBArgs b; memset(&b, 0, sizeof(b));
  b.n = J; b.n0 = 0; b.K = K; b.L = L; b.slabs = s->Pv; b.split = 1; b.n_pad = J; b.G = s->cols.X; b.b = h->ss_bpart;
  launch_ssys_b(b, h->stream);
  launch_ssys_residual(h->ss_AB, h->ss_AB + (size_t)n2 * n2, h->ss_bpart, ssys_b_blocks(J), h->S, n2, h->ss_r, h->stream);
}

// the chain over n_order entries of order_dev (enqueue_tri_chain: whole passes of K L >= 64 on the system in the pass's order)
static void otvb_enqueue_chain(bnmtf_model* h, const int* order_dev, int n_order, int only_params) {
  SSysChainVbArgs a; memset(&a, 0, sizeof(a));
  a.K = h->K; a.L = h->L; a.n_order = n_order; a.only_params = only_params; a.order = order_dev;
  a.A = h->ss_AB; a.r0 = h->ss_r; a.lambdaS = h->lambdaS; a.tau = h->tau_f;
  a.E = h->S; a.var = h->varS; a.mu = h->muS; a.tauq = h->tauS;
  a.Aperm = nullptr;
  if (n_order == h->K * h->L && !only_params && n_order >= 64) {
    launch_ssys_permute(h->ss_AB, order_dev, n_order, h->ss_Aperm, h->stream);
    a.Aperm = h->ss_Aperm;
  }
  launch_ssys_chain_vb(a, h->stream);
}

// what a half sweep of F (rows) or G needs of the other factor and S: the effective factor (mean and second moment) and, for F,
// the masked variance sums of G over the row list (those of F over the column list come with the column Grams)
static void otvb_enqueue_side(bnmtf_model* h, bool rows) {
  ObsState* s = h->obs;
  ObsTriVbEffArgs e; memset(&e, 0, sizeof(e));
  e.S = h->S; e.varS = h->varS; e.K = h->K; e.L = h->L;
  if (rows) { e.X = s->cols.X; e.varX = s->cols.var; e.n = h->J; e.transposeS = 1; e.out = s->ceffX; e.out2 = s->ceffS2; e.outT = s->ceffXT; e.out2T = s->ceffS2T; e.ldT = s->cols.ldT; }
  else      { e.X = s->rows.X; e.varX = s->rows.var; e.n = h->I; e.transposeS = 0; e.out = s->reffX; e.out2 = s->reffS2; e.outT = s->reffXT; e.out2T = s->reffS2T; e.ldT = s->rows.ldT; }
  launch_obs_trivb_eff(e, h->stream);
  if (rows) {
    ObsMvArgs m; memset(&m, 0, sizeof(m));
    m.ptr = s->rows.ptr; m.idx = s->rows.idx; m.n = h->I; m.V = s->cols.var; m.out = h->mv_rows;
    launch_obs_mv(m, h->stream);
  }
}

// the half sweep of F (rows) or G against its effective factor, with the column order and the covariance term's operands
static ObsVbSweepArgs otvb_sweep_args(bnmtf_model* h, bool rows, const int* order_dev) {
  ObsVbSweepArgs a = obs_vb_sweep_args(h, rows, otri_other(h, rows));
  a.XT = nullptr;                                  // (XT / S2T: not written by this instantiation; a tri list owns no S2T)
  a.order = order_dev; a.cov_S = h->S; a.cov_mv = rows ? h->mv_rows : h->mv_cols;
  if (rows) { a.cov_sc = h->L; a.cov_st = 1; a.cov_n = h->L; }       // column k of F, inner l: S[k][l] (tri_sweep_args)
  else      { a.cov_sc = 1; a.cov_st = h->L; a.cov_n = h->K; }       // column l of G, inner k: S[k][l]
  return a;
}

static int otvb_reserve_order(bnmtf_model* h, size_t n) {
  if (h->tri_order_cap >= n) return BNMTF_OK;
  dfree(h->tri_order); h->tri_order_cap = 0;
  CHK(dalloc(&h->tri_order, n, false));
  h->tri_order_cap = n;
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_otvb_set_state(bnmtf_handle h, const double* muF, const double* tauF, const double* expF, const double* varF,
                         const double* muS, const double* tauS, const double* expS, const double* varS,
                         const double* muG, const double* tauG, const double* expG, const double* varG, double exptau) try {
  CHK(obs_check(h, true, kObsNoState));
  if (!muF || !tauF || !expF || !varF || !muS || !tauS || !expS || !varS || !muG || !tauG || !expG || !varG) {
    set_error("bnmtf_otvb_set_state: null argument"); return BNMTF_EINVAL;
  }
  CHK(otvb_alloc(h));
  h->obs->vb_state = false;
  h->have_state = false;                 // (the expectations are replaced: a sampler's state ends here)
  CHK(obs_put_q(h, h->obs->rows, muF, tauF, expF, varF));
  CHK(obs_put_q(h, h->obs->cols, muG, tauG, expG, varG));
  const size_t n2 = (size_t)h->K * h->L;
  std::vector<float> tmp(n2);
  const double* src[4] = {muS, tauS, expS, varS};
  float* dst[4] = {h->muS, h->tauS, h->S, h->varS};
  for (int q = 0; q < 4; ++q) {
    for (size_t t = 0; t < n2; ++t) tmp[t] = (float)src[q][t];
    HIPCHK(hipMemcpyAsync(dst[q], tmp.data(), n2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  CHK(set_tau(h, exptau));
  h->have_state = true;
  h->obs->vb_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otvb_get_state(bnmtf_handle h, double* muF, double* tauF, double* expF, double* varF,
                         double* muS, double* tauS, double* expS, double* varS,
                         double* muG, double* tauG, double* expG, double* varG) try {
  CHK(obs_check(h, true, kObsVbState));
  ObsList& r = h->obs->rows; ObsList& c = h->obs->cols;
  if (muF) CHK(download_matrix(h, r.mu, h->I, h->K, kObsTriStride, muF));
  if (tauF) CHK(download_matrix(h, r.tauq, h->I, h->K, kObsTriStride, tauF));
  if (expF) CHK(download_matrix(h, r.X, h->I, h->K, kObsTriStride, expF));
  if (varF) CHK(download_matrix(h, r.var, h->I, h->K, kObsTriStride, varF));
  if (muG) CHK(download_matrix(h, c.mu, h->J, h->L, kObsTriStride, muG));
  if (tauG) CHK(download_matrix(h, c.tauq, h->J, h->L, kObsTriStride, tauG));
  if (expG) CHK(download_matrix(h, c.X, h->J, h->L, kObsTriStride, expG));
  if (varG) CHK(download_matrix(h, c.var, h->J, h->L, kObsTriStride, varG));
  double* dst[4] = {muS, tauS, expS, varS};
  const float* src[4] = {h->muS, h->tauS, h->S, h->varS};
  for (int q = 0; q < 4; ++q) if (dst[q]) CHK(download_matrix(h, src[q], h->K, h->L, h->L, dst[q]));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// update_F(k) (which = 0), update_S(k, l) (which = 1), update_G(l) (which = 2) for the state the device holds; moments != 0 also
// the matching update_exp_*
int bnmtf_otvb_update(bnmtf_handle h, int which, int k, int l, int moments) try {
  CHK(obs_check(h, true, kObsVbState));
  if (which < 0 || which > 2) { set_error("bnmtf_otvb_update: which is 0 (F), 1 (S) or 2 (G)"); return BNMTF_EINVAL; }
  if (which == 1) {
    if (k < 0 || k >= h->K || l < 0 || l >= h->L) { set_error("S index out of range"); return BNMTF_EINVAL; }
    CHK(otvb_reserve_order(h, 64));
    const int a = k * h->L + l;
    HIPCHK(hipMemcpyAsync(h->tri_order, &a, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));          // (a is a local)
    otvb_enqueue_ssys(h, false);
    otvb_enqueue_chain(h, h->tri_order, 1, moments ? 0 : 1);
  } else {
    const bool rows = which == 0;
    const int col = rows ? k : l, W = rows ? h->K : h->L;
    if (col < 0 || col >= W) { set_error("column %d out of range", col); return BNMTF_EINVAL; }
    if (!rows) otvb_enqueue_gram(h);                   // (mv_cols of the current q(F))
    otvb_enqueue_side(h, rows);
    ObsVbSweepArgs a = otvb_sweep_args(h, rows, nullptr);
    a.only_k = col; a.moments = moments ? 1 : 0;
    launch_obs_trivb_sweep(a, h->stream);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_otvb_exp_square_diff(bnmtf_handle h, double* out) try {
  CHK(obs_check(h, true, kObsVbState));
  if (!out) { set_error("bnmtf_otvb_exp_square_diff: null argument"); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  ObsTriVbEsdArgs a; memset(&a, 0, sizeof(a));
  a.ptr = s->rows.ptr; a.idx = s->rows.idx; a.val = s->rows.val; a.n = h->I; a.K = h->K; a.L = h->L;
  a.F = s->rows.X; a.varF = s->rows.var; a.G = s->cols.X; a.varG = s->cols.var; a.S = h->S; a.varS = h->varS; a.part = s->esd_part;
  launch_obs_trivb_esd(a, s->out8, h->stream);
  HIPCHK(hipMemcpyAsync(out, s->out8, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// run(iterations).  orders [n_iter][K L + K + L]: per iteration the S entries (k L + l), the F columns and the G columns in update
// order, each a list of valid indices; they go to the device once.  Outputs as bnmtf_vb_run's.
int bnmtf_otvb_run(bnmtf_handle h, int n_iter, const int32_t* orders, double* exptau_out, double* perf_out, double* elbo_terms_out,
                   double* times_out) try {
  CHK(obs_check(h, true, kObsVbState));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  if (!orders) { set_error("bnmtf_otvb_run: orders required"); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  const int K = h->K, L = h->L, n2 = K * L, per = n2 + K + L;
  for (int it = 0; it < n_iter; ++it)          // (the kernels index S, F and G with them)
    for (int t = 0; t < per; ++t) {
      const int v = orders[(size_t)it * per + t], lim = t < n2 ? n2 : (t < n2 + K ? K : L);
      if (v < 0 || v >= lim) { set_error("bnmtf_otvb_run: order %d of iteration %d is %d, outside 0 .. %d", t, it, v, lim - 1); return BNMTF_EINVAL; }
    }
  CHK(otvb_reserve_order(h, (size_t)n_iter * per));
  HIPCHK(hipMemcpyAsync(h->tri_order, orders, (size_t)n_iter * per * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(vb_reserve_rec(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    const int* ord = h->tri_order + (size_t)it * per;
    // ---- S entries: the system of the current q(F), q(G); its column Grams came from behind the last F sweep of this call
    otvb_enqueue_ssys(h, it > 0);
    otvb_enqueue_chain(h, ord, n2, 0);
    // ---- F columns against G S^T
    otvb_enqueue_side(h, true);
    ObsVbSweepArgs a = otvb_sweep_args(h, true, ord + n2);
    a.stat = s->rows.vstat;
    launch_obs_trivb_sweep(a, h->stream);
    // ---- behind the F sweep: W~_j, Pv_j and mvF_j of the new q(F) -- the G sweep's, the third term's and the next S system's
    otvb_enqueue_gram(h);
    // ---- G columns against F S
    otvb_enqueue_side(h, false);
    a = otvb_sweep_args(h, false, ord + n2 + K);
    a.stat = s->cols.vstat; a.part = s->part;
    launch_obs_trivb_sweep(a, h->stream);
    // ---- update_tau, update_exp_tau and the record
    TriThirdArgs t3; memset(&t3, 0, sizeof(t3));
    t3.rows = h->J; t3.K = K; t3.L = L; t3.G = s->cols.X; t3.S = h->S; t3.mv = h->mv_cols; t3.part = h->tri_third;
    launch_tri_third(t3, h->stream);
    ObsTriVbFinishArgs f; memset(&f, 0, sizeof(f));
    f.f = obs_vb_finish_args(h, it);
    f.third = h->tri_third; f.n_third = tri_third_blocks(h->J);
    launch_obs_trivb_finish(f, h->stream);
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

}  // extern "C"
