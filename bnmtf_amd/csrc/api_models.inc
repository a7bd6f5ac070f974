// BNMTF Gibbs driver (C ABI part 2) -- included at the end of api.hip.

namespace bnmtf {

// effective factors share the factor-storage part of Dir (no R shard, no slots)
static int alloc_eff(Dir& e, int nglob, int W, int other_inner_pad) {
  e.nglob = nglob; e.W = W; e.KP = W <= 32 ? 32 : 64;
  CHK(alloc_factor(e, other_inner_pad));
  CHK(dalloc(&e.C64, (size_t)64 * 64));
  CHK(dalloc(&e.C32, (size_t)64 * 64));
  CHK(dalloc(&e.colsum, 64));
  CHK(dalloc(&e.colsum2, 64));
  return BNMTF_OK;
}

static int bnmtf_alloc_extras(bnmtf_model* h, const double* lambdaS) {
  const int K = h->K, L = h->L;
  CHK(alloc_eff(h->reff, h->I, L, h->cols.inner_pad));     // U_eff = F S   (I x L)
  CHK(alloc_eff(h->ceff, h->J, K, h->rows.inner_pad));     // V_eff = G S^T (J x K)
  CHK(dalloc(&h->slabsS, (size_t)h->cols.split * h->cols.n_pad * h->rows.KP));
  CHK(dalloc(&h->CfS, (size_t)K * L));
  CHK(dalloc(&h->deltaS, 64));
  h->s_blocks = (h->cols.n + 15) / 16;
  CHK(dalloc(&h->s_partial, (size_t)std::max(h->s_blocks, 1) * L));
  CHK(dalloc(&h->s_w, (size_t)std::max(h->cols.n, 1) * h->rows.KP));
  CHK(dalloc(&h->s_omp, (size_t)K * kSOmegaChunks * h->cols.KP * h->cols.KP));
  std::vector<float> ls((size_t)K * L);
  for (size_t t = 0; t < ls.size(); ++t) ls[t] = (float)lambdaS[t];
  CHK(dalloc(&h->lambdaS, ls.size(), false));
  HIPCHK(hipMemcpy(h->lambdaS, ls.data(), ls.size() * sizeof(float), hipMemcpyHostToDevice));
  CHK(dalloc(&h->s_numer, 1)); CHK(dalloc(&h->s_taup, 1));
  // the dense K.L x K.L system of the S step (kernel_ssys.hip) when a row / a column Gram is one 32 x 32 MFMA tile
  h->ssys = K <= 32 && L <= 32 && !(getenv("BNMTF_SSYS") && atoi(getenv("BNMTF_SSYS")) == 0);
  if (h->ssys) {
    const size_t n2 = (size_t)K * L;
    const int wtiles = ssys_gemm_wave_tiles(K, L);                 // 2 x 2 MFMA tiles per wave over the packed (k <= k') x (l <= l') pairs
    // column ranges: at most 512 blocks of four waves = two per CU, ALL resident at once -- with a few more than that some CUs
    // run three blocks back to back while the rest idle (525 blocks measured 37 us against 21 us of MFMA time)
    h->ss_nsplit = std::max(1, std::min({512 / std::max((wtiles + 3) / 4, 1), std::max(h->cols.n / 64, 1), 32}));
    const size_t nc = (size_t)std::max(h->cols.n, 1) + 2;          // + 2 zero rows: what a column range reads past its end
    CHK(dalloc(&h->ss_Wc, nc * tri_padded(K)));                     // (dalloc zero-fills: the pads and the extra rows are never written)
    CHK(dalloc(&h->ss_Gc, nc * tri_padded(L)));
    CHK(dalloc(&h->ss_slabs, (size_t)h->ss_nsplit * tri_padded(K) * tri_padded(L)));
    CHK(dalloc(&h->ss_AB, n2 * n2 + n2));
    CHK(dalloc(&h->ss_r, n2));
    CHK(dalloc(&h->ss_cands, n2 * 16));                            // [K L][4 candidates][4 floats]
    CHK(dalloc(&h->ss_rec, (size_t)1024 * 25));                             // [K L][4] own constants + [K L][4 candidates][4]: the chain's records
    CHK(dalloc(&h->ss_tinv, (size_t)K * 1024));                    // [K][32][32]: the rows' triangular inverses (the chain multiplies, it does not walk)
    CHK(dalloc(&h->ss_bpart, (size_t)ssys_b_blocks(h->cols.n) * n2));
  }
  return BNMTF_OK;
}

// (A, b) of the S system for the current F, G (and the residual r = b - A S): everything the K.L conditionals need
static int enqueue_ssys_build(bnmtf_model* h) {
  Dir& c = h->cols; Dir& r = h->rows;
  const int K = h->K, L = h->L, n2 = K * L;
  // b's side of the system (the pass over R~ for Pv = R~^T F, then b = sum_j Pv_j (x) G_j) does not meet A's side (the masked
  // column Grams, the packed GEMM) before the residual: BNMTF_S_STREAMS=1 runs it on a second stream beside A's side
  // (measured twice, rounds 2 and 5: the S step's own timer -14 us, the iteration unchanged or slower -- make EXPERIMENTS=1)
#ifdef BNMTF_EXPERIMENTS
  static const bool two_streams = getenv("BNMTF_S_STREAMS") != nullptr && atoi(getenv("BNMTF_S_STREAMS")) != 0;
#else
  constexpr bool two_streams = false;
#endif
  hipStream_t sb = h->stream;
  if (two_streams) {
    if (!h->aux_stream) HIPCHK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&h->ev_aux0, &h->ev_aux1})
      if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIPCHK(hipEventRecord(h->ev_aux0, h->stream));
    HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_aux0, 0));
    sb = h->aux_stream;
  }
  {
    GemmArgs g;
    g.big = c.big; g.ld = c.n_pad; g.X = r.X; g.slabs = h->slabsS; g.n_pad = c.n_pad; g.split = c.split; g.inner_per_wave = c.ipw; g.tw = c.gemm_tw;
    launch_gemm(g, r.KP, sb);                              // Pv = R~^T F on the local columns
  }
  bool b_in_gram = false;
  SSysBArgs bargs;
  {
    SSysBArgs b;
    b.n = c.n; b.n0 = c.n0; b.K = K; b.L = L; b.slabs = h->slabsS; b.split = c.split; b.n_pad = c.n_pad; b.G = c.X; b.b = h->ss_bpart;
    // (one GPU, one stream: b's blocks ride in the column Grams' launch, below -- both follow the contraction, neither reads the other)
    b_in_gram = !two_streams && !h->comm;
    bargs = b;
    if (!b_in_gram) launch_ssys_b(b, sb);
    // (several GPUs: b is summed over the ranks with A, so it has to exist ahead of the residual kernel, which otherwise adds b's parts itself)
    if (h->comm) launch_ssys_sum_parts(h->ss_bpart, ssys_b_blocks(c.n), (size_t)n2, h->ss_AB + (size_t)n2 * n2, sb);
    if (two_streams) HIPCHK(hipEventRecord(h->ev_aux1, sb));
  }
  SColGramArgs w;
  w.n = c.n; w.K = K; w.F = r.X; w.varF = nullptr; w.Cf64 = r.C64; w.cf_diag_extra = nullptr;
  w.slot_ptr = c.slot_ptr; w.idx = c.idx; w.Wc = h->ss_Wc;
  GammaPackArgs gp;
  gp.n = c.n; gp.n0 = c.n0; gp.L = L; gp.G = c.X; gp.varG = nullptr; gp.Gc = h->ss_Gc;
  launch_scol_gram(w, gp, h->stream, b_in_gram ? &bargs : nullptr);   // + the packed second moments of G's rows (and b's blocks), in the same launch
  SSysGemmArgs g;
  g.n = c.n; g.K = K; g.L = L; g.nsplit = h->ss_nsplit; g.Wc = h->ss_Wc; g.Gc = h->ss_Gc; g.slabs = h->ss_slabs;
  launch_ssys_gemm(g, h->stream);
  launch_ssys_reduce(h->ss_slabs, h->ss_nsplit, K, L, h->ss_AB, h->stream);
  if (two_streams) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_aux1, 0));
  if (h->comm) CHK(comm_allreduce_sum_f32(h->comm, h->ss_AB, n2 * n2 + n2, h->stream));   // the K.L Gram exchange: one all-reduce
  launch_ssys_residual(h->ss_AB, h->ss_AB + (size_t)n2 * n2, h->comm ? nullptr : h->ss_bpart, ssys_b_blocks(c.n), h->S, n2, h->ss_r, h->stream,
                       h->ss_cands, (uint32_t)h->iteration, (uint32_t)h->seed, (uint32_t)(h->seed >> 32),   // + the chain's first candidates for this iteration
                       h->ss_tinv, K, L, h->tau_f, h->ss_rec, h->ss_rec + (size_t)1024 * 8, h->ss_rec + (size_t)1024 * 24);                                                       // + its rows' triangular inverses
  return BNMTF_OK;
}
static void enqueue_ssys_chain(bnmtf_model* h, int update, int cond) {
  SSysChainArgs a;
  a.K = h->K; a.L = h->L; a.update = update; a.cond = cond; a.min_x = update != 0 ? h->cur_min_x : 0.f;
  a.A = h->ss_AB; a.r0 = h->ss_r; a.S = h->S; a.lambdaS = h->lambdaS; a.tau = h->tau_f;
  a.key0 = (uint32_t)h->seed; a.key1 = (uint32_t)(h->seed >> 32); a.it = (uint32_t)h->iteration;
  a.cands = reinterpret_cast<const float4*>(h->ss_cands); a.Tinv = h->ss_tinv;
  a.own8 = reinterpret_cast<const float4*>(h->ss_rec); a.recT = reinterpret_cast<const float4*>(h->ss_rec + (size_t)1024 * 8); a.Tn = h->ss_rec + (size_t)1024 * 24;
  a.numer_out = h->s_numer; a.tau_out = h->s_taup;
  launch_ssys_chain(a, h->stream);
}

static void enqueue_small_product(bnmtf_model* h, const Dir& src, Dir& dst, int transposeS) {
  // (forming the product inside the relayout kernel, as its rows are staged, was tried in round 3: the relayout kernel
  // went from 7 to 19 us -- 16 KB more LDS per block, fewer blocks resident -- against the 7 us of this launch)
  SmallProductArgs p;
  p.X = src.X; p.rows = src.nglob; p.KPin = src.KP; p.S = h->S; p.K = h->K; p.L = h->L;
  p.transposeS = transposeS; p.out = dst.X; p.KPout = dst.KP;
  launch_small_product(p, h->stream);
  enqueue_post(h, dst);
}

// one row k of S (all L entries, or only the evaluation of (k, cond_l))
static void enqueue_srow(bnmtf_model* h, int k, int update, int cond_l, bool apply_prev) {
  Dir& c = h->cols; Dir& r = h->rows;
  SRowArgs a;
  a.n = c.n; a.n0 = c.n0; a.k = k; a.K = h->K; a.L = h->L; a.KPk = r.KP; a.KPl = c.KP;
  a.G = c.X; a.FT = r.XT; a.ldT = r.ldT; a.slabs = h->slabsS; a.split = c.split; a.n_pad = c.n_pad;
  a.slot_ptr = c.slot_ptr; a.idx = c.idx; a.q = c.q; a.CfS = h->CfS;
  a.delta_prev = h->deltaS; a.apply_prev = apply_prev ? 1 : 0; a.partial = h->s_partial;
  launch_srow_gather(a, h->s_blocks, h->stream);
  SDrawArgs d;
  d.k = k; d.K = h->K; d.L = h->L; d.KPk = r.KP; d.nblocks = h->s_blocks; d.update = update; d.cond_l = cond_l; d.LP = c.KP; d.nch = kSOmegaChunks; d.min_x = update != 0 ? h->cur_min_x : 0.f;
  d.partial = h->s_partial; d.omp = h->s_omp; d.S = h->S; d.lambdaS = h->lambdaS; d.tau = h->tau_f; d.Cf64 = r.C64; d.CfS = h->CfS;
  d.delta_out = h->deltaS; d.key0 = (uint32_t)h->seed; d.key1 = (uint32_t)(h->seed >> 32); d.it = (uint32_t)h->iteration;
  d.word0 = h->s_word0; d.ldword = h->s_ldword > 0 ? h->s_ldword : h->L;
  d.numer_out = h->s_numer; d.tau_out = h->s_taup;
  launch_srow_draw(d, h->stream);
}

// everything the S rows need for the current (F, S, G): Pv = R~^T F, U_eff, q, Cf.S
static void enqueue_s_prepare(bnmtf_model* h) {
  Dir& c = h->cols; Dir& r = h->rows;
  {
    GemmArgs g;
    g.big = c.big; g.ld = c.n_pad; g.X = r.X; g.slabs = h->slabsS; g.n_pad = c.n_pad; g.split = c.split; g.inner_per_wave = c.ipw; g.tw = c.gemm_tw;
    launch_gemm(g, r.KP, h->stream);
  }
  SOmegaArgs o;
  o.n = c.n; o.n0 = c.n0; o.K = h->K; o.L = h->L; o.KPk = r.KP; o.KPl = c.KP; o.nch = kSOmegaChunks; o.zero_row = r.nglob;
  o.F = r.X; o.G = c.X; o.Cf32 = r.C32; o.slot_ptr = c.slot_ptr; o.idx = c.idx; o.w = h->s_w; o.omp = h->s_omp;
  // q_ij = U_eff,i . G_j on the missing entries (column slots), U_eff = F S
  if (c.KP == 32) {
    SmallProductArgs p;
    p.X = r.X; p.rows = r.nglob; p.KPin = r.KP; p.S = h->S; p.K = h->K; p.L = h->L; p.transposeS = 0; p.out = h->reff.X; p.KPout = h->reff.KP;
    launch_small_product(p, h->stream);                   // rows only: no relayout / Gram of U_eff is needed here
    launch_srow_qinit(o, h->reff.X, c.q, h->stream);
  } else {
    enqueue_small_product(h, r, h->reff, 0);
    SweepArgs s = sweep_args(h, c, h->reff, kSweepDraw, kStreamCols);
    s.qinit_only = 1;
    launch_sweep(s, h->stream);
  }
  launch_cfs(r.C64, r.KP, h->S, h->K, h->L, h->CfS, h->stream);
  launch_srow_omega(o, h->stream);
}

}  // namespace bnmtf

extern "C" {

int bnmtf_set_state(bnmtf_handle h, const double* F, const double* S, const double* G, double tau) try {
  CHK(refuse_obs(h, "bnmtf_set_state"));
  if (h->L == 0) { set_error("bnmtf_set_state on a BNMF handle"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  h->std_cur = false; h->small_cur = false;
  h->tri_pv_current = h->tri_mv_cols_current = h->tri_w_current = false;
  if (h->std_built) {
    CHK(upload_factor(h, h->rows, F));
    CHK(upload_factor(h, h->cols, G));
    std::vector<float> sf((size_t)h->K * h->L);
    for (size_t t = 0; t < sf.size(); ++t) sf[t] = (float)S[t];
    HIPCHK(hipMemcpyAsync(h->S, sf.data(), sf.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->std_cur = true;
  }
  if (h->small) CHK(small_upload_state(h, F, G, S));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->ho_regions_current = false;          // (q hand-over: whatever the regions hold belongs to the state that was just replaced)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_get_state(bnmtf_handle h, double* F, double* S, double* G, double* tau) try {
  CHK(refuse_obs(h, "bnmtf_get_state"));
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  if (h->small && h->small_cur) CHK(small_download_state(h, F, G, S));
  else {
    if (F) CHK(download_matrix(h, h->rows.X, h->I, h->rows.W, h->rows.KP, F));
    if (G) CHK(download_matrix(h, h->cols.X, h->J, h->cols.W, h->cols.KP, G));
  }
  if (S && !(h->small && h->small_cur)) {
    std::vector<float> sf((size_t)h->K * h->L);
    HIPCHK(hipMemcpyAsync(sf.data(), h->S, sf.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t t = 0; t < sf.size(); ++t) S[t] = sf[t];
  }
  if (tau) {
    HIPCHK(hipMemcpyAsync(tau, h->tau_d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_cond_params(bnmtf_handle h, int which, int k, int l, double* numer_out, double* tau_out) try {
  if (h->L == 0) { set_error("bnmtf_cond_params on a BNMF handle"); return BNMTF_ESTATE; }
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  if (h->world != 1) { set_error("cond_params is a single-GPU test hook"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));
  if (which == 1) {
    if (k < 0 || k >= h->K || l < 0 || l >= h->L) { set_error("S index out of range"); return BNMTF_EINVAL; }
    if (h->ssys) {
      CHK(enqueue_ssys_build(h));
      enqueue_ssys_chain(h, BNMTF_UPDATE_DRAW, k * h->L + l);
    } else {
      enqueue_s_prepare(h);
      enqueue_srow(h, k, BNMTF_UPDATE_DRAW, l, false);
    }
    HIPCHK(hipMemcpyAsync(numer_out, h->s_numer, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(tau_out, h->s_taup, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return BNMTF_OK;
  }
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& e = which == 0 ? h->ceff : h->reff;
  const int col = which == 0 ? k : l;
  if (col < 0 || col >= d.W) { set_error("column %d out of range", col); return BNMTF_EINVAL; }
  if (which == 0) enqueue_small_product(h, h->cols, h->ceff, 1);   // V_eff = G S^T
  else            enqueue_small_product(h, h->rows, h->reff, 0);   // U_eff = F S
  enqueue_gemm(h, d, e, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
  SweepArgs s = sweep_args(h, d, e, kSweepDraw, which == 0 ? kStreamRows : kStreamCols);
  s.cond_k = col;
  enqueue_sweep(h, d, e, s, false);
  HIPCHK(hipMemcpyAsync(numer_out, d.numer, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tau_out, d.taup, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// A BNMTF handle as block (rows row0.., columns col0..) of the S of a WIDER tri-factorisation (bnmtf_amd/_blocked.py: TriBlocks): the
// draws of its entries are keyed by their place in the wide S (L_wide columns), its S step runs row by row (bnmtf_s_rows), never
// on the one-launch path or the dense system (whose candidate records are keyed by the handle's own K L).
int bnmtf_set_s_block(bnmtf_handle h, int row0, int col0, int L_wide) try {
  CHK(refuse_obs(h, "bnmtf_set_s_block"));
  if (h->L == 0 || h->comm) { set_error("bnmtf_set_s_block: BNMTF handles on one GPU"); return BNMTF_ESTATE; }
  if (row0 < 0 || col0 < 0 || L_wide < col0 + h->L) { set_error("bnmtf_set_s_block: the block does not lie inside a K x %d matrix", L_wide); return BNMTF_EINVAL; }
  h->s_word0 = (uint32_t)row0 * (uint32_t)L_wide + (uint32_t)col0;
  h->s_ldword = L_wide;
  h->block_mode = true;
  h->small_mode = 0;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// Rows k0 .. k1-1 of S (bnmtf_gibbs_optimised.py:157-160 restricted to those rows, every l in order) for the handle's current F, G,
// tau, iteration counter and DATA (bnmf_set_residual_data: what the rest of a wider model explains taken off R).  The caller
// owns everything else of the iteration.
int bnmtf_s_rows(bnmtf_handle h, int k0, int k1, int update) try {
  if (h->L == 0 || h->comm) { set_error("bnmtf_s_rows: BNMTF handles on one GPU"); return BNMTF_ESTATE; }
  if (k0 < 0 || k1 > h->K || k0 > k1 || update < 0 || update > BNMTF_UPDATE_ICM) { set_error("bnmtf_s_rows: rows [%d, %d) of %d, a known update rule", k0, k1, h->K); return BNMTF_EINVAL; }
  if (!h->have_state) { set_error("no state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));
  if (!h->std_cur) { set_error("bnmtf_s_rows: set the state first"); return BNMTF_ESTATE; }
  h->small_cur = false;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  enqueue_s_prepare(h);
  for (int k = k0; k < k1; ++k) enqueue_srow(h, k, update, -1, k > k0);
  // (the last row's deltas are applied to q by the next row's gather: nothing reads q behind the last row here)
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_gibbs_run(bnmtf_handle h, int n_iter, int update, float* F_out, float* S_out, float* G_out,
                    double* tau_out, double* perf_out, double* times_out) try {
  if (h->L == 0) { set_error("bnmtf_gibbs_run on a BNMF handle"); return BNMTF_ESTATE; }
  if (!h->have_state) { set_error("bnmtf_gibbs_run before bnmtf_set_state"); return BNMTF_ESTATE; }
  if (n_iter <= 0) return n_iter == 0 ? BNMTF_OK : BNMTF_EINVAL;
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  CHK(heldout_begin(h, n_iter));
  if (small_wanted(h)) {                       // a small model: the whole call is one launch (kernel_small.hip)
    SmallOut o{F_out, G_out, tau_out, perf_out, times_out};
    o.S = S_out;
    return small_run_many(&h, 1, n_iter, update, &o);
  }
  CHK(ensure_std(h));
  h->std_cur = true; h->small_cur = false;
  if (h->comm && !h->ssys) { set_error("BNMTF over several GPUs needs K, L <= 32 (the dense S system)"); return BNMTF_EINVAL; }
  CHK(ensure_rec(h, (size_t)n_iter));
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  if (mode == kSweepDraw) CHK(stage_gamma_variates(h, n_iter));      // (as bnmf_gibbs_run: the Gamma variates depend on seed and iteration only)
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  Dir& r = h->rows; Dir& c = h->cols;
  const bool acc_used = h->comm != nullptr || !h->use_fast || !c.fast_ok || c.f_gen_count > 0 || !(c.nch == 2 || sweep_fast_supported(c.KP, c.pw));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  SampleSink sink;
  sink.add(r.X, h->I, r.W, r.KP, F_out);
  sink.add(h->S, h->K, h->L, h->L, S_out);
  sink.add(c.X, h->J, c.W, c.KP, G_out);
  CHK(sink.begin(h, n_iter));
  CHK(expectation_begin(h));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));      // finish adds acc to the on-chip sweep's sums: zero unless a sweep used it
  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    // ---- F columns: other = V_eff = G S^T
    enqueue_small_product(h, c, h->ceff, 1);
    enqueue_gemm(h, r, h->ceff, BNMTF_KERNEL_GEMM_ROWS);
    {
      ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_ROWS);
      SweepArgs s = sweep_args(h, r, h->ceff, mode, kStreamRows);
      enqueue_sweep(h, r, h->ceff, s, false);
    }
    if (h->comm) CHK(comm_allgather_factor(h->comm, r.X, r.KP, r.nglob, h->world, h->stream));   // rows of F drawn by their owners
    r.snap_dst = sink.slot_for(it, r.X);         // F's sample goes out with its relayout
    enqueue_post(h, r);
    // ---- S entries, row by row
    {
      ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_S);
      if (h->ssys) {
        CHK(enqueue_ssys_build(h));
        enqueue_ssys_chain(h, update, -1);
      } else {
        enqueue_s_prepare(h);
        for (int k = 0; k < h->K; ++k) enqueue_srow(h, k, update, -1, k > 0);
      }
    }
    // ---- G columns: other = U_eff = F S
    enqueue_small_product(h, r, h->reff, 0);
    // R~^T (F S) = (R~^T F) S: the S step has just formed R~^T F for this very F (slabsS), so the G sweep's contraction is a
    // K x L product per column instead of another pass over R~ (BNMTF_TRI_GEMM_COLS=1: the pass over R~, for comparison)
#ifdef BNMTF_EXPERIMENTS
    static const bool gemm_cols = getenv("BNMTF_TRI_GEMM_COLS") != nullptr;
#else
    constexpr bool gemm_cols = false;
#endif
    if (gemm_cols) enqueue_gemm(h, c, h->reff, BNMTF_KERNEL_GEMM_COLS);
    else {
      ScopedKernelTimer t(h, BNMTF_KERNEL_GEMM_COLS);
      SlabProductArgs sp;
      sp.slabs = h->slabsS; sp.split = c.split; sp.n_pad = c.n_pad; sp.KPin = r.KP; sp.S = h->S; sp.K = h->K; sp.L = h->L; sp.n = c.n; sp.out = c.slabs; sp.KPout = c.KP;
      launch_slab_product(sp, h->stream);
    }
    if (acc_used) HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));    // (the on-chip sweep leaves its sums in c.stats)
    {
      ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_COLS);
      SweepArgs s = sweep_args(h, c, h->reff, mode, kStreamCols);
      s.acc = h->acc;
      if (!gemm_cols) s.split = 1;               // one summed slab
      enqueue_sweep(h, c, h->reff, s, true);
    }
    const bool fast_stats = h->last_sweep_fast;
    if (h->comm) {
      CHK(comm_allgather_factor(h->comm, c.X, c.KP, c.nglob, h->world, h->stream));
      if (fast_stats) launch_sum_stats(c.stats, c.stats_blocks, h->acc, h->stream);   // fold the slab before the exchange
      CHK(comm_allreduce_sum(h->comm, h->acc, 4, h->stream));
    }
    c.snap_dst = sink.slot_for(it, c.X);
    enqueue_post(h, c);
    FinishArgs f;
    f.Cr64 = h->reff.C64; f.Cc64 = c.C64; f.sr = h->reff.colsum; f.sc = c.colsum; f.KP = c.KP;
    f.acc = h->acc; f.stats = (fast_stats && !h->comm) ? c.stats : nullptr; f.nstats = (fast_stats && !h->comm) ? c.stats_blocks : 0;
    f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta; f.update = update;
    f.key0 = (uint32_t)h->seed; f.key1 = (uint32_t)(h->seed >> 32); f.it = (uint32_t)h->iteration;
    f.gunit = mode == kSweepDraw ? h->gunit + it : nullptr;
    f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->rec + (size_t)it * 5;
    f.copy_src = h->S; f.copy_dst = sink.slot_for(it, h->S); f.copy_n = h->K * h->L;       // S's sample rides in this launch (S is final since the S step)
    launch_finish(f, h->stream);
    CHK(sink.close_slot(it));
    expectation_add(h, it);
    heldout_enqueue(h, it, h->stream);
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sink.finish());
  HIPCHK(hipGetLastError());
  drain_events(h);
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 5);
  HIPCHK(hipMemcpy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int it = 0; it < n_iter; ++it) {
    if (tau_out) tau_out[it] = rec[(size_t)it * 5];
    if (perf_out) for (int m = 0; m < 3; ++m) perf_out[(size_t)it * 3 + m] = rec[(size_t)it * 5 + 1 + m];
  }
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// A list of independent tri-factorisations, n_iter iterations each: the ones of the one-launch path that share a device go down
// in ONE grid (kernel_small.hip, a block per model), the others run one after the other (bnmf_gibbs_run_many's contract).
int bnmtf_gibbs_run_many(const bnmtf_handle* hs, int n_models, int n_iter, int update, float* const* F_outs, float* const* S_outs, float* const* G_outs,
                         double* const* tau_outs, double* const* perf_outs, double* const* times_outs,
                         double* const* F_final, double* const* S_final, double* const* G_final, double* const* tau_final) try {
  if (n_models < 0 || n_iter < 0) { set_error("negative count"); return BNMTF_EINVAL; }
  if (n_models == 0 || n_iter == 0) return BNMTF_OK;
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  for (int b = 0; b < n_models; ++b) if (hs[b]->L == 0) { set_error("bnmtf_gibbs_run_many on a BNMF handle (model %d)", b); return BNMTF_ESTATE; }
  for (int b = 0; b < n_models; ++b) CHK(heldout_refuse_many(hs[b], "bnmtf_gibbs_run_many", b));
  auto out_of = [&](int b) {
    SmallOut o{F_outs ? F_outs[b] : nullptr, G_outs ? G_outs[b] : nullptr, tau_outs ? tau_outs[b] : nullptr, perf_outs ? perf_outs[b] : nullptr,
               times_outs ? times_outs[b] : nullptr, F_final ? F_final[b] : nullptr, G_final ? G_final[b] : nullptr, tau_final ? tau_final[b] : nullptr};
    o.S = S_outs ? S_outs[b] : nullptr; o.S_final = S_final ? S_final[b] : nullptr;
    return o;
  };
  std::vector<bnmtf_model*> batch; std::vector<SmallOut> outs;
  std::vector<char> taken(n_models, 0);
  // models on model b's device that actually JOIN the launch, b included: the rule of a CU-filling or wide-rank model depends on
  // the batch size (small_wanted), so the count is taken to its fixed point -- a model that would run alone on the multi-launch
  // path does not make a "batch" for the others (round 5's advice)
  auto peers = [&](int b) {
    int n = 0;
    for (int c = 0; c < n_models; ++c) n += (hs[c]->small && hs[c]->small_mode != 0 && hs[c]->device == hs[b]->device) ? 1 : 0;
    for (int round = 0; round < n_models && n > 0; ++round) {
      int m = 0;
      for (int c = 0; c < n_models; ++c) m += (hs[c]->device == hs[b]->device && small_wanted(hs[c], n)) ? 1 : 0;
      if (m == n) break;
      n = m;
    }
    return n;
  };
  for (int b = 0; b < n_models; ++b) {
    if (taken[b]) continue;
    const int np = peers(b);
    if (!small_wanted(hs[b], np)) {
      const SmallOut o = out_of(b);
      CHK(bnmtf_gibbs_run(hs[b], n_iter, update, o.U, o.S, o.V, o.tau, o.perf, o.times));
      if (o.U_final || o.S_final || o.V_final || o.tau_final) CHK(bnmtf_get_state(hs[b], o.U_final, o.S_final, o.V_final, o.tau_final));
      taken[b] = 1;
      continue;
    }
    batch.clear(); outs.clear();
    for (int c = b; c < n_models; ++c)
      if (!taken[c] && small_wanted(hs[c], np) && hs[c]->device == hs[b]->device) {
        for (bnmtf_model* x : batch) if (x == hs[c]) { set_error("bnmtf_gibbs_run_many: the same handle twice"); return BNMTF_EINVAL; }
        batch.push_back(hs[c]); outs.push_back(out_of(c)); taken[c] = 1;
      }
    CHK(small_run_many(batch.data(), (int)batch.size(), n_iter, update, outs.data()));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// ------------------------------------------------------------------------------- BNMF VB
static int ensure_vb(bnmtf_model* h) {
  CHK(ensure_std(h));                       // (a model that started on the small path: the multi-launch structures first)
  if (h->vb_ready) return BNMTF_OK;
  for (Dir* d : {&h->rows, &h->cols}) {
    const size_t n = (size_t)d->xrows * d->KP;
    CHK(dalloc(&d->mu, n)); CHK(dalloc(&d->tauq, n)); CHK(dalloc(&d->var, n)); CHK(dalloc(&d->S2, n));
    CHK(dalloc(&d->S2T, (size_t)d->KP * d->ldT));
    CHK(dalloc(&d->XS, (size_t)d->KP * d->ldT * 2));
    CHK(dalloc(&d->vb_asq, n)); CHK(dalloc(&d->vb_vsq, n));
    CHK(dalloc(&d->vb_stats, (size_t)std::max(d->n, 1) * 8));
  }
  // the masked sums of the on-chip sweep (kernel_maskgemm.hip): a unit's row of the mask as bits, the other factor's moments
  // as bf16 planes (rows = this direction's padded inner extent), the slabs of the product
  for (int w = 0; w < 2; ++w) {
    Dir& d = w == 0 ? h->rows : h->cols;
    Dir& o = w == 0 ? h->cols : h->rows;
    if (!h->Mtrain || d.n_pad <= 0 || d.inner_pad <= 0) continue;
    const int ldw = d.inner_pad / 32;
    CHK(dalloc(&d.mbits, (size_t)d.n_pad * ldw, false));
    launch_mask_bits(h->Mtrain, h->I, h->J, w == 0 ? 1 : 0, d.n0, d.n, o.nglob, d.n_pad, ldw, d.mbits, h->stream);
    o.xb_rows = d.inner_pad;
    CHK(dalloc(&o.XB, (size_t)3 * (d.inner_pad / 16) * (2 * o.KP) * 4, false));
    CHK(dalloc(&o.xb_umax, (size_t)2 * o.KP)); CHK(dalloc(&o.xb_cexp, (size_t)2 * o.KP));
    CHK(dalloc(&o.xb_mpart, (size_t)post_blocks(o.nglob) * 2 * o.KP));
    // inner slices of the masked product: as many (a power of two, at most 8) as keep the grid within one block per CU
    // (four slices and slabs at 8192^2, K = 64)
    {
      const int ugpb = 4 / (2 * d.KP / 32), nxb = (d.n_pad / 128 + ugpb - 1) / ugpb;       // blocks per inner slice
      d.msplit = 1;
      while (d.msplit < 8 && nxb * d.msplit * 2 <= 256 && d.inner_pad % (32 * d.msplit * 2) == 0) d.msplit *= 2;
      d.mipw = d.inner_pad / d.msplit;                 // inner rows of a block's slice
    }
    CHK(dalloc(&d.mslabs, (size_t)d.msplit * d.n_pad * 2 * d.KP, false));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  CHK(dalloc(&h->A2d, (size_t)h->I * 64)); CHK(dalloc(&h->B2d, (size_t)h->J * 64));
  CHK(dalloc(&h->vbred, 24));
  h->vb_ready = true;
  return BNMTF_OK;
}
static int upload_plain(bnmtf_model* h, Dir& d, float* dev, const double* src) {
  std::vector<float> tmp((size_t)d.nglob * d.KP, 0.0f);
  for (int r = 0; r < d.nglob; ++r)
    for (int k = 0; k < d.W; ++k) tmp[(size_t)r * d.KP + k] = (float)src[(size_t)r * d.W + k];
  HIPCHK(hipMemcpyAsync(dev, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}
static int vb_upload_dir(bnmtf_model* h, Dir& d, const double* mu, const double* tauq, const double* ex, const double* var) {
  if (mu) CHK(upload_plain(h, d, d.mu, mu));
  if (tauq) CHK(upload_plain(h, d, d.tauq, tauq));
  if (var) CHK(upload_plain(h, d, d.var, var));
  if (ex) CHK(upload_plain(h, d, d.X, ex));
  if (ex || var) {                                      // S2 = var + exp^2 from the device copies
    std::vector<float> e((size_t)d.nglob * d.KP), v((size_t)d.nglob * d.KP);
    HIPCHK(hipMemcpy(e.data(), d.X, e.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v.data(), d.var, v.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < e.size(); ++t) v[t] = v[t] + e[t] * e[t];
    HIPCHK(hipMemcpy(d.S2, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  enqueue_post(h, d, true);
  return BNMTF_OK;
}
static SweepArgs vb_sweep_args(bnmtf_model* h, Dir& d, Dir& o, uint32_t stream_id) {
  SweepArgs s = sweep_args(h, d, o, kSweepVB, stream_id);
  s.vb_stats = d.vb_stats;
  if (g_recorder) s.it = 0;            // (the variational kernels draw nothing; a recorded argument list that does not change is not uploaded again)
  return s;
}
// One full VB half sweep (every column, moments refreshed).  Fast path: the 16-wave kernel + the ELBO-pieces pass, when
// the direction's slot layout allows it; otherwise the generic kernel.  want_acc: the three SSE-identity sums -> h->acc.
// want_acc: the three SSE-identity sums -> h->acc, or -- stats_blocks given and the on-chip kernels run -- left as d.stats'
// *stats_blocks per-block rows for the end-of-iteration kernel to fold (0: everything is in h->acc)
static void enqueue_vb_sweep(bnmtf_model* h, Dir& d, Dir& o, uint32_t stream_id, bool want_acc, int* stats_blocks = nullptr) {
  if (stats_blocks) *stats_blocks = 0;
  SweepArgs s = vb_sweep_args(h, d, o, stream_id);
  const bool fast = h->use_fast && d.fast_ok && d.wide_can && d.pair_ok && d.f_gen_count == 0 && sweep_vb_supported(d.KP, d.pw) &&
                    (g_recorder || !getenv("BNMTF_VB_GENERIC"));      // (recording: vb_batchable has looked)
  h->last_vb_path = !fast ? 1 : 2;
  if (!fast) {
    if (want_acc) s.acc = h->acc;
    launch_sweep(s, h->stream);
    d.vb_stat_rows = d.n;                       // one row of pieces per unit
    return;
  }
  FastArgs f{};
  memset(&f, 0, sizeof(f));
  f.unit_map = d.f_unit_map; f.pair_E = d.f_pair_E; f.pair_base = d.f_pair_base; f.off = d.f_off; f.off16 = d.f_off16;
  f.npairs = d.f_npairs; f.mz = d.mz; f.pw = d.pw; f.nw = d.use_wide ? 16 : 8;      // VB block shape: 16 unit waves when that fills the chip (same rule as the Gibbs sweep)
  f.XoT = o.XT; f.ldT_o = o.ldT; f.XoT2 = o.XT2; f.ld2_o = o.ldT; f.XoS = o.XS;
  f.vb_asq = d.vb_asq; f.vb_vsq = d.vb_vsq;
  f.stats = want_acc ? d.stats : nullptr;
  // Round 4: the on-chip kernels of the Gibbs sweep run the variational update too (sweep_chip.inc, MODE = kSweepVB), once the
  // two chain-independent masked sums of every (unit, column) are there: sum_miss S2other and sum_miss Eother^2 as ONE product
  // of the mask's bits with the other factor's moments on the matrix cores (kernel_maskgemm.hip).  Otherwise (vb_chip_ok: small
  // ranks, BNMTF_VB_PATH=pairs) the round-1 kernel that gathers (E, S2) pair panels and forms both sums inside the column loop
  // (kernel_sweep_vb.hip).
  const bool chip = vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows);      // (both directions, or the pair panels are kept up to date for the other)
  if (chip) {
    h->last_vb_path = 3;
    // (the column maxima: left by the relayout of o -- its Gram blocks see every row --, or taken by a pass of their own)
    launch_vb_planes(o.S2, o.X, o.nglob, o.xb_rows, o.KP, o.xb_umax, o.xb_umax_posted, o.xb_cexp, o.XB, h->stream);
    MaskGemmArgs mg;
    mg.bits = d.mbits; mg.ldw = d.inner_pad / 32; mg.XB = o.XB; mg.rows_pad = o.xb_rows; mg.cexp = o.xb_cexp; mg.slabs = d.mslabs;
    mg.n_pad = d.n_pad; mg.split = d.msplit; mg.inner_per_wave = d.mipw;
    launch_maskgemm(mg, d.KP, h->stream);
    f.mslabs = d.mslabs; f.msplit = d.msplit;
    f.nch = 1; f.mh = 0; f.pw1 = 0; f.twin = 0;
    set_handover(h, d, o, f, f.nw == d.ho_ppb);
    if (f.nw == 16) launch_sweep_wide(s, f, h->stream); else launch_sweep_fast(s, f, h->stream);
    launch_vb_pieces_slabs(d.n, d.n0, d.KP, d.W, d.mu, d.tauq, d.X, d.var, d.lambda, d.mslabs, d.msplit, d.n_pad, d.vb_stats, h->stream);
    d.vb_stat_rows = (d.n + 3) / 4;
    if (want_acc) {
      if (stats_blocks) *stats_blocks = (d.f_npairs + f.nw - 1) / f.nw;
      else launch_sum_stats(d.stats, (d.f_npairs + f.nw - 1) / f.nw, h->acc, h->stream);
    }
    return;
  }
  set_handover(h, d, o, f, f.nw == 16 && d.ho_ppb == 16);
  launch_sweep_vb(s, f, h->stream);
  launch_vb_pieces(d.n, d.n0, d.KP, d.W, d.mu, d.tauq, d.X, d.var, d.lambda, d.vb_asq, d.vb_vsq, d.vb_stats, h->stream);
  d.vb_stat_rows = (d.n + 3) / 4;             // one row per block of four units
  if (want_acc) {
    if (stats_blocks) *stats_blocks = sweep_vb_blocks(d.f_npairs, f.nw);
    else launch_sum_stats(d.stats, sweep_vb_blocks(d.f_npairs, f.nw), h->acc, h->stream);
  }
}
static int vb_esd_direct(bnmtf_model* h, double* out, double* terms = nullptr) {
  const int I = h->I, J = h->J, K = h->K;
  // metric_kernel's second-moment pass is one load of 32 x K into tiles of 64 columns (not chunked like its first product), and
  // Ad / Bd / A2d / B2d hold 64 columns: a handle is at most BNMTF_MAX_RANK = 64 wide (bnmtf_create), wider models are column blocks
  if (K > 64) { set_error("exp_square_diff: a handle of %d columns (the second-moment pass holds 64; wider models run as column blocks)", K); return BNMTF_EINVAL; }
  std::vector<double> a((size_t)I * K), b((size_t)J * K), a2((size_t)I * K), b2((size_t)J * K);
  CHK(download_matrix(h, h->rows.X, I, K, h->rows.KP, a.data()));
  CHK(download_matrix(h, h->cols.X, J, K, h->cols.KP, b.data()));
  CHK(download_matrix(h, h->rows.S2, I, K, h->rows.KP, a2.data()));
  CHK(download_matrix(h, h->cols.S2, J, K, h->cols.KP, b2.data()));
  HIPCHK(hipMemcpyAsync(h->Ad, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->Bd, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->A2d, a2.data(), a2.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->B2d, b2.data(), b2.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  MetricArgs m;
  m.R = h->Rfull; m.Mp = h->Mtrain; m.I = I; m.J = J; m.A = h->Ad; m.B = h->Bd; m.K = K; m.A2 = h->A2d; m.B2 = h->B2d; m.out6 = h->out6;
  CHK(metric_partials(h, &m.part));
  launch_metric_sums(m, h->stream);
  double s[8];
  HIPCHK(hipMemcpyAsync(s, h->out6, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  *out = (s[2] - 2.0 * s[5] + s[4]) + s[6];
  if (terms) { terms[0] = s[2] - 2.0 * s[5] + s[4]; terms[1] = s[6]; }
  return BNMTF_OK;
}

int bnmf_vb_set_state(bnmtf_handle h, const double* muU, const double* tauU, const double* expU, const double* varU,
                      const double* muV, const double* tauV, const double* expV, const double* varV, double exptau) try {
  if (h->L != 0) { set_error("VB is defined for BNMF handles"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_vb(h));
  CHK(vb_upload_dir(h, h->rows, muU, tauU, expU, varU));
  CHK(vb_upload_dir(h, h->cols, muV, tauV, expV, varV));
  CHK(set_tau(h, exptau));
  h->have_state = true;
  h->ho_regions_current = false;          // (q hand-over: whatever the regions hold belongs to the state that was just replaced)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vb_get_state(bnmtf_handle h, double* muU, double* tauU, double* expU, double* varU,
                      double* muV, double* tauV, double* expV, double* varV) try {
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  Dir& r = h->rows; Dir& c = h->cols;
  if (muU) CHK(download_matrix(h, r.mu, h->I, r.W, r.KP, muU));
  if (tauU) CHK(download_matrix(h, r.tauq, h->I, r.W, r.KP, tauU));
  if (expU) CHK(download_matrix(h, r.X, h->I, r.W, r.KP, expU));
  if (varU) CHK(download_matrix(h, r.var, h->I, r.W, r.KP, varU));
  if (muV) CHK(download_matrix(h, c.mu, h->J, c.W, c.KP, muV));
  if (tauV) CHK(download_matrix(h, c.tauq, h->J, c.W, c.KP, tauV));
  if (expV) CHK(download_matrix(h, c.X, h->J, c.W, c.KP, expV));
  if (varV) CHK(download_matrix(h, c.var, h->J, c.W, c.KP, varV));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vb_update(bnmtf_handle h, int which, int k, int moments) try {
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  if (k < 0 || k >= d.W) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  if (h->world != 1) { set_error("update_U(k) / update_V(k) are single-GPU hooks (a sharded model updates through run())"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  enqueue_gemm(h, d, o, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
  SweepArgs s = vb_sweep_args(h, d, o, which == 0 ? kStreamRows : kStreamCols);
  s.only_k = k; s.vb_moments = moments ? 1 : 0; s.vb_stats = nullptr;
  launch_sweep(s, h->stream);
  enqueue_post(h, d, true);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vb_exp_square_diff(bnmtf_handle h, double* out) try {
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return vb_esd_direct(h, out);
} BNMTF_ABI_GUARD

// exp_square_diff() in its two parts: {sum_Omega (R - E[U] E[V]^T)^2, sum_Omega sum_k [(varU+expU^2)(varV+expV^2) - expU^2 expV^2]}.
// The second part is a sum over the columns, i.e. additive over the column blocks of a model wider than 64 (_blocked.py).
int bnmf_vb_esd_terms(bnmtf_handle h, double out[2]) try {
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  double esd = 0.0;
  CHK(vb_esd_direct(h, &esd, out));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// one half of a VB iteration (bnmf_vb_optimised.py:134-141): update_U(k) + update_exp_U(k) for every k (which = 0) or the same
// for V, with the handle's current exptau; contraction, sweep, relayout + Gram.  update_tau / update_exp_tau, the metrics and the
// ELBO are the caller's (a column-blocked model: bnmtf_amd/_blocked.py).
int bnmf_vb_half_sweep(bnmtf_handle h, int which) try {
  if (!h->vb_ready || !h->have_state) { set_error("bnmf_vb_half_sweep before bnmf_vb_set_state"); return BNMTF_ESTATE; }
  if (which < 0 || which > 1) { set_error("which = 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  if (h->comm) { set_error("bnmf_vb_half_sweep: one GPU"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  h->ho_active = false;
  h->rows.ho_filled = h->cols.ho_filled = false;
  enqueue_gemm(h, d, o, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  enqueue_vb_sweep(h, d, o, which == 0 ? kStreamRows : kStreamCols, false);
  enqueue_post(h, d, true);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vb_masked_sums(bnmtf_handle h, int which, double* asq, double* vsq) try {
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  if (which != 0 && which != 1) { set_error("which = 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  if (!(d.mbits && o.XB && d.mslabs)) { set_error("this model has no masked-sum operands (no mask on the device)"); return BNMTF_ESTATE; }
  launch_vb_planes(o.S2, o.X, o.nglob, o.xb_rows, o.KP, o.xb_umax, false, o.xb_cexp, o.XB, h->stream);      // (the maxima by a pass of their own: whatever path the relayout took)
  o.xb_umax_posted = false;
  MaskGemmArgs mg;
  mg.bits = d.mbits; mg.ldw = d.inner_pad / 32; mg.XB = o.XB; mg.rows_pad = o.xb_rows; mg.cexp = o.xb_cexp; mg.slabs = d.mslabs;
  mg.n_pad = d.n_pad; mg.split = d.msplit; mg.inner_per_wave = d.mipw;
  launch_maskgemm(mg, d.KP, h->stream);
  const size_t slab = (size_t)d.n_pad * 2 * d.KP;
  std::vector<float> hs((size_t)d.msplit * slab);
  HIPCHK(hipMemcpyAsync(hs.data(), d.mslabs, hs.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < d.W; ++k) {
      float a = 0.f, v = 0.f;                        // slabs added in slab order, in fp32: as the sweep's prologue adds them
      for (int sl = 0; sl < d.msplit; ++sl) { a += hs[sl * slab + (size_t)u * 2 * d.KP + k]; v += hs[sl * slab + (size_t)u * 2 * d.KP + d.KP + k]; }
      if (asq) asq[(size_t)u * d.W + k] = (double)a;
      if (vsq) vsq[(size_t)u * d.W + k] = (double)v;
    }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// Hook (tests), read-only: the column maxima of [S2 | E^2] of one FACTOR (which = 0: U, 1: V) -- the fixed-point grid of the
// masked product's digit planes -- as the factor's last relayout left them (xb_umax, *was_posted = xb_umax_posted: gram_reduce_kernel's
// maxima block) and by a pass of vb_colmax_kernel into a scratch buffer.  The model's maxima and their flag stay as they are; the
// pass goes through launch_vb_planes, whose other outputs (the digit planes and their exponents) are derived data that every
// product rebuilds ahead of its launch.
int bnmf_vb_column_maxima(bnmtf_handle h, int which, uint32_t* posted, uint32_t* own, int* was_posted) try {
  CHK(refuse_obs(h, "bnmf_vb_column_maxima"));
  if (!h->vb_ready || !h->have_state) { set_error("no VB state set"); return BNMTF_ESTATE; }
  if (which != 0 && which != 1) { set_error("which = 0 (the factor U) or 1 (V)"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  Dir& o = which == 0 ? h->rows : h->cols;
  if (!(o.XB && o.xb_umax && o.xb_cexp)) { set_error("this model has no masked-sum operands (no mask on the device)"); return BNMTF_ESTATE; }
  const size_t ncol = (size_t)2 * o.KP;
  if (posted) HIPCHK(hipMemcpyAsync(posted, o.xb_umax, ncol * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (own) {
    DevBuf<unsigned> scratch;
    CHK(scratch.alloc(ncol));
    launch_vb_planes(o.S2, o.X, o.nglob, o.xb_rows, o.KP, scratch.p, false, o.xb_cexp, o.XB, h->stream);
    HIPCHK(hipMemcpyAsync(own, scratch.p, ncol * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));            // (before the scratch buffer goes)
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if (was_posted) *was_posted = o.xb_umax_posted ? 1 : 0;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// One variational iteration (bnmf_vb_optimised.py:121-153 + :181-187) of a model on h->stream -- or, while a Recorder is installed
// (many.h; api_many.inc: the caller has checked vb_batchable), into its records: `recording` leaves the record's index to the
// list-form end-of-iteration kernel.
static int enqueue_vb_iteration(bnmtf_model* h, int it, bool recording) {
  Dir& r = h->rows; Dir& c = h->cols;
  enqueue_gemm(h, r, c, BNMTF_KERNEL_GEMM_ROWS);
  { ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_ROWS); enqueue_vb_sweep(h, r, c, kStreamRows, false); }
  if (h->comm) {   // the other direction's panels are built from (E, S2) of every row: gather the owners' blocks
    CHK(comm_allgather_factor(h->comm, r.X, r.KP, r.nglob, h->world, h->stream));
    CHK(comm_allgather_factor(h->comm, r.S2, r.KP, r.nglob, h->world, h->stream));
  }
  enqueue_post(h, r, true);
  enqueue_gemm(h, c, r, BNMTF_KERNEL_GEMM_COLS);
  // (acc: written by the generic sweep's atomics only -- the on-chip kernels leave per-block sums for the end-of-iteration kernel; it
  // is zeroed once before the loop and again behind an iteration that used it)
  int sweep_blocks = 0;
  { ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_COLS); enqueue_vb_sweep(h, c, r, kStreamCols, true, h->comm ? nullptr : &sweep_blocks); }
  VbFinishArgs f;
  memset(&f, 0, sizeof(f));                              // (padding too: a recorded list compares argument bytes)
  f.extra = nullptr; f.n_extra = 0;
  f.sweep_stats = sweep_blocks > 0 ? c.stats : nullptr; f.n_sweep_stats = sweep_blocks;
  f.acc = h->acc; f.stats_r = r.vb_stats; f.nr = r.vb_stat_rows; f.stats_c = c.vb_stats; f.nc = c.vb_stat_rows;
  if (h->comm) {
    CHK(comm_allgather_factor(h->comm, c.X, c.KP, c.nglob, h->world, h->stream));
    CHK(comm_allgather_factor(h->comm, c.S2, c.KP, c.nglob, h->world, h->stream));
    // every per-unit / per-block sum of the two sweeps folded into 20 doubles and exchanged once:
    // [0..2] the SSE-identity sums, [4..9] the six ELBO / exp_square_diff pieces of the rows, [12..17] of the columns
    HIPCHK(hipMemsetAsync(h->vbred, 0, 24 * sizeof(double), h->stream));
    launch_sum_cols(h->acc, 1, 4, 3, h->vbred, h->stream);
    launch_sum_cols(r.vb_stats, r.vb_stat_rows, 8, 6, h->vbred + 4, h->stream);
    launch_sum_cols(c.vb_stats, c.vb_stat_rows, 8, 6, h->vbred + 12, h->stream);
    CHK(comm_allreduce_sum(h->comm, h->vbred, 20, h->stream));
    f.acc = h->vbred; f.stats_r = h->vbred + 4; f.nr = 1; f.stats_c = h->vbred + 12; f.nc = 1;
  }
  enqueue_post(h, c, true);
  f.Cr64 = r.C64; f.Cc64 = c.C64; f.sr = r.colsum; f.sc = c.colsum; f.s2r = r.colsum2; f.s2c = c.colsum2; f.KP = r.KP;
  f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
  f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = recording ? h->vb_rec : h->vb_rec + (size_t)it * 16;
  if (recording && (sweep_blocks == 0 || !g_recorder)) { set_error("a recorded variational iteration left the list-form kernels"); return BNMTF_ESTATE; }
  launch_vb_finish(f, h->stream);
  if (sweep_blocks == 0) HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));       // (used: clean for the next iteration)
  h->iteration++;
  return BNMTF_OK;
}

int bnmf_vb_run(bnmtf_handle h, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out) try {
  if (!h->vb_ready || !h->have_state) { set_error("bnmf_vb_run before bnmf_vb_set_state"); return BNMTF_ESTATE; }
  if (n_iter <= 0) return n_iter == 0 ? BNMTF_OK : BNMTF_EINVAL;
  HIPCHK(hipSetDevice(h->device));
  Dir& r = h->rows; Dir& c = h->cols;
  CHK(vb_reserve_rec(h, n_iter));
  CHK(heldout_begin(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  HandoverScope ho_scope{h};
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(enqueue_vb_iteration(h, it, false));
    heldout_enqueue(h, it, h->stream);           // (a mask set: on E[U], E[V] of this iteration)
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
  }
  if (h->comm)      // q(U), q(V) parameters of the other ranks' rows (bnmf_vb_get_state returns whole matrices)
    for (Dir* d : {&r, &c})
      for (float* X : {d->mu, d->tauq, d->var}) CHK(comm_allgather_factor(h->comm, X, d->KP, d->nglob, h->world, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  ho_scope.commit();
  drain_events(h);
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 16);
  HIPCHK(hipMemcpy(rec.data(), h->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_vb_rec(rec.data(), n_iter, exptau_out, perf_out, elbo_terms_out);
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
