// Variational tri-factorisation driver (C ABI part 3, bnmtf_vb_optimised.py) -- included at the end of api.hip.
// Device state: q(F) in rows.{mu, tauq, X = E, var, S2}, q(G) in cols.*, q(S) in {muS, tauS, S = E, varS}; the F and G
// updates run the BNMF-VB sweep against the effective factors (ceff / reff hold mean and second moment), the S entries
// run on the dense second-moment system of kernel_ssys.hip.  K, L <= 32, single GPU.

namespace bnmtf {

// The launch sites of a recorded iteration (many.h: site_at; api_many.inc): the records of the models of a batch are aligned by
// site, not by position -- a model's first iteration of a call forms R~^T E[F] and the column Grams inside the S system (later ones
// take them from behind the F sweep), and only K L >= 64 permutes the system for the chain.
enum TriSite {
  kTsPv, kTsColGram, kTsGammaPack, kTsSysGemm, kTsSysReduce, kTsSysB, kTsResidual, kTsColsumRows, kTsGemmRows, kTsPermute, kTsChain,
  kTsProductF, kTsSlabF, kTsSweepF, kTsPostF, kTsColGramsNext, kTsPvNext, kTsProductG, kTsSlabG, kTsSweepG, kTsPostG, kTsThird,
  kTsFinish
};

static int ensure_tri(bnmtf_model* h) {
  if (h->tri_ready) return BNMTF_OK;
  if (h->L == 0) { set_error("the tri-factorisation VB calls need a BNMTF handle (L > 0)"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_std(h));                        // (a model that started on the one-launch path: the multi-launch structures, the S system among them)
  if (!h->ssys) { set_error("bnmtf_vb needs K, L <= 32 (dense S system)"); return BNMTF_EINVAL; }
  CHK(ensure_vb(h));
  for (Dir* d : {&h->reff, &h->ceff}) {                 // effective factors carry a second moment too
    const size_t n = (size_t)d->xrows * d->KP;
    CHK(dalloc(&d->S2, n)); CHK(dalloc(&d->S2T, (size_t)d->KP * d->ldT)); CHK(dalloc(&d->XS, (size_t)d->KP * d->ldT * 2));
  }
  const size_t n2 = (size_t)h->K * h->L;
  CHK(dalloc(&h->muS, n2)); CHK(dalloc(&h->tauS, n2)); CHK(dalloc(&h->varS, n2));
  CHK(dalloc(&h->mv_rows, (size_t)std::max(h->rows.n, 1) * 32)); CHK(dalloc(&h->mv_cols, (size_t)std::max(h->cols.n, 1) * 32));
  CHK(dalloc(&h->tri_sums, 24));
  CHK(dalloc(&h->tri_third, (size_t)std::max(tri_third_blocks(h->cols.n), 1)));
  CHK(dalloc(&h->ss_Aperm, n2 * n2));
  h->tri_ready = true;
  return BNMTF_OK;
}

// second-moment S system for the current q(F), q(G): A~ (with the var terms), b, and r = b - A~ E[S]
// Behind the F sweep (q(F) final for this iteration): the masked column Grams W~_j of the NEXT S system -- a function of q(F) alone --
// and, out of the same gathers, the masked variance sums of F the G sweep's covariance term reads (mv_cols: the kernel's sum over
// the missing rows IS masked_colsum_kernel's).  One pass over the missing entries' rows of (E[F], varF) instead of two (round 6).
static void enqueue_tri_colgrams(bnmtf_model* h) {
  Dir& c = h->cols; Dir& r = h->rows;
  SColGramArgs w;
  memset(&w, 0, sizeof(w));                              // (padding too: a recorded list compares argument bytes)
  w.n = c.n; w.K = h->K; w.F = r.X; w.varF = r.var; w.Cf64 = r.C64; w.cf_diag_extra = r.colsum2;
  w.slot_ptr = c.slot_ptr; w.idx = c.idx; w.Wc = h->ss_Wc; w.var_obs_out = h->mv_cols;
  GammaPackArgs gp;
  memset(&gp, 0, sizeof(gp));
  gp.n = 0; gp.n0 = c.n0; gp.L = h->L; gp.G = c.X; gp.varG = c.var; gp.Gc = h->ss_Gc;
  launch_scol_gram(w, gp, h->stream);
  h->tri_w_current = h->tri_mv_cols_current = true;
}
static void enqueue_tri_pv(bnmtf_model* h) {        // slabsS = R~^T E[F]
  Dir& c = h->cols; Dir& r = h->rows;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.big = c.big; g.ld = c.n_pad; g.X = r.X; g.slabs = h->slabsS; g.n_pad = c.n_pad; g.split = c.split; g.inner_per_wave = c.ipw; g.tw = c.gemm_tw;
  launch_gemm(g, r.KP, h->stream);
}
static int enqueue_tri_ssys(bnmtf_model* h, bool pv_current = false) {
  Dir& c = h->cols; Dir& r = h->rows;
  const int K = h->K, L = h->L, n2 = K * L;
  if (!pv_current) {
    site_at(kTsPv);
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.big = c.big; g.ld = c.n_pad; g.X = r.X; g.slabs = h->slabsS; g.n_pad = c.n_pad; g.split = c.split; g.inner_per_wave = c.ipw; g.tw = c.gemm_tw;
    launch_gemm(g, r.KP, h->stream);                       // Pv = R~^T E[F]
  }
  GammaPackArgs gp;                                         // E[G_jl G_jl'] = E[G_jl] E[G_jl'] + [l = l'] varG_jl
  memset(&gp, 0, sizeof(gp));
  gp.n = c.n; gp.n0 = c.n0; gp.L = L; gp.G = c.X; gp.varG = c.var; gp.Gc = h->ss_Gc;
  if (h->tri_w_current) {
    site_at(kTsGammaPack);
    launch_gamma_pack(gp, h->stream);    // (the column Grams of this q(F) were formed behind its sweep: enqueue_tri_colgrams)
  } else {
    site_at(kTsColGram);
    SColGramArgs w;
    memset(&w, 0, sizeof(w));
    w.n = c.n; w.K = K; w.F = r.X; w.varF = r.var; w.Cf64 = r.C64;
    w.cf_diag_extra = r.colsum2;                            // C~f_kk = sum_i (E[F_ik]^2 + varF_ik): the column sums of the second moments
    w.slot_ptr = c.slot_ptr; w.idx = c.idx; w.Wc = h->ss_Wc;
    if (h->tri_mv_cols_current) { w.varF = nullptr; w.var_obs = h->mv_cols; }    // (the masked variance sums of this q(F) are there: no second gather)
    launch_scol_gram(w, gp, h->stream);
  }
  SSysGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.n = c.n; g.K = K; g.L = L; g.nsplit = h->ss_nsplit; g.Wc = h->ss_Wc; g.Gc = h->ss_Gc; g.slabs = h->ss_slabs;
  site_at(kTsSysGemm);
  launch_ssys_gemm(g, h->stream);
  site_at(kTsSysReduce);
  launch_ssys_reduce(h->ss_slabs, h->ss_nsplit, K, L, h->ss_AB, h->stream);
  SSysBArgs b;
  memset(&b, 0, sizeof(b));
  b.n = c.n; b.n0 = c.n0; b.K = K; b.L = L; b.slabs = h->slabsS; b.split = c.split; b.n_pad = c.n_pad; b.G = c.X; b.b = h->ss_bpart;
  site_at(kTsSysB);
  launch_ssys_b(b, h->stream);
  if (h->comm) {
    // several GPUs: (A~, b) of the ranks' column ranges summed with ONE all-reduce (the "K x L Gram" exchange, as bnmtf_gibbs_run's S step)
    launch_ssys_sum_parts(h->ss_bpart, ssys_b_blocks(c.n), (size_t)n2, h->ss_AB + (size_t)n2 * n2, h->stream);
    CHK(comm_allreduce_sum_f32(h->comm, h->ss_AB, n2 * n2 + n2, h->stream));
  }
  site_at(kTsResidual);
  launch_ssys_residual(h->ss_AB, h->ss_AB + (size_t)n2 * n2, h->comm ? nullptr : h->ss_bpart, ssys_b_blocks(c.n), h->S, n2, h->ss_r, h->stream);
  return BNMTF_OK;
}
// order_step (recording): order_dev is the order of the call's first iteration, the list forms add it x order_step
static void enqueue_tri_chain(bnmtf_model* h, const int* order_dev, int n_order, int only_params, int order_step = 0) {
  SSysChainVbArgs a;
  memset(&a, 0, sizeof(a));
  a.K = h->K; a.L = h->L; a.n_order = n_order; a.only_params = only_params; a.order = order_dev;
  a.A = h->ss_AB; a.r0 = h->ss_r; a.lambdaS = h->lambdaS; a.tau = h->tau_f;
  a.E = h->S; a.var = h->varS; a.mu = h->muS; a.tauq = h->tauS;
  a.Aperm = nullptr;
  if (n_order == h->K * h->L && !only_params && n_order >= 64 && h->ss_Aperm) {      // a whole pass: the system in the pass's order
    site_at(kTsPermute);
    launch_ssys_permute(h->ss_AB, order_dev, n_order, h->ss_Aperm, h->stream, order_step);
    a.Aperm = h->ss_Aperm;
  }
  site_at(kTsChain);
  launch_ssys_chain_vb(a, h->stream, order_step);
}

// everything update_F (which = 0) / update_G (which = 2) needs before its sweep: effective factor (mean, second moment,
// panels, Gram), the masked variance sums of the other factor, the contraction
static void enqueue_tri_masked_colsum(bnmtf_model* h, int which, hipStream_t st) {
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& o = which == 0 ? h->cols : h->rows;
  MaskedColsumArgs m;
  memset(&m, 0, sizeof(m));
  m.n = d.n; m.slot_ptr = d.slot_ptr; m.idx = d.idx; m.V = o.var; m.colsum2 = o.colsum2; m.C64 = o.C64;
  m.out = which == 0 ? h->mv_rows : h->mv_cols;
  launch_masked_colsum(m, st);
}
// pieces: 1 effective factor (+ its relayout and Gram), 2 masked variance sums, 4 the contraction against the effective factor
static void enqueue_tri_side_prepare(bnmtf_model* h, int which, int pieces = 7) {
  Dir& d = which == 0 ? h->rows : h->cols;      // factor being updated
  Dir& o = which == 0 ? h->cols : h->rows;      // the other observed-side factor
  Dir& e = which == 0 ? h->ceff : h->reff;      // effective factor built from o and S
  if (pieces & 1) {
    SmallProductVbArgs p;
    memset(&p, 0, sizeof(p));
    p.X = o.X; p.varX = o.var; p.rows = o.nglob; p.S = h->S; p.varS = h->varS; p.K = h->K; p.L = h->L;
    p.transposeS = which == 0 ? 1 : 0; p.out = e.X; p.outS2 = e.S2;
    launch_small_product_vb(p, h->stream);
    enqueue_post(h, e, true);
  }
  if (pieces & 2) enqueue_tri_masked_colsum(h, which, h->stream);
  if (pieces & 4) enqueue_gemm(h, d, e, which == 0 ? BNMTF_KERNEL_GEMM_ROWS : BNMTF_KERNEL_GEMM_COLS);
}
static SweepArgs tri_sweep_args(bnmtf_model* h, int which, const int* order_dev) {
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& e = which == 0 ? h->ceff : h->reff;
  SweepArgs s = vb_sweep_args(h, d, e, which == 0 ? kStreamRows : kStreamCols);
  s.cov_S = h->S; s.cov_mv = which == 0 ? h->mv_rows : h->mv_cols; s.order = order_dev;
  if (which == 0) { s.cov_sc = h->L; s.cov_st = 1; s.cov_n = h->L; }       // column k of F, inner l: S[k][l]
  else            { s.cov_sc = 1; s.cov_st = h->L; s.cov_n = h->K; }       // column l of G, inner k: S[k][l]
  return s;
}

// One full F (which = 0) or G (which = 2) half sweep in the order handed over, moments refreshed, ELBO pieces behind it
// (d.vb_stats, d.vb_stat_rows rows).  Round 6: on the on-chip pair-panel kernel of the BNMF-VB sweep (kernel_sweep_vb.hip, COV)
// when the direction's slot layout allows it -- the generic kernel (one wave per unit, q in global memory) was 484 us per half
// sweep at 4096^2, K = L = 32.  want_acc: the three sums of the SSE identity -> h->acc (zeroed by the caller).
// order_step (recording): order_dev is the column order of the call's first iteration, the list form adds it x order_step
static void enqueue_tri_sweep(bnmtf_model* h, int which, const int* order_dev, bool want_acc, bool one_slab = false, int* stats_blocks = nullptr,
                              int order_step = 0) {
  if (stats_blocks) *stats_blocks = 0;
  Dir& d = which == 0 ? h->rows : h->cols;
  Dir& e = which == 0 ? h->ceff : h->reff;
  SweepArgs s = tri_sweep_args(h, which, order_dev);
  if (one_slab) s.split = 1;                  // (the contraction came as a product of slabs with S: one summed slab)
  // (BNMTF_VB_PATH=masked: the relayout leaves the (E, S2) pair panels out -- api.hip enqueue_post)
  const bool masked = vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows);
  const bool fast = h->use_fast && d.fast_ok && d.wide_can && d.pair_ok && d.f_gen_count == 0 && sweep_vb_cov_supported(d.KP, d.pw) &&
                    e.XS && e.XT2 && !masked && !getenv("BNMTF_VB_GENERIC");
  h->last_tri_path = fast ? 2 : 1;
  if (!fast) {
    if (want_acc) s.acc = h->acc;
    launch_sweep(s, h->stream);
    d.vb_stat_rows = d.n;
    return;
  }
  FastArgs f;
  memset(&f, 0, sizeof(f));
  f.unit_map = d.f_unit_map; f.pair_E = d.f_pair_E; f.pair_base = d.f_pair_base; f.off = d.f_off; f.off16 = d.f_off16;
  f.npairs = d.f_npairs; f.mz = d.mz; f.pw = d.pw; f.nw = d.use_wide ? 16 : 8;
  f.XoT = e.XT; f.ldT_o = e.ldT; f.XoT2 = e.XT2; f.ld2_o = e.ldT; f.XoS = e.XS;
  f.vb_asq = d.vb_asq; f.vb_vsq = d.vb_vsq;
  f.stats = want_acc ? d.stats : nullptr;
  f.nch = 1; f.ho_rows_total = (int)d.f_slots;      // (no q hand-over: S changes between the G sweep and the next F sweep)
  launch_sweep_vb(s, f, h->stream, order_step);
  launch_vb_pieces(d.n, d.n0, d.KP, d.W, d.mu, d.tauq, d.X, d.var, d.lambda, d.vb_asq, d.vb_vsq, d.vb_stats, h->stream);
  d.vb_stat_rows = (d.n + 3) / 4;
  if (want_acc) {
    if (stats_blocks) *stats_blocks = sweep_vb_blocks(d.f_npairs, f.nw);      // (folded by the end-of-iteration kernel)
    else launch_sum_stats(d.stats, sweep_vb_blocks(d.f_npairs, f.nw), h->acc, h->stream);
  }
}

// exp_square_diff and the training-mask sums: three direct fp64 passes (tri_factors_kernel lays out the factors)
static int enqueue_tri_sums(bnmtf_model* h) {
  Dir& r = h->rows; Dir& c = h->cols;
  for (int which = 0; which < 3; ++which) {
    const int width = which == 0 ? h->L : (which == 1 ? 2 * h->L : h->K + h->L);
    TriFactorArgs f;
    f.which = which; f.K = h->K; f.L = h->L; f.S = h->S; f.varS = h->varS;
    f.side = 0; f.rows = h->I; f.X = r.X; f.varX = r.var; f.out = h->Ad; launch_tri_factors(f, h->stream);
    f.side = 1; f.rows = h->J; f.X = c.X; f.varX = c.var; f.out = h->Bd; launch_tri_factors(f, h->stream);
    MetricArgs m;
    m.R = h->Rfull; m.Mp = h->Mtrain; m.I = h->I; m.J = h->J; m.A = h->Ad; m.B = h->Bd; m.K = width; m.A2 = nullptr; m.B2 = nullptr;
    m.out6 = h->tri_sums + 8 * which;
    CHK(metric_partials(h, &m.part));
    launch_metric_sums(m, h->stream);
  }
  return BNMTF_OK;
}

// BNMTF_TRI_OVERLAP=0: the passes over R~ of an iteration in line instead of beside the S pass (A/B switch)
static bool tri_overlap(const bnmtf_model* h) {
  static const bool off = [] { const char* e = getenv("BNMTF_TRI_OVERLAP"); return e && atoi(e) == 0; }();
  return !off && !h->comm;       // (several GPUs: every rank's passes cover its own rows / columns only; in line)
}

// One iteration of bnmtf_vb_run (update_S in the order's first K L entries, update_F in the next K, update_G in the last L; update_tau,
// the metrics, the ELBO's pieces) on h->stream -- or, while a Recorder is installed (api_many.inc: the caller has checked
// trivb_batchable), into its records, each under its site.  Recording, the order and the record of the
// iteration are the call's FIRST ones (the list forms add `it` steps), and the work that runs on the second stream otherwise
// (the masked variance sums of G, R~ E[G]) is recorded in line: the same kernels on the same operands, the same bits.
static int enqueue_trivb_iteration(bnmtf_model* h, int it, bool recording) {
  Dir& r = h->rows; Dir& c = h->cols;
  const int K = h->K, L = h->L, per = K * L + K + L;
  const bool overlap = tri_overlap(h);
  if (recording && (!g_recorder || !overlap)) { set_error("a recorded tri-factorisation iteration needs a recorder and the overlapped passes"); return BNMTF_ESTATE; }
  const int* ord = h->tri_order + (recording ? 0 : (size_t)it * per);
  const int step = recording ? per : 0;
  // Contractions of an iteration (round 6): R~ (E[G] E[S]^T) = (R~ E[G]) E[S]^T and R~^T (E[F] E[S]) = (R~^T E[F]) E[S] -- the passes over
  // R~ do not wait for S.  R~ E[G] and the masked variance sums of G (E[G], varG: final since the last G sweep) run on a second
  // stream BESIDE the S pass (one compute unit of 256 for ~160 us); R~^T E[F] is formed once behind the F sweep and serves the G
  // step and the next iteration's S system.  Three passes over R~ on the critical path became one.  BNMTF_TRI_OVERLAP=0: in line.
  // Several GPUs (round 6): rows of F and columns of G updated by their owners; the blocks of (E, var, S2) gathered behind each half
  // sweep (the other side's effective factor, masked variance sums and column Grams read every row); the S system summed over the
  // ranks' column ranges and walked by every rank; the iteration's sums exchanged as 21 doubles.
  auto slab_product = [&](const float* slabs_in, int split, int n_pad, float* out, int n, int transposeS) {
    SlabProductArgs sp;
    memset(&sp, 0, sizeof(sp));
    sp.slabs = slabs_in; sp.split = split; sp.n_pad = n_pad; sp.KPin = 32; sp.S = h->S; sp.K = K; sp.L = L; sp.n = n; sp.out = out; sp.KPout = 32;
    sp.transposeS = transposeS;
    launch_slab_product(sp, h->stream);
  };
  auto gemm_rows = [&](hipStream_t st) {                            // r.slabs = R~ E[G]
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.big = r.big; g.ld = r.n_pad; g.X = c.X; g.slabs = r.slabs; g.n_pad = r.n_pad; g.split = r.split; g.inner_per_wave = r.ipw; g.tw = r.gemm_tw;
    launch_gemm(g, r.KP, st);
  };
  {   // ---- S entries in shuffled order
    ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_S);
    CHK(enqueue_tri_ssys(h, overlap && h->tri_pv_current));
    if (recording) {
      site_at(kTsColsumRows);
      enqueue_tri_masked_colsum(h, 0, h->stream);
      site_at(kTsGemmRows);
      gemm_rows(h->stream);
    } else if (overlap) {
      HIPCHK(hipEventRecord(h->ev_aux0, h->stream));
      HIPCHK(hipStreamWaitEvent(h->aux_stream, h->ev_aux0, 0));
      enqueue_tri_masked_colsum(h, 0, h->aux_stream);
      gemm_rows(h->aux_stream);
      HIPCHK(hipEventRecord(h->ev_aux1, h->aux_stream));
    }
    enqueue_tri_chain(h, ord, K * L, 0, step);
  }
  // ---- F columns in their shuffled order
  if (overlap) {
    site_at(kTsProductF);
    enqueue_tri_side_prepare(h, 0, 1);
    if (!recording) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_aux1, 0));
    site_at(kTsSlabF);
    slab_product(r.slabs, r.split, r.n_pad, r.slabs, r.n, 1);       // (in place: a unit's half wave reads all of its row before it writes slab 0)
  } else enqueue_tri_side_prepare(h, 0);
  {
    ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_ROWS);
    site_at(kTsSweepF);
    enqueue_tri_sweep(h, 0, ord + K * L, false, overlap, nullptr, step);
  }
  if (h->comm)
    for (float* X : {r.X, r.var, r.S2}) CHK(comm_allgather_factor(h->comm, X, r.KP, r.nglob, h->world, h->stream));
  site_at(kTsPostF);
  enqueue_post(h, r, true);
  site_at(kTsColGramsNext);
  enqueue_tri_colgrams(h);                 // (+ mv_cols for the G sweep below)
  // ---- G columns
  if (overlap) {
    { ScopedKernelTimer t(h, BNMTF_KERNEL_GEMM_COLS); site_at(kTsPvNext); enqueue_tri_pv(h); }      // R~^T E[F] of the F just written
    h->tri_pv_current = true;
    site_at(kTsProductG);
    enqueue_tri_side_prepare(h, 2, 1);
    site_at(kTsSlabG);
    slab_product(h->slabsS, c.split, c.n_pad, c.slabs, c.n, 0);
  } else enqueue_tri_side_prepare(h, 2, 1 | 4);
  int sweep_blocks = 0;
  {
    ScopedKernelTimer t(h, BNMTF_KERNEL_SWEEP_COLS);
    site_at(kTsSweepG);
    enqueue_tri_sweep(h, 2, ord + K * L + K, true, overlap, h->comm ? nullptr : &sweep_blocks, step);
  }
  if (h->comm)
    for (float* X : {c.X, c.var, c.S2}) CHK(comm_allgather_factor(h->comm, X, c.KP, c.nglob, h->world, h->stream));
  site_at(kTsPostG);
  enqueue_post(h, c, true);
  // ---- update_tau, update_exp_tau, predict(M).  Round 6: exp_square_diff (:235-239) without a pass over R -- it was three
  // direct fp64 passes of 323 us each at 4096^2.  With m = E[F] E[S] (the G sweep's effective factor: mean m, second moment S2e):
  //   first term + the metrics: the SSE identity on the G sweep's own sums (sum P.G, sum_miss q, sum_miss q^2) and the Grams;
  //   second + fourth term  = sum_Omega sum_l (S2G_jl S2e_il - E[G_jl]^2 m_il^2)  -- the BNMF-VB second-moment term against the
  //                           effective factor: column sums, Gram diagonals and the sweep's two masked sums per (j, l);
  //   third term            = sum_jk mvF_jk ((E[S] E[G]^T)^2 - E[S]^2 (E[G]^2)^T)_kj  with the masked variance sums of the G step.
  TriThirdArgs t3;
  memset(&t3, 0, sizeof(t3));
  t3.rows = c.n; t3.K = K; t3.L = L; t3.G = c.X + (size_t)c.n0 * 32; t3.S = h->S; t3.mv = h->mv_cols; t3.part = h->tri_third;
  site_at(kTsThird);
  launch_tri_third(t3, h->stream);
  VbFinishArgs f;
  memset(&f, 0, sizeof(f));
  f.acc = h->acc; f.stats_r = r.vb_stats; f.nr = r.vb_stat_rows; f.stats_c = c.vb_stats; f.nc = c.vb_stat_rows;
  f.Cr64 = h->reff.C64; f.Cc64 = c.C64; f.sr = h->reff.colsum; f.sc = c.colsum; f.s2r = h->reff.colsum2; f.s2c = c.colsum2; f.KP = c.KP;
  f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
  f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->vb_rec + (recording ? 0 : (size_t)it * 16);      // (recording: the list form adds `it` records)
  f.extra = h->tri_third; f.n_extra = tri_third_blocks(c.n);
  f.sweep_stats = sweep_blocks > 0 ? c.stats : nullptr; f.n_sweep_stats = sweep_blocks;
  if (h->comm) {
    // [0..2] the SSE-identity sums, [4..9] the pieces of the rows, [12..17] of the columns, [20] the third term: one all-reduce
    HIPCHK(hipMemsetAsync(h->vbred, 0, 24 * sizeof(double), h->stream));
    launch_sum_cols(h->acc, 1, 4, 3, h->vbred, h->stream);
    launch_sum_cols(r.vb_stats, r.vb_stat_rows, 8, 6, h->vbred + 4, h->stream);
    launch_sum_cols(c.vb_stats, c.vb_stat_rows, 8, 6, h->vbred + 12, h->stream);
    launch_sum_cols(h->tri_third, tri_third_blocks(c.n), 1, 1, h->vbred + 20, h->stream);
    CHK(comm_allreduce_sum(h->comm, h->vbred, 21, h->stream));
    f.acc = h->vbred; f.stats_r = h->vbred + 4; f.nr = 1; f.stats_c = h->vbred + 12; f.nc = 1;
    f.extra = h->vbred + 20; f.n_extra = 1;
  }
  site_at(kTsFinish);
  launch_vb_finish(f, h->stream);
  if (recording && (sweep_blocks == 0 || g_recorder->missing)) {
    set_error("a recorded tri-factorisation iteration met a kernel without a list form (%s)", g_recorder->missing ? g_recorder->missing : "the G sweep's sums");
    return BNMTF_ESTATE;
  }
  if (sweep_blocks == 0) HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));       // (acc was used: clean for the next iteration)
  h->iteration++;
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_vb_set_state(bnmtf_handle h, const double* muF, const double* tauF, const double* expF, const double* varF,
                       const double* muS, const double* tauS, const double* expS, const double* varS,
                       const double* muG, const double* tauG, const double* expG, const double* varG, double exptau) try {
  HIPCHK(hipSetDevice(h->device));
  CHK(ensure_tri(h));
  CHK(vb_upload_dir(h, h->rows, muF, tauF, expF, varF));
  CHK(vb_upload_dir(h, h->cols, muG, tauG, expG, varG));
  const size_t n2 = (size_t)h->K * h->L;
  std::vector<float> tmp(n2);
  const double* src[4] = {muS, tauS, expS, varS};
  float* dst[4] = {h->muS, h->tauS, h->S, h->varS};
  for (int q = 0; q < 4; ++q) {
    if (!src[q]) continue;
    for (size_t t = 0; t < n2; ++t) tmp[t] = (float)src[q][t];
    HIPCHK(hipMemcpy(dst[q], tmp.data(), n2 * sizeof(float), hipMemcpyHostToDevice));
  }
  CHK(set_tau(h, exptau));
  h->have_state = true;
  h->tri_pv_current = h->tri_mv_cols_current = h->tri_w_current = false;
  h->ho_regions_current = false;          // (q hand-over: whatever the regions hold belongs to the state that was just replaced)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_vb_get_state(bnmtf_handle h, double* muF, double* tauF, double* expF, double* varF,
                       double* muS, double* tauS, double* expS, double* varS,
                       double* muG, double* tauG, double* expG, double* varG) try {
  if (!h->tri_ready || !h->have_state) { set_error("no bnmtf_vb state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  Dir& r = h->rows; Dir& c = h->cols;
  if (muF) CHK(download_matrix(h, r.mu, h->I, r.W, r.KP, muF));
  if (tauF) CHK(download_matrix(h, r.tauq, h->I, r.W, r.KP, tauF));
  if (expF) CHK(download_matrix(h, r.X, h->I, r.W, r.KP, expF));
  if (varF) CHK(download_matrix(h, r.var, h->I, r.W, r.KP, varF));
  if (muG) CHK(download_matrix(h, c.mu, h->J, c.W, c.KP, muG));
  if (tauG) CHK(download_matrix(h, c.tauq, h->J, c.W, c.KP, tauG));
  if (expG) CHK(download_matrix(h, c.X, h->J, c.W, c.KP, expG));
  if (varG) CHK(download_matrix(h, c.var, h->J, c.W, c.KP, varG));
  double* dst[4] = {muS, tauS, expS, varS};
  const float* src[4] = {h->muS, h->tauS, h->S, h->varS};
  for (int q = 0; q < 4; ++q) if (dst[q]) CHK(download_matrix(h, src[q], h->K, h->L, h->L, dst[q]));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// update_F(k) (which = 0, :241-250), update_S(k,l) (which = 1, :252-262), update_G(l) (which = 2, :264-273) for the
// current state; moments != 0 also runs the matching update_exp_* (:276-285).
int bnmtf_vb_update(bnmtf_handle h, int which, int k, int l, int moments) try {
  if (!h->tri_ready || !h->have_state) { set_error("no bnmtf_vb state set"); return BNMTF_ESTATE; }
  if (h->world != 1) { set_error("update_F(k) / update_S(k,l) / update_G(l) are single-GPU hooks (a sharded model updates through run())"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  h->tri_pv_current = h->tri_mv_cols_current = h->tri_w_current = false;
  if (which == 1) {
    if (k < 0 || k >= h->K || l < 0 || l >= h->L) { set_error("S index out of range"); return BNMTF_EINVAL; }
    if (h->tri_order_cap < 1) { dfree(h->tri_order); CHK(dalloc(&h->tri_order, 64, false)); h->tri_order_cap = 64; }
    const int a = k * h->L + l;
    HIPCHK(hipMemcpy(h->tri_order, &a, sizeof(int), hipMemcpyHostToDevice));
    CHK(enqueue_tri_ssys(h));
    enqueue_tri_chain(h, h->tri_order, 1, moments ? 0 : 1);
  } else {
    Dir& d = which == 0 ? h->rows : h->cols;
    const int col = which == 0 ? k : l;
    if (col < 0 || col >= d.W) { set_error("column %d out of range", col); return BNMTF_EINVAL; }
    enqueue_tri_side_prepare(h, which);
    SweepArgs s = tri_sweep_args(h, which, nullptr);
    s.only_k = col; s.vb_moments = moments ? 1 : 0; s.vb_stats = nullptr;
    launch_sweep(s, h->stream);
    enqueue_post(h, d, true);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// exp_square_diff() (:235-239) and the six training-mask sums (n, sum R, sum R^2, sum P, sum P^2, sum R P; P = E[F]E[S]E[G]^T)
int bnmtf_vb_exp_square_diff(bnmtf_handle h, double* esd_out, double sums_out[6]) try {
  if (!h->tri_ready || !h->have_state) { set_error("no bnmtf_vb state set"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  CHK(enqueue_tri_sums(h));
  double s[24];
  HIPCHK(hipMemcpyAsync(s, h->tri_sums, sizeof(s), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  if (esd_out) *esd_out = (s[2] - 2.0 * s[5] + s[4]) + s[8 + 3] + s[16 + 3];
  if (sums_out) for (int t = 0; t < 6; ++t) sums_out[t] = s[t];
  return BNMTF_OK;
} BNMTF_ABI_GUARD

// run(iterations) (:160-205).  orders [n_iter][K L + K + L]: per iteration the shuffled S entries (k L + l), F columns
// and G columns (the host draws them with random.shuffle, as the reference does).  exptau_out [n_iter]; perf_out
// [n_iter][3]; elbo_terms_out [n_iter][10] = {exp_square_diff, beta_s, the four O(IK) sums of elbo() for F, the four for
// G} (the K L terms of S are finished by the host); times_out [n_iter].
int bnmtf_vb_run(bnmtf_handle h, int n_iter, const int32_t* orders, double* exptau_out, double* perf_out,
                 double* elbo_terms_out, double* times_out) try {
  if (!h->tri_ready || !h->have_state) { set_error("bnmtf_vb_run before bnmtf_vb_set_state"); return BNMTF_ESTATE; }
  if (n_iter <= 0) return n_iter == 0 ? BNMTF_OK : BNMTF_EINVAL;
  if (!orders) { set_error("bnmtf_vb_run: orders required"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  Dir& r = h->rows; Dir& c = h->cols;
  const int K = h->K, L = h->L, per = K * L + K + L;
  if (h->tri_order_cap < (size_t)n_iter * per) { dfree(h->tri_order); CHK(dalloc(&h->tri_order, (size_t)n_iter * per, false)); h->tri_order_cap = (size_t)n_iter * per; }
  HIPCHK(hipMemcpy(h->tri_order, orders, (size_t)n_iter * per * sizeof(int), hipMemcpyHostToDevice));
  CHK(vb_reserve_rec(h, n_iter));
  CHK(heldout_begin(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  if (tri_overlap(h)) {                    // (the second stream of enqueue_trivb_iteration)
    if (!h->aux_stream) HIPCHK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&h->ev_aux0, &h->ev_aux1})
      if (!*e) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(enqueue_trivb_iteration(h, it, false));
    heldout_enqueue(h, it, h->stream);           // (a mask set: on E[F], E[S], E[G] of this iteration)
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
  }
  if (h->comm)      // the q parameters of the other ranks' rows / columns (bnmtf_vb_get_state returns whole matrices)
    for (Dir* d : {&r, &c})
      for (float* X : {d->mu, d->tauq}) CHK(comm_allgather_factor(h->comm, X, d->KP, d->nglob, h->world, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  drain_events(h);
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 16);
  HIPCHK(hipMemcpy(rec.data(), h->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_vb_rec(rec.data(), n_iter, exptau_out, perf_out, elbo_terms_out);       // (terms: esd, beta_s, the four sums of F, the four of G)
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
