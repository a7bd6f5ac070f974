// Many variational tri-factorisations, one launch per launch site (many.h, api_many.inc) -- included at the end of api.hip.  The
// reference's model searches over bnmtf_vb_optimised (experiments_gdsc/cross_validation/vb_nmtf/greedysearch_xval_vb.py: 10 folds x
// a greedy walk over K, L of the 622 x 138 GDSC matrix) are dozens to hundreds of independent small models; an iteration of one is
// ~25 dependent launches of a few dozen blocks each, and its S chain runs on one block.  bnmtf_vb_run_many walks the models'
// iterations in lock-step: a model's iteration is recorded (enqueue_trivb_iteration with a Recorder installed) with the site key of
// every record, and the records of a site that agree in kernel, block and grid become one launch with blockIdx.z = model.  The
// records are aligned by key, not by position: a call's first iteration forms R~^T E[F] and the column Grams inside the S system,
// later ones do not, and only K L >= 64 permutes the system for the blocked chain (whose block grows with K L).  The list forms run
// the single-model kernels' bodies: every model ends with the bits of its own bnmtf_vb_run.

namespace {

// a model whose iteration consists of kernels that have a list form: one GPU, no per-kernel timers, the overlapped passes over R~,
// both sweeps on the pair-panel kernel with the covariance term in its 8 + 2-wave shape, no A/B switch without a list form
bool trivb_batchable(bnmtf_model* h) {
  if (h->comm || h->profiling || !h->tri_ready || !h->have_state || h->block_mode || !tri_overlap(h)) return false;
  if (ssys_ab_switch_set() || trivb_ab_switch_set() || getenv("BNMTF_VB_GENERIC")) return false;
  if (vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows)) return false;          // (BNMTF_VB_PATH=masked: the generic sweep)
  for (int which : {0, 2}) {
    const Dir& d = which == 0 ? h->rows : h->cols;
    const Dir& e = which == 0 ? h->ceff : h->reff;
    if (!(h->use_fast && d.fast_ok && d.wide_can && d.pair_ok && d.f_gen_count == 0 && sweep_vb_cov_supported(d.KP, d.pw) && e.XS && e.XT2) ||
        d.use_wide)
      return false;
  }
  return true;
}

}  // namespace

extern "C" {

// bnmtf_vb_run of n_models models (one device); orders[b]: model b's [n_iter][K L + K + L] update orders (bnmtf_vb_run's).  Outputs
// per model, model-major: exptau_out[n_models][n_iter], perf_out[n_models][n_iter][3], elbo_terms_out[n_models][n_iter][10],
// times_out[n_models][n_iter] (the batch's clock); any of them may be null.  Models that cannot join a batch (several GPUs,
// per-kernel timers, the 16-wave sweeps, an A/B switch) are run by bnmtf_vb_run one after the other.  *launch_info (optional,
// 2 ints): models that shared launches, argument-list uploads.
int bnmtf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, const int32_t* const* orders, double* exptau_out, double* perf_out,
                      double* elbo_terms_out, double* times_out, int* launch_info) try {
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  if (n_models < 0 || (n_models > 0 && (!hs || !orders))) { set_error("bnmtf_vb_run_many: %d models at %p, orders at %p", n_models, (void*)hs, (const void*)orders); return BNMTF_EINVAL; }
  if (n_iter < 0) { set_error("run: negative iteration count"); return BNMTF_EINVAL; }
  for (int b = 0; b < n_models; ++b) {
    if (!hs[b]) { set_error("run_many: null handle (model %d)", b); return BNMTF_EINVAL; }
    for (int c = 0; c < b; ++c) if (hs[c] == hs[b]) { set_error("run_many: model %d is given twice", b); return BNMTF_EINVAL; }
    if (hs[b]->device != hs[0]->device) { set_error("run_many: the models of a call share a device (model %d: device %d, model 0: device %d)", b, hs[b]->device, hs[0]->device); return BNMTF_EINVAL; }
    if (!hs[b]->tri_ready || !hs[b]->have_state) { set_error("bnmtf_vb_run_many before bnmtf_vb_set_state (model %d)", b); return BNMTF_ESTATE; }
    if (n_iter > 0 && !orders[b]) { set_error("bnmtf_vb_run_many: orders required (model %d)", b); return BNMTF_EINVAL; }
  }
  if (n_models == 0 || n_iter == 0) return BNMTF_OK;
  auto out = [&](double* base, int b, int per) { return base ? base + (size_t)b * n_iter * per : nullptr; };
  std::vector<int> batch;
  for (int b = 0; b < n_models; ++b) if (trivb_batchable(hs[b])) batch.push_back(b);
  if (batch.size() < 2) batch.clear();
  {
    std::vector<char> in(n_models, 0);
    for (int b : batch) in[b] = 1;
    for (int b = 0; b < n_models; ++b)
      if (!in[b]) CHK(bnmtf_vb_run(hs[b], n_iter, orders[b], out(exptau_out, b, 1), out(perf_out, b, 3), out(elbo_terms_out, b, 10), out(times_out, b, 1)));
  }
  if (batch.empty()) return BNMTF_OK;
  HIPCHK(hipSetDevice(hs[0]->device));
  const size_t nb = batch.size();
  for (int b : batch) {
    bnmtf_model* h = hs[b];
    const size_t per = (size_t)h->K * h->L + h->K + h->L;
    if (h->tri_order_cap < (size_t)n_iter * per) { dfree(h->tri_order); CHK(dalloc(&h->tri_order, (size_t)n_iter * per, false)); h->tri_order_cap = (size_t)n_iter * per; }
    HIPCHK(hipMemcpy(h->tri_order, orders[b], (size_t)n_iter * per * sizeof(int), hipMemcpyHostToDevice));
    if (h->vb_rec_cap < (size_t)n_iter) { dfree(h->vb_rec); CHK(dalloc(&h->vb_rec, (size_t)n_iter * 16)); h->vb_rec_cap = n_iter; }
    HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));           // (everything the model's own stream still holds -- its state's upload -- before the batch's stream reads it)
  }
  hipStream_t st = hs[batch[0]]->stream;
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], st));
  std::vector<Recorder> recs(nb);
  std::vector<TriSiteKeys> keys(nb), last(nb);
  SiteMembers at;
  std::vector<std::unique_ptr<ManySite>> sites;
  long uploads = 0;
  for (int it = 0; it < n_iter; ++it) {
    bool same = it > 0;
    for (size_t i = 0; i < nb; ++i) {
      recs[i].clear(); keys[i].clear();
      RecorderScope scope(&recs[i]);
      CHK(enqueue_trivb_iteration(hs[batch[i]], it, true, &keys[i]));
      if (keys[i].key.size() != recs[i].recs.size()) { set_error("run_many: model %d has %zu records and %zu site keys", batch[i], recs[i].recs.size(), keys[i].key.size()); return BNMTF_ESTATE; }
      same = same && keys[i].key == last[i].key;
    }
    if (!same) {                                     // the sites in key order (the first iterations of a call differ from the later ones)
      std::map<std::pair<int, int>, size_t> order;
      for (size_t i = 0; i < nb; ++i)
        for (const auto& k : keys[i].key) order[k] = 0;
      size_t n = 0;
      for (auto& o : order) o.second = n++;
      at.assign(n, {});
      for (size_t i = 0; i < nb; ++i)
        for (size_t q = 0; q < keys[i].key.size(); ++q) at[order[keys[i].key[q]]].push_back({(int)i, (int)q});
      for (size_t i = 0; i < nb; ++i) last[i].key = keys[i].key;
    }
    CHK(launch_sites(recs, at, sites, it, st, &uploads));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (launch_info) { launch_info[0] = (int)nb; launch_info[1] = (int)uploads; }
  std::vector<double> tm(times_out ? n_iter : 0);
  for (int it = 0; it < (int)tm.size(); ++it) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[it + 1]); tm[it] = (double)ms * 1e-3; }
  std::vector<double> rec((size_t)n_iter * 16);
  for (int b : batch) {
    HIPCHK(hipMemcpy(rec.data(), hs[b]->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *e = out(exptau_out, b, 1), *p = out(perf_out, b, 3), *t = out(elbo_terms_out, b, 10), *tt = out(times_out, b, 1);
    for (int it = 0; it < n_iter; ++it) {
      const double* q = &rec[(size_t)it * 16];
      if (e) e[it] = q[0];
      if (p) for (int m = 0; m < 3; ++m) p[(size_t)it * 3 + m] = q[1 + m];
      if (t) for (int m = 0; m < 10; ++m) t[(size_t)it * 10 + m] = q[4 + m];
      if (tt) tt[it] = tm[it];
    }
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
