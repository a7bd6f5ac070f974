// Many non-probabilistic models, one launch per launch site (many.h, api_many.inc) -- included at the end of api.hip.  The
// reference's model searches over these models (a cross-validation's ranks x folds of the 622 x 138 GDSC matrix) are dozens of
// independent small models; a kernel of one of them fills a few dozen blocks of the chip, and an NMTF iteration is a chain of
// K L + 9 dependent launches.  bnmtf_np_run_many walks the models' iterations in lock-step: a model's iteration is recorded
// (np_iteration with a Recorder installed) with the site key of every record, and the records of a site become one launch with
// blockIdx.z = model.  Models may differ in shape, in K and L and in kind, so their iterations differ in length: the records are
// aligned by site key (before the S step, S pass t, after it), not by position -- a model with a shorter S chain has no record at
// the later passes.  The list forms run the single-model kernels' bodies: every model ends with the bits of its own run.

extern "C" {

// bnmf_np_run / bnmtf_np_run of n_models handles of bnmtf_np_create on one device (NMF and NMTF in any mix).  Outputs per model,
// model-major: perf_out[n_models][n_iter][3], idiv_out[n_models][n_iter], times_out[n_models][n_iter] (the batch's clock); any of
// them may be null.  *launch_info (optional, 2 ints): models that shared launches, argument-list uploads.
int bnmtf_np_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* perf_out, double* idiv_out, double* times_out, int* launch_info) try {
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  if (n_models < 0 || (n_models > 0 && !hs)) { set_error("bnmtf_np_run_many: %d models at %p", n_models, (void*)hs); return BNMTF_EINVAL; }
  if (n_iter < 0) { set_error("run: negative iteration count"); return BNMTF_EINVAL; }
  for (int b = 0; b < n_models; ++b) {
    if (!hs[b]) { set_error("run_many: null handle (model %d)", b); return BNMTF_EINVAL; }
    if (!hs[b]->np) { set_error("run_many: model %d is not a handle of bnmtf_np_create", b); return BNMTF_EINVAL; }
    for (int c = 0; c < b; ++c) if (hs[c] == hs[b]) { set_error("run_many: model %d is given twice", b); return BNMTF_EINVAL; }
    if (hs[b]->device != hs[0]->device) { set_error("run_many: the models of a call share a device (model %d: device %d, model 0: device %d)", b, hs[b]->device, hs[0]->device); return BNMTF_EINVAL; }
    if (!hs[b]->np->have_state) { set_error("bnmtf_np_run_many before set_state (model %d)", b); return BNMTF_ESTATE; }
  }
  if (n_models == 0 || n_iter == 0) return BNMTF_OK;
  auto out = [&](double* base, int b, int per) { return base ? base + (size_t)b * n_iter * per : nullptr; };
  if (n_models == 1) { HIPCHK(hipSetDevice(hs[0]->device)); return np_run(hs[0], n_iter, out(perf_out, 0, 3), out(idiv_out, 0, 1), out(times_out, 0, 1)); }
  HIPCHK(hipSetDevice(hs[0]->device));
  const size_t nm = n_models;
  for (size_t b = 0; b < nm; ++b) {
    NpState* s = hs[b]->np;
    if ((size_t)n_iter > s->rec_cap) {
      dfree(s->rec); s->rec_cap = 0;
      CHK(dalloc(&s->rec, (size_t)n_iter * 8, false));
      s->rec_cap = n_iter;
    }
    HIPCHK(hipStreamSynchronize(hs[b]->stream));      // (whatever the model's own stream still holds, before the batch's stream reads it)
  }
  hipStream_t st = hs[0]->stream;
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], st));
  std::vector<Recorder> recs(nm);
  std::vector<NpSiteKeys> keys(nm);
  SiteMembers at;
  std::vector<size_t> n_recs(nm);
  std::vector<std::unique_ptr<ManySite>> sites;
  long uploads = 0;
  for (int it = 0; it < n_iter; ++it) {
    for (size_t b = 0; b < nm; ++b) {
      recs[b].clear();
      RecorderScope scope(&recs[b]);
      NpSiteKeys* k = nullptr;
      if (it == 0) k = &keys[b];
      CHK(np_iteration(hs[b], hs[b]->np->rec, k));
      if (it == 0) n_recs[b] = recs[b].recs.size();
      else if (recs[b].recs.size() != n_recs[b]) { set_error("run_many: model %d enqueued %zu launches, %zu before", (int)b, recs[b].recs.size(), n_recs[b]); return BNMTF_ESTATE; }
    }
    if (it == 0) {                                   // the sites in key order; every later iteration records the same keys
      std::map<std::pair<int, int>, size_t> order;
      for (size_t b = 0; b < nm; ++b) {
        if (keys[b].key.size() != n_recs[b]) { set_error("run_many: model %d has %zu records and %zu site keys", (int)b, n_recs[b], keys[b].key.size()); return BNMTF_ESTATE; }
        for (const auto& k : keys[b].key) order[k] = 0;
      }
      size_t n = 0;
      for (auto& o : order) o.second = n++;
      at.assign(n, {});
      for (size_t b = 0; b < nm; ++b)
        for (size_t q = 0; q < n_recs[b]; ++q) at[order[keys[b].key[q]]].push_back({(int)b, (int)q});
    }
    CHK(launch_sites(recs, at, sites, it, st, &uploads));
    for (size_t b = 0; b < nm; ++b) hs[b]->iteration++;
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (launch_info) { launch_info[0] = (int)nm; launch_info[1] = (int)uploads; }
  std::vector<double> tm(times_out ? n_iter : 0);
  for (int it = 0; it < (int)tm.size(); ++it) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[it + 1]); tm[it] = (double)ms * 1e-3; }
  std::vector<double> rec((size_t)n_iter * 8);
  for (size_t b = 0; b < nm; ++b) {
    HIPCHK(hipMemcpy(rec.data(), hs[b]->np->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *p = out(perf_out, (int)b, 3), *d = out(idiv_out, (int)b, 1), *t = out(times_out, (int)b, 1);
    for (int it = 0; it < n_iter; ++it) {
      if (p) np_perf(&rec[(size_t)it * 8], p + (size_t)it * 3);
      if (d) d[it] = rec[(size_t)it * 8 + 6];
      if (t) t[it] = tm[it];
    }
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
