// Many variational models, one launch per kernel (round 6; many.h).  The reference's model searches
// (experiments_gdsc/cross_validation/vb_nmf/linesearch_xval_vb.py:17-52: 10 folds x 4 ranks of a 622 x 138 matrix) are dozens
// of independent small models; a kernel of one of them occupies a few dozen blocks of the chip and its iteration is a chain of
// eleven dependent launches.  bnmf_vb_run_many walks the models' iterations in lock-step: the host code of a model's iteration
// runs with a Recorder installed (the launchers append their list-form kernel and arguments instead of launching), then the
// records of a launch site become ONE launch with blockIdx.z = model.  The kernels' bodies are the single-model kernels' bodies:
// every model ends with the bits its own bnmf_vb_run gives.

namespace bnmtf { thread_local Recorder* g_recorder = nullptr; }

namespace {

// a model whose iteration consists of kernels that have a list form: one GPU, the pair-panel variational sweep in its 8 + 2-wave
// shape (no q hand-over), no per-kernel timers
bool vb_batchable(bnmtf_model* h) {
  if (h->comm || h->profiling || !h->vb_ready || !h->have_state || h->block_mode) return false;
  for (Dir* d : {&h->rows, &h->cols}) {
    const bool fast = h->use_fast && d->fast_ok && d->wide_can && d->pair_ok && d->f_gen_count == 0 && sweep_vb_supported(d->KP, d->pw) &&
                      !getenv("BNMTF_VB_GENERIC");
    if (!fast || d->use_wide) return false;
  }
  return !(vb_chip_ok(h->rows, h->cols) && vb_chip_ok(h->cols, h->rows));
}

struct ManySite {
  void* dev = nullptr; size_t cap = 0;
  std::vector<unsigned char> last;
  ~ManySite() { if (dev) (void)hipFree(dev); }
};

// The launch sites of one iteration: at[s] lists (model, record index) of the models that have a record at site s, in model
// order.  Of a site, the models whose records agree in kernel, block and grid (grid.x too unless the kernel leaves by its own
// block count) share a launch.  Argument lists live in device memory and are uploaded again only when their bytes change (a
// variational iteration's arguments do not, after the first).
typedef std::vector<std::vector<std::pair<int, int>>> SiteMembers;
int launch_sites(std::vector<Recorder>& recs, const SiteMembers& at, std::vector<std::unique_ptr<ManySite>>& sites, int it, hipStream_t st,
                 long* uploads) {
  const size_t nm = recs.size(), ns = at.size();
  if (sites.size() < ns * nm) { const size_t old = sites.size(); sites.resize(ns * nm); for (size_t i = old; i < sites.size(); ++i) sites[i] = std::make_unique<ManySite>(); }
  std::vector<char> done;
  std::vector<int> members;
  for (size_t s = 0; s < ns; ++s) {
    const auto& here = at[s];
    auto rec = [&](size_t q) -> const LaunchRec& { return recs[here[q].first].recs[here[q].second]; };
    auto args = [&](size_t q) { return recs[here[q].first].args(rec(q)); };
    done.assign(here.size(), 0);
    int part = 0;
    for (size_t m0 = 0; m0 < here.size(); ++m0) {
      if (done[m0]) continue;
      const LaunchRec& r0 = rec(m0);
      unsigned gx = r0.grid.x; size_t lds = r0.lds;
      members.clear();
      for (size_t m = m0; m < here.size(); ++m) {
        if (done[m]) continue;
        const LaunchRec& r = rec(m);
        const bool same = r.fn == r0.fn && r.block.x == r0.block.x && r.block.y == r0.block.y && r.block.z == r0.block.z && r.grid.y == r0.grid.y &&
                          r.grid.z == 1 && r.size == r0.size && r.flex == r0.flex && (r.flex || r.grid.x == r0.grid.x);
        if (!same || members.size() == 65535) continue;
        done[m] = 1; members.push_back((int)m);
        gx = std::max(gx, r.grid.x); lds = std::max(lds, r.lds);
      }
      ManySite& site = *sites[s * nm + part++];
      const size_t sz = r0.size, total = sz * members.size();
      bool changed = site.last.size() != total;
      for (size_t k = 0; k < members.size() && !changed; ++k)
        changed = memcmp(site.last.data() + k * sz, args(members[k]), sz) != 0;
      if (changed) {
        if (getenv("BNMTF_MANY_DEBUG")) fprintf(stderr, "many: it %d site %d part %d: argument list of %zu models uploaded\n", it, (int)s, part - 1, members.size());
        site.last.resize(total);
        for (size_t k = 0; k < members.size(); ++k) memcpy(site.last.data() + k * sz, args(members[k]), sz);
        HIPCHK(hipStreamSynchronize(st));              // (a launch in flight may still read the old list)
        if (site.cap < total) { if (site.dev) (void)hipFree(site.dev); site.dev = nullptr; site.cap = 0; HIPCHK(hipMalloc(&site.dev, total)); site.cap = total; }
        HIPCHK(hipMemcpy(site.dev, site.last.data(), total, hipMemcpyHostToDevice));
        ++*uploads;
      }
      void* list = site.dev; int itv = it;
      void* kargs[2] = {&list, &itv};
      HIPCHK(hipLaunchKernel(r0.fn, dim3(gx, r0.grid.y, (unsigned)members.size()), r0.block, kargs, lds, st));
    }
  }
  return BNMTF_OK;
}

// the records of one iteration, site by site: every model enqueues the same launches in the same order (the variational path)
int launch_recorded(std::vector<Recorder>& recs, std::vector<std::unique_ptr<ManySite>>& sites, int it, hipStream_t st, long* uploads) {
  const size_t nm = recs.size(), ns = recs[0].recs.size();
  for (size_t m = 1; m < nm; ++m)
    if (recs[m].recs.size() != ns) { set_error("run_many: model %d enqueues %d launches an iteration, model 0 %d", (int)m, (int)recs[m].recs.size(), (int)ns); return BNMTF_ESTATE; }
  SiteMembers at(ns);
  for (size_t s = 0; s < ns; ++s)
    for (size_t m = 0; m < nm; ++m) at[s].push_back({(int)m, (int)s});
  return launch_sites(recs, at, sites, it, st, uploads);
}

struct RecorderScope {
  explicit RecorderScope(Recorder* r) { g_recorder = r; }
  ~RecorderScope() { g_recorder = nullptr; }
};

}  // namespace

extern "C" {

// bnmf_vb_run of n_models models (one device).  Outputs per model, model-major: exptau_out[n_models][n_iter],
// perf_out[n_models][n_iter][3], elbo_terms_out[n_models][n_iter][10], times_out[n_models][n_iter] (the batch's clock: every model
// of a batch finishes an iteration together); any of them may be null.  Models that cannot join a batch (several GPUs, the
// 16-wave shapes of large problems, per-kernel timers on) are run one after the other.  *launch_info (optional, 2 ints): models
// that shared launches, argument-list uploads.
int bnmf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out,
                     int* launch_info) try {
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  if (n_models <= 0 || !hs) return n_models == 0 ? BNMTF_OK : BNMTF_EINVAL;
  if (n_iter <= 0) return n_iter == 0 ? BNMTF_OK : BNMTF_EINVAL;
  for (int b = 0; b < n_models; ++b) {
    if (!hs[b]) { set_error("run_many: null handle (model %d)", b); return BNMTF_EINVAL; }
    if (!hs[b]->vb_ready || !hs[b]->have_state) { set_error("bnmf_vb_run_many before bnmf_vb_set_state (model %d)", b); return BNMTF_ESTATE; }
    if (hs[b]->device != hs[0]->device) { set_error("run_many: the models of a call share a device"); return BNMTF_EINVAL; }
    for (int c = 0; c < b; ++c) if (hs[c] == hs[b]) { set_error("run_many: model %d is given twice", b); return BNMTF_EINVAL; }
  }
  auto out = [&](double* base, int b, int per) { return base ? base + (size_t)b * n_iter * per : nullptr; };
  std::vector<int> batch;
  for (int b = 0; b < n_models; ++b) if (vb_batchable(hs[b])) batch.push_back(b);
  if (batch.size() < 2) batch.clear();
  {
    std::vector<char> in(n_models, 0);
    for (int b : batch) in[b] = 1;
    for (int b = 0; b < n_models; ++b)
      if (!in[b]) CHK(bnmf_vb_run(hs[b], n_iter, out(exptau_out, b, 1), out(perf_out, b, 3), out(elbo_terms_out, b, 10), out(times_out, b, 1)));
  }
  if (batch.empty()) return BNMTF_OK;
  HIPCHK(hipSetDevice(hs[0]->device));
  const size_t nb = batch.size();
  std::vector<std::unique_ptr<HandoverScope>> scopes;
  for (int b : batch) {
    bnmtf_model* h = hs[b];
    if (h->vb_rec_cap < (size_t)n_iter) { dfree(h->vb_rec); CHK(dalloc(&h->vb_rec, (size_t)n_iter * 16)); h->vb_rec_cap = n_iter; }
    scopes.push_back(std::make_unique<HandoverScope>(h));
    HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));           // (everything the model's own stream still holds -- its state's upload -- before the batch's stream reads it)
  }
  hipStream_t st = hs[batch[0]]->stream;
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], st));
  std::vector<Recorder> recs(nb);
  std::vector<std::unique_ptr<ManySite>> sites;
  long uploads = 0;
  for (int it = 0; it < n_iter; ++it) {
    for (size_t i = 0; i < nb; ++i) {
      recs[i].clear();
      RecorderScope scope(&recs[i]);
      CHK(enqueue_vb_iteration(hs[batch[i]], it, true));
      if (recs[i].missing) { set_error("run_many: a recorded variational iteration met a kernel without a list form (%s)", recs[i].missing); return BNMTF_ESTATE; }
    }
    CHK(launch_recorded(recs, sites, it, st, &uploads));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  if (launch_info) { launch_info[0] = (int)nb; launch_info[1] = (int)uploads; }
  std::vector<double> rec((size_t)n_iter * 16);
  for (int b : batch) {
    HIPCHK(hipMemcpy(rec.data(), hs[b]->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    double *e = out(exptau_out, b, 1), *p = out(perf_out, b, 3), *t = out(elbo_terms_out, b, 10), *tm = out(times_out, b, 1);
    for (int it = 0; it < n_iter; ++it) {
      const double* q = &rec[(size_t)it * 16];
      if (e) e[it] = q[0];
      if (p) for (int m = 0; m < 3; ++m) p[(size_t)it * 3 + m] = q[1 + m];
      if (t) for (int m = 0; m < 10; ++m) t[(size_t)it * 10 + m] = q[4 + m];
      if (tm) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[it + 1]); tm[it] = (double)ms * 1e-3; }
    }
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
