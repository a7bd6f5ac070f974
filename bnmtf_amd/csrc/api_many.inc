// Many models, one launch per launch site (many.h) -- included at the end of api.hip.  The reference's model searches (a
// cross-validation's folds x ranks, a greedy walk over K, L: experiments_gdsc/cross_validation/) are dozens to hundreds of independent
// small models; a kernel of one of them occupies a few dozen blocks of the chip, and its iteration is a chain of dependent launches
// (eleven for bnmf_vb, ~25 for bnmtf_vb with its S chain on one block, K L + 9 for NMTF).  run_many walks the models' iterations in
// lock-step: the host code of a model's iteration runs with a Recorder installed (the launchers append their list-form kernel, its
// arguments and the site key instead of launching), then the records of a site that agree in kernel, block and grid become ONE
// launch with blockIdx.z = model.  Records meet by key, not by position, so models may differ in shape, rank and kind: a shorter S
// chain has no record at the later passes, a call's first bnmtf_vb iteration forms R~^T E[F] and the column Grams inside the S system
// and later ones do not.  The list forms run the single-model kernels' bodies: every model ends with the bits of its own run.
// A family of models (ManyFamily) brings what differs; the three entry points below marshal their arguments and call run_many.

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

struct RecorderScope {
  explicit RecorderScope(Recorder* r) { g_recorder = r; }
  ~RecorderScope() { g_recorder = nullptr; }
};


// at[s]: the records of site s, the sites in key order
void align_sites(const std::vector<Recorder>& recs, SiteMembers& at) {
  std::map<std::pair<int, int>, size_t> order;
  for (const Recorder& r : recs)
    for (const auto& k : r.keys) order[k] = 0;
  size_t n = 0;
  for (auto& o : order) o.second = n++;
  at.assign(n, {});
  for (size_t i = 0; i < recs.size(); ++i)
    for (size_t q = 0; q < recs[i].keys.size(); ++q) at[order[recs[i].keys[q]]].push_back({(int)i, (int)q});
}

// a model's slices of the model-major outputs: the family's (up to three) arrays and the batch's clock; any may be null
struct ManyOut { double* a[3]; double* times; };

// What a family of models brings to run_many.
struct ManyFamily {
  const char* name;                    // the entry point, for messages
  int width[3];                        // doubles per model and iteration of the family's output arrays (0: no such array)
  bool takes_orders;                   // per model the update orders of its run (bnmtf_vb)
  bool handover;                       // a HandoverScope per batched model, as the model's own run holds one
  bool same_length;                    // no site is named: every model enqueues the same launches, aligned by position
  int (*ready)(bnmtf_model*, int b);   // the right kind of handle, with a state -- or the message and the code
  bool (*batchable)(bnmtf_model*);     // its iteration consists of kernels that have a list form
  int (*prepare)(bnmtf_model*, int n_iter, const int32_t* orders);     // before the model's own stream is drained
  int (*enqueue)(bnmtf_model*, int it);                                // one recorded iteration
  int (*run_alone)(bnmtf_model*, int n_iter, const int32_t* orders, const ManyOut& o);   // the model's own entry point
  int (*read_out)(bnmtf_model*, int n_iter, const ManyOut& o);         // the device record -> the family's outputs
};
// (every family: a model with a held-out mask -- bnmtf_set_heldout -- reserves its record in prepare and appends the held-out launch
// pair at kHeldoutSite behind the iteration's records; a model without one records nothing there.)

int check_many_handles(const ManyFamily& f, bnmtf_handle* hs, int n_models, int n_iter, const int32_t* const* orders) {
  if (n_models < 0 || (n_models > 0 && (!hs || (f.takes_orders && !orders)))) {
    set_error("%s: %d models at %p, orders at %p", f.name, n_models, (void*)hs, (const void*)orders);
    return BNMTF_EINVAL;
  }
  if (n_iter < 0) { set_error("run: negative iteration count"); return BNMTF_EINVAL; }
  for (int b = 0; b < n_models; ++b) {
    if (!hs[b]) { set_error("run_many: null handle (model %d)", b); return BNMTF_EINVAL; }
    for (int c = 0; c < b; ++c) if (hs[c] == hs[b]) { set_error("run_many: model %d is given twice", b); return BNMTF_EINVAL; }
    if (hs[b]->device != hs[0]->device) { set_error("run_many: the models of a call share a device (model %d: device %d, model 0: device %d)", b, hs[b]->device, hs[0]->device); return BNMTF_EINVAL; }
    CHK(f.ready(hs[b], b));
    if (f.takes_orders && n_iter > 0 && !orders[b]) { set_error("%s: orders required (model %d)", f.name, b); return BNMTF_EINVAL; }
  }
  return BNMTF_OK;
}

// n_iter iterations of n_models models of one family on one device.  The models that can share launches -- two at least -- walk in
// lock-step on the first one's stream; the others run through their own entry point one after the other.  *launch_info (optional,
// 2 ints): models that shared launches, argument-list uploads.
int run_many(const ManyFamily& f, bnmtf_handle* hs, int n_models, int n_iter, const int32_t* const* orders, double* const (&outs)[3],
             double* times_out, int* launch_info) {
  if (launch_info) launch_info[0] = launch_info[1] = 0;
  CHK(check_many_handles(f, hs, n_models, n_iter, orders));
  if (n_models == 0 || n_iter == 0) return BNMTF_OK;
  auto out = [&](int b) {
    ManyOut o;
    for (int k = 0; k < 3; ++k) o.a[k] = outs[k] ? outs[k] + (size_t)b * n_iter * f.width[k] : nullptr;
    o.times = times_out ? times_out + (size_t)b * n_iter : nullptr;
    return o;
  };
  std::vector<int> batch;
  for (int b = 0; b < n_models; ++b) if (f.batchable(hs[b])) batch.push_back(b);
  if (batch.size() < 2) batch.clear();
  {
    std::vector<char> in(n_models, 0);
    for (int b : batch) in[b] = 1;
    for (int b = 0; b < n_models; ++b)
      if (!in[b]) CHK(f.run_alone(hs[b], n_iter, orders ? orders[b] : nullptr, out(b)));
  }
  if (batch.empty()) return BNMTF_OK;
  HIPCHK(hipSetDevice(hs[0]->device));
  const size_t nb = batch.size();
  std::vector<std::unique_ptr<HandoverScope>> scopes;
  for (int b : batch) {
    bnmtf_model* h = hs[b];
    CHK(f.prepare(h, n_iter, orders ? orders[b] : nullptr));
    if (f.handover) scopes.push_back(std::make_unique<HandoverScope>(h));
    HIPCHK(hipStreamSynchronize(h->stream));           // (everything the model's own stream still holds -- its state's upload -- before the batch's stream reads it)
  }
  hipStream_t st = hs[batch[0]]->stream;
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], st));
  std::vector<Recorder> recs(nb);
  std::vector<std::vector<std::pair<int, int>>> last(nb);
  SiteMembers at;
  std::vector<std::unique_ptr<ManySite>> sites;
  long uploads = 0;
  for (int it = 0; it < n_iter; ++it) {
    bool same = it > 0;
    for (size_t i = 0; i < nb; ++i) {
      recs[i].clear();
      RecorderScope scope(&recs[i]);
      CHK(f.enqueue(hs[batch[i]], it));
      if (recs[i].missing) { set_error("run_many: a recorded iteration met a kernel without a list form (%s)", recs[i].missing); return BNMTF_ESTATE; }
      if (recs[i].keys.size() != recs[i].recs.size()) { set_error("run_many: model %d has %zu records and %zu site keys", batch[i], recs[i].recs.size(), recs[i].keys.size()); return BNMTF_ESTATE; }
      auto unnamed = [](const Recorder& r) { size_t n = 0; for (const auto& k : r.keys) n += k.first < 0; return n; };      // (the held-out pair has a site)
      if (f.same_length && unnamed(recs[i]) != unnamed(recs[0])) { set_error("run_many: model %d enqueues %d launches an iteration, model 0 %d", (int)i, (int)unnamed(recs[i]), (int)unnamed(recs[0])); return BNMTF_ESTATE; }
      same = same && recs[i].keys == last[i];
    }
    if (!same) {                                       // (the first iteration of a call may differ from the later ones)
      align_sites(recs, at);
      for (size_t i = 0; i < nb; ++i) last[i] = recs[i].keys;
    }
    CHK(launch_sites(recs, at, sites, it, st, &uploads));
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  for (int b : batch) heldout_end(hs[b], n_iter);
  if (launch_info) { launch_info[0] = (int)nb; launch_info[1] = (int)uploads; }
  std::vector<double> tm(times_out ? n_iter : 0);
  ev.seconds((int)tm.size(), tm.data());
  for (int b : batch) {
    const ManyOut o = out(b);
    CHK(f.read_out(hs[b], n_iter, o));
    if (o.times) std::copy(tm.begin(), tm.end(), o.times);
  }
  return BNMTF_OK;
}

int vb_read_out(bnmtf_model* h, int n_iter, const ManyOut& o) {
  std::vector<double> rec((size_t)n_iter * 16);
  HIPCHK(hipMemcpy(rec.data(), h->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_vb_rec(rec.data(), n_iter, o.a[0], o.a[1], o.a[2]);
  return BNMTF_OK;
}
// (acc: zeroed on the model's own stream, which the driver drains next)
int vb_prepare(bnmtf_model* h, int n_iter, const int32_t*) {
  CHK(vb_reserve_rec(h, n_iter));
  CHK(heldout_begin(h, n_iter));
  HIPCHK(hipMemsetAsync(h->acc, 0, 4 * sizeof(double), h->stream));
  return BNMTF_OK;
}

// bnmf_vb_optimised: every model enqueues the same eleven launches.  Not batched: several GPUs, the 16-wave shapes of large
// problems, per-kernel timers on.
const ManyFamily kVbFamily = {
  "bnmf_vb_run_many", {1, 3, 10}, false, true, true,
  [](bnmtf_model* h, int b) { if (h->vb_ready && h->have_state) return BNMTF_OK; set_error("bnmf_vb_run_many before bnmf_vb_set_state (model %d)", b); return BNMTF_ESTATE; },
  vb_batchable, vb_prepare,
  [](bnmtf_model* h, int it) { CHK(enqueue_vb_iteration(h, it, true)); heldout_enqueue(h, it, h->stream); return BNMTF_OK; },
  [](bnmtf_model* h, int n_iter, const int32_t*, const ManyOut& o) { return bnmf_vb_run(h, n_iter, o.a[0], o.a[1], o.a[2], o.times); },
  vb_read_out};

// bnmtf_vb_optimised: the sites of TriSite; the orders of a model's run are uploaded before the loop (the list forms step through
// them).  Not batched: several GPUs, per-kernel timers, the 16-wave sweeps, an A/B switch.
const ManyFamily kTriVbFamily = {
  "bnmtf_vb_run_many", {1, 3, 10}, true, false, false,
  [](bnmtf_model* h, int b) { if (h->tri_ready && h->have_state) return BNMTF_OK; set_error("bnmtf_vb_run_many before bnmtf_vb_set_state (model %d)", b); return BNMTF_ESTATE; },
  trivb_batchable,
  [](bnmtf_model* h, int n_iter, const int32_t* orders) {
    const size_t n = (size_t)n_iter * ((size_t)h->K * h->L + h->K + h->L);
    if (h->tri_order_cap < n) { dfree(h->tri_order); h->tri_order_cap = 0; CHK(dalloc(&h->tri_order, n, false)); h->tri_order_cap = n; }
    HIPCHK(hipMemcpy(h->tri_order, orders, n * sizeof(int), hipMemcpyHostToDevice));
    return vb_prepare(h, n_iter, nullptr);
  },
  [](bnmtf_model* h, int it) { CHK(enqueue_trivb_iteration(h, it, true)); heldout_enqueue(h, it, h->stream); return BNMTF_OK; },
  [](bnmtf_model* h, int n_iter, const int32_t* orders, const ManyOut& o) { return bnmtf_vb_run(h, n_iter, orders, o.a[0], o.a[1], o.a[2], o.times); },
  vb_read_out};

// nmf_np.NMF and nmtf_np.NMTF in any mix: the sites of NpSite; every model with a state is batched.
const ManyFamily kNpFamily = {
  "bnmtf_np_run_many", {3, 1, 0}, false, false, false,
  [](bnmtf_model* h, int b) {
    if (!h->np) { set_error("run_many: model %d is not a handle of bnmtf_np_create", b); return BNMTF_EINVAL; }
    if (!h->np->have_state) { set_error("bnmtf_np_run_many before set_state (model %d)", b); return BNMTF_ESTATE; }
    return BNMTF_OK;
  },
  [](bnmtf_model*) { return true; },
  [](bnmtf_model* h, int n_iter, const int32_t*) { CHK(np_reserve_rec(h->np, n_iter)); return heldout_begin(h, n_iter); },
  [](bnmtf_model* h, int it) { CHK(np_iteration(h, h->np->rec)); np_heldout_enqueue(h, it); return BNMTF_OK; },
  [](bnmtf_model* h, int n_iter, const int32_t*, const ManyOut& o) { HIPCHK(hipSetDevice(h->device)); return np_run(h, n_iter, o.a[0], o.a[1], o.times); },
  [](bnmtf_model* h, int n_iter, const ManyOut& o) {
    std::vector<double> rec((size_t)n_iter * 8);
    HIPCHK(hipMemcpy(rec.data(), h->np->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    unpack_np_rec(rec.data(), n_iter, o.a[0], o.a[1]);
    return BNMTF_OK;
  }};

}  // namespace

extern "C" {

// The *_run of n_models models on one device (include/bnmtf_hip.h).  Outputs per model, model-major, any of them null:
// exptau_out[n_models][n_iter], perf_out[n_models][n_iter][3], elbo_terms_out[n_models][n_iter][10], idiv_out[n_models][n_iter],
// times_out[n_models][n_iter] (the batch's clock: the models of a batch finish an iteration together).  orders[b]: model b's
// [n_iter][K L + K + L] update orders (bnmtf_vb_run's).
int bnmf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out,
                     int* launch_info) try {
  double* const outs[3] = {exptau_out, perf_out, elbo_terms_out};
  return run_many(kVbFamily, hs, n_models, n_iter, nullptr, outs, times_out, launch_info);
} BNMTF_ABI_GUARD

int bnmtf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, const int32_t* const* orders, double* exptau_out, double* perf_out,
                      double* elbo_terms_out, double* times_out, int* launch_info) try {
  double* const outs[3] = {exptau_out, perf_out, elbo_terms_out};
  return run_many(kTriVbFamily, hs, n_models, n_iter, orders, outs, times_out, launch_info);
} BNMTF_ABI_GUARD

int bnmtf_np_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* perf_out, double* idiv_out, double* times_out, int* launch_info) try {
  double* const outs[3] = {perf_out, idiv_out, nullptr};
  return run_many(kNpFamily, hs, n_models, n_iter, nullptr, outs, times_out, launch_info);
} BNMTF_ABI_GUARD

}  // extern "C"
