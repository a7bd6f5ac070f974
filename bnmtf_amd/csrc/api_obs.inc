// The observed-entry layout (C ABI part 6, layout='observed') -- included at the end of api.hip, ahead of api_obs_tri.inc and
// api_obs_trivb.inc, which build on what is here.
// A handle of bnmtf_obs_create (two factors) or bnmtf_otri_create (the tri-factorisation: h->L > 0) holds, in ONE ObsState, the
// observed entries as a row list and a column list, both factors row major and transposed in fp32, the prior rates, the long
// form's residual scratch and the second half sweep's partial sums: memory proportional to the number of observed entries.  None
// of the samplers' layouts, no dense operand, no copy of R or M.  The optional parts of the state:
//   * the tri-factorisation's effective factors and Pv (bnmtf_otri_create; null on a two-factor handle), with a row stride of 32
//     where a two-factor handle has K rounded up to 4;
//   * the variational buffers -- q's parameters and the half sweeps' partial sums per direction, the transposed S2 of a two-factor
//     handle, the effective factors' second moments of a tri-factorisation --, allocated by the first bnmf_vbo_set_state /
//     bnmtf_otvb_set_state, so a Gibbs / ICM handle holds none of them.
//   * the non-probabilistic models' parts (bnmtf_onp_create, api_obs_np.inc: the marker `np` is set): no prior rates, a row
//     stride per direction, NMTF's S and effective factors, eight-wide partial sums; such a handle runs the bnmtf_onp_* calls
//     only, and those run no other handle.
// obs_free is the one owner of all of it.  This file has the state, the helpers every model on the layout shares (one direction's
// build / put / q, the common part of create, the half sweeps' argument builders, the record and the hooks' tails, the list
// metric) and the two-factor models: the Gibbs / ICM iteration is two launches of obs_sweep_kernel and obs_finish_kernel
// (kernel_obs.hip) on the handle's stream, the samples leave through the SampleSink like bnmf_gibbs_run's, written into their
// slots by the sweeps themselves; the variational model (bnmf_vbo_*, kernel_obs_vb.hip) is at the end of the file.  One GPU.

namespace bnmtf {

struct ObsList {                 // one direction: units, their entries' inner indices and values
  uint32_t* ptr = nullptr; uint32_t* idx = nullptr; float* val = nullptr;
  float* X = nullptr; float* XT = nullptr; int n = 0, W = 0, ldT = 0;   // the direction's factor of W columns: [n][stride] and [W][ldT]
  int stride = 0;                                                  // its row stride: the state's, or -- a handle of bnmtf_onp_create -- W rounded up to 4
  float* lambda = nullptr;                                         // [n][stride]; null on a handle of bnmtf_onp_create, as the next two
  double* numer = nullptr; double* taup = nullptr;                 // cond-params scratch [n]
  uint32_t longest = 0; size_t long_units = 0;                     // most entries of a unit; units beyond the register form
  // variational state (obs_alloc_q): q's mu, tau, var [n][stride] beside the expectation in X / XT; on a two-factor handle also
  // S2 = var + X^2 transposed [W][ldT] with XT's zero word behind every column; the half sweep's partial sums [obs_sweep_blocks(n)][6]
  float* mu = nullptr; float* tauq = nullptr; float* var = nullptr; float* S2T = nullptr;
  double* vstat = nullptr;
  void free_all() {              // every pointer member above
    dfree(ptr); dfree(idx); dfree(val); dfree(X); dfree(XT); dfree(lambda); dfree(numer); dfree(taup);
    dfree(mu); dfree(tauq); dfree(var); dfree(S2T); dfree(vstat);
  }
};
struct ObsState {
  ObsList rows, cols;              // U's and V's direction, or F's (W = K) and G's (W = L)
  size_t n = 0; int stride = 0;    // entries; row stride of every row-major factor: K rounded up to 4, or kObsTriStride
  float* escratch = nullptr;       // [n]
  double* part = nullptr;          // [obs_sweep_blocks(J)][4]
  double* scal = nullptr;          // tau_d, tau_f and out8 of the metric sums (one allocation)
  double* out8 = nullptr;
  bool force_long = false;
  bool vb_alloc = false, vb_state = false;   // the variational buffers exist; they hold the state of the last variational set_state / run
  double* esd_part = nullptr;      // [obs_vb_esd_blocks(I)] exp_square_diff's partial sums
  // the tri-factorisation only (api_obs_tri.inc, api_obs_trivb.inc)
  float* ceffX = nullptr; float* ceffXT = nullptr;    // G S^T: [J][32] and [K][cols.ldT]
  float* reffX = nullptr; float* reffXT = nullptr;    // F S:   [I][32] and [L][rows.ldT]
  float* Pv = nullptr;                                // R~^T F [J][32]
  float* ceffS2 = nullptr; float* ceffS2T = nullptr;  // variational: second moment of G S^T, [J][32] and [K][cols.ldT]
  float* reffS2 = nullptr; float* reffS2T = nullptr;  // ... and of F S, [I][32] and [L][rows.ldT]
  // a handle of bnmtf_onp_create only (api_obs_np.inc): the marker; NMTF's S and the S step's output [K][L] and block partials
  // [2][onp_s_blocks(I)][2] (its effective factors are ceffX .. reffXT above, at the strides K and L rounded up to 4); the last half
  // sweep's and the metric call's partial sums [..][8]; the run's records [iterations][8]; what the single-column calls carry
  bool np = false;
  float* npS = nullptr; float* npS2 = nullptr; double* np_spart = nullptr;
  double* np_part = nullptr; double* np_mpart = nullptr;
  double* np_rec = nullptr; size_t np_rec_cap = 0;
  int np_next_which = -1, np_next_col = -1;        // escratch holds the P that column np_next_col of this direction continues from
};

static bool obs_is_tri(const bnmtf_model* h) { return h->L > 0; }
static bool obs_is_np(const bnmtf_model* h) { return h->obs && h->obs->np; }

static void obs_free(bnmtf_model* h) {
  ObsState* s = h->obs;
  if (!s) return;
  s->rows.free_all(); s->cols.free_all();
  dfree(s->escratch); dfree(s->part); dfree(s->scal); dfree(s->esd_part);
  dfree(s->ceffX); dfree(s->ceffXT); dfree(s->reffX); dfree(s->reffXT); dfree(s->Pv);
  dfree(s->ceffS2); dfree(s->ceffS2T); dfree(s->reffS2); dfree(s->reffS2T);
  dfree(s->npS); dfree(s->npS2); dfree(s->np_spart); dfree(s->np_part); dfree(s->np_mpart); dfree(s->np_rec);
  h->tau_d = nullptr; h->tau_f = nullptr;
  delete s;
  h->obs = nullptr;              // (a tri-factorisation's S, lambdaS and S system's buffers are the model's own: bnmtf_destroy frees them)
}

// Every entry point's first step (the bnmtf_onp_* calls: onp_check, api_obs_np.inc).  tri: the call belongs to the bnmtf_otri_* / bnmtf_otvb_* family; need: the state it works on.
// A tri-factorisation's sampler calls refuse a variational state; the two-factor ones run on its expectations (DESIGN.md section 2.7).
enum { kObsNoState = 0, kObsSamplerState, kObsVbState };
static int obs_check(bnmtf_model* h, bool tri, int need) {
  if (!h || !h->obs || h->obs->np || obs_is_tri(h) != tri) { set_error("not a handle of %s", tri ? "bnmtf_otri_create" : "bnmtf_obs_create"); return BNMTF_EINVAL; }
  if (need == kObsSamplerState && !h->have_state) { set_error("%s has not been called", tri ? "bnmtf_otri_set_state" : "bnmf_obs_set_state"); return BNMTF_ESTATE; }
  if (need == kObsSamplerState && tri && h->obs->vb_state) {
    set_error("the handle holds a variational state (bnmtf_otvb_set_state): it runs the bnmtf_otvb_* calls until bnmtf_otri_set_state replaces it");
    return BNMTF_ESTATE;
  }
  if (need == kObsVbState && !(h->obs->vb_state && h->have_state)) { set_error("%s has not been called", tri ? "bnmtf_otvb_set_state" : "bnmf_vbo_set_state"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

// The entries sorted by (major, minor) with two stable counting sorts: ptr [nmajor + 1], the minor indices ascending within a
// unit, the values beside them.  Returns the position of an entry that occurs twice, or -1.
static long long obs_sort(uint64_t n, const int32_t* major, const int32_t* minor, const float* values, int nmajor, int nminor,
                          std::vector<uint32_t>& ptr, std::vector<uint32_t>& idx, std::vector<float>& val) {
  std::vector<uint32_t> by_minor(n), cnt((size_t)nminor + 1, 0);
  for (uint64_t e = 0; e < n; ++e) cnt[(size_t)minor[e] + 1]++;
  for (int m = 0; m < nminor; ++m) cnt[m + 1] += cnt[m];
  for (uint64_t e = 0; e < n; ++e) by_minor[cnt[minor[e]]++] = (uint32_t)e;
  ptr.assign((size_t)nmajor + 1, 0);
  for (uint64_t e = 0; e < n; ++e) ptr[(size_t)major[e] + 1]++;
  for (int u = 0; u < nmajor; ++u) ptr[u + 1] += ptr[u];
  std::vector<uint32_t> at(ptr.begin(), ptr.end() - 1);
  idx.resize(n); val.resize(n);
  for (uint64_t q = 0; q < n; ++q) {
    const uint32_t e = by_minor[q];
    const uint32_t pos = at[major[e]]++;
    idx[pos] = (uint32_t)minor[e]; val[pos] = values[e];
  }
  for (int u = 0; u < nmajor; ++u)
    for (uint32_t p = ptr[u] + 1; p < ptr[u + 1]; ++p)
      if (idx[p] == idx[p - 1]) return (long long)p;
  return -1;
}

// What a create holds of the entries, built on the host before any device call (and handed out by bnmtf_obs_build_lists): the
// checked entries as a row list and a column list, and the sums of R over them.  Refuses an entry outside the matrix, an entry
// that occurs twice and a row or column without entries.
struct ObsLists {
  std::vector<uint32_t> rptr, ridx, cptr, cidx;
  std::vector<float> rval, cval;
  double sumR = 0, sumR2 = 0;
};
static int obs_lists(int I, int J, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values, ObsLists& ls) {
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("between 1 and 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e) {
    if (rows[e] < 0 || rows[e] >= I || cols[e] < 0 || cols[e] >= J) {
      set_error("entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], I, J);
      return BNMTF_EINVAL;
    }
    const double r = values[e]; ls.sumR += r; ls.sumR2 += r * r;
  }
  const long long dup = obs_sort(n, rows, cols, values, I, J, ls.rptr, ls.ridx, ls.rval);
  if (dup >= 0) {
    const int i = (int)(std::upper_bound(ls.rptr.begin(), ls.rptr.end(), (uint32_t)dup) - ls.rptr.begin()) - 1;
    set_error("the entry (%d, %u) occurs twice", i, ls.ridx[(size_t)dup]);
    return BNMTF_EINVAL;
  }
  (void)obs_sort(n, cols, rows, values, J, I, ls.cptr, ls.cidx, ls.cval);
  for (int i = 0; i < I; ++i) if (ls.rptr[i + 1] == ls.rptr[i]) { set_error("Fully unobserved row in R, row %d.", i); return BNMTF_EINVAL; }
  for (int j = 0; j < J; ++j) if (ls.cptr[j + 1] == ls.cptr[j]) { set_error("Fully unobserved column in R, column %d.", j); return BNMTF_EINVAL; }
  return BNMTF_OK;
}

// one direction: the list, the prior rates [n][stride], the factor of W columns in both forms and the hooks' scratch (lambda
// null: neither rates nor hooks -- the non-probabilistic models have no conditionals)
static int obs_build_dir(bnmtf_model* h, ObsList& d, int n, int W, int KP, const std::vector<uint32_t>& ptr, const std::vector<uint32_t>& idx,
                         const std::vector<float>& val, const double* lambda) {
  d.n = n; d.W = W; d.stride = KP; d.ldT = round_up(n + 1, 64);          // (a zero behind every column of the transposed forms: the sweep's empty slots gather it)
  CHK(upload(&d.ptr, ptr, h->stream));
  CHK(upload(&d.idx, idx, h->stream));
  CHK(upload(&d.val, val, h->stream));
  if (lambda) {
    std::vector<float> lam((size_t)n * KP, 0.f);
    for (int u = 0; u < n; ++u)
      for (int k = 0; k < W; ++k) lam[(size_t)u * KP + k] = (float)lambda[(size_t)u * W + k];
    CHK(upload(&d.lambda, lam, h->stream));
  }
  CHK(dalloc(&d.X, (size_t)n * KP));
  CHK(dalloc(&d.XT, (size_t)W * d.ldT));
  if (lambda) {
    CHK(dalloc(&d.numer, (size_t)n, false));
    CHK(dalloc(&d.taup, (size_t)n, false));
  }
  for (int u = 0; u < n; ++u) {
    const uint32_t c = ptr[u + 1] - ptr[u];
    d.longest = std::max(d.longest, c);
    if (c > (uint32_t)kObsMaxSlots * 64u) d.long_units++;
  }
  return BNMTF_OK;
}

// fp64 host [n][W] -> fp32 device [n][stride] and [W][ldT]
static int obs_put(bnmtf_model* h, ObsList& d, const double* src) {
  const int W = d.W, KP = d.stride;
  std::vector<float> x((size_t)d.n * KP, 0.f), xt((size_t)W * d.ldT, 0.f);
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < W; ++k) {
      const float v = (float)src[(size_t)u * W + k];
      x[(size_t)u * KP + k] = v; xt[(size_t)k * d.ldT + u] = v;
    }
  HIPCHK(hipMemcpyAsync(d.X, x.data(), x.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.XT, xt.data(), xt.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

// a direction's variational buffers; with_S2T: the transposed second moment a two-factor half sweep gathers from the other
// direction (a tri-factorisation gathers its effective factor's instead)
static int obs_alloc_q(bnmtf_model* h, ObsList& d, bool with_S2T) {
  const size_t nk = (size_t)d.n * h->obs->stride;
  if (!d.mu) CHK(dalloc(&d.mu, nk));
  if (!d.tauq) CHK(dalloc(&d.tauq, nk));
  if (!d.var) CHK(dalloc(&d.var, nk));
  if (with_S2T && !d.S2T) CHK(dalloc(&d.S2T, (size_t)d.W * d.ldT));
  if (!d.vstat) CHK(dalloc(&d.vstat, (size_t)obs_sweep_blocks(d.n) * 6));
  return BNMTF_OK;
}

// fp64 host [n][W] x 4 -> the direction's fp32 q: mu, tau, var [n][stride]; the expectation in X / XT; where the direction owns
// an S2T, S2 = var + exp^2 there
static int obs_put_q(bnmtf_model* h, ObsList& d, const double* mu, const double* tau, const double* ex, const double* var) {
  const int W = d.W, KP = h->obs->stride;
  const size_t nk = (size_t)d.n * KP;
  std::vector<float> m(nk, 0.f), t(nk, 0.f), v(nk, 0.f), s2(d.S2T ? (size_t)W * d.ldT : 0, 0.f);
  for (int u = 0; u < d.n; ++u)
    for (int k = 0; k < W; ++k) {
      const size_t src = (size_t)u * W + k, at = (size_t)u * KP + k;
      m[at] = (float)mu[src]; t[at] = (float)tau[src]; v[at] = (float)var[src];
      if (d.S2T) {
        const float e = (float)ex[src];
        s2[(size_t)k * d.ldT + u] = fmaf(e, e, v[at]);            // (as the sweep forms it)
      }
    }
  CHK(obs_put(h, d, ex));
  HIPCHK(hipMemcpyAsync(d.mu, m.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.tauq, t.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d.var, v.data(), nk * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (d.S2T) HIPCHK(hipMemcpyAsync(d.S2T, s2.data(), s2.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return BNMTF_OK;
}

// The common part of bnmtf_obs_create / bnmtf_otri_create (the callers have checked their arguments): the lists, the model, its
// stream, the state with both directions and the scalars.  The handle is the guard's from the moment it exists: every way out of
// a create but release(), an exception included, destroys it.  bnmtf_onp_create (np): null prior rates, the columns' factor at
// a stride of its own and the marker; its half sweeps' partial sums are eight wide and its own.
struct ObsCreateGuard {
  bnmtf_model* h = nullptr;
  ~ObsCreateGuard() { if (h) bnmtf_destroy(h); }
  bnmtf_model* release() { bnmtf_model* r = h; h = nullptr; return r; }
};
static int obs_create_common(ObsCreateGuard& guard, int I, int J, int K, int L, int stride, uint64_t n, const int32_t* rows, const int32_t* cols,
                             const float* values, const double* lambda_rows, const double* lambda_cols, double alpha, double beta,
                             uint64_t seed, int device, bool np = false, int stride_cols = 0) {
  ObsLists ls;
  CHK(obs_lists(I, J, n, rows, cols, values, ls));
  HIPCHK(hipSetDevice(device));
  bnmtf_model* h = new bnmtf_model();
  guard.h = h;
  const int Wc = L > 0 ? L : K;
  h->I = I; h->J = J; h->K = K; h->L = L; h->device = device;
  h->alpha = alpha; h->beta = beta; h->seed = seed;
  h->n_obs = (double)n; h->sumR = ls.sumR; h->sumR2 = ls.sumR2;
  h->rows.nglob = I; h->rows.m = J; h->rows.W = K; h->cols.nglob = J; h->cols.m = I; h->cols.W = Wc;
  h->std_built = false;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; set_error("hipStreamCreate failed"); return BNMTF_EHIP; }
  h->obs = new ObsState();
  ObsState* s = h->obs;
  s->n = (size_t)n; s->stride = stride; s->np = np;
  const char* fl = getenv("BNMTF_OBS_LONG");
  s->force_long = fl && fl[0] == '1';
  CHK(obs_build_dir(h, s->rows, I, K, stride, ls.rptr, ls.ridx, ls.rval, lambda_rows));
  CHK(obs_build_dir(h, s->cols, J, Wc, stride_cols > 0 ? stride_cols : stride, ls.cptr, ls.cidx, ls.cval, lambda_cols));
  CHK(dalloc(&s->escratch, (size_t)n, false));
  if (!np) CHK(dalloc(&s->part, (size_t)obs_sweep_blocks(J) * 4, false));
  CHK(dalloc(&s->scal, 16));
  h->tau_d = s->scal; h->tau_f = reinterpret_cast<float*>(s->scal + 1); s->out8 = s->scal + 8;
  return BNMTF_OK;
}

// What a half sweep reads of its other operand: row major [m][stride], transposed [.][ldT] (ldT > m: word m of every column is
// zero) and, for the variational sweeps, the second moment transposed.  Two factors: the other direction's list itself.
struct ObsOther { const float* X; const float* XT; const float* S2T; int ldT, m; };
static ObsOther obs_other(bnmtf_model* h, bool rows) {
  const ObsList& o = rows ? h->obs->cols : h->obs->rows;
  return ObsOther{o.X, o.XT, o.S2T, o.ldT, o.n};
}

// the half sweep of a direction (rows: U or F) against `o`
static ObsSweepArgs obs_sweep_args(bnmtf_model* h, bool rows, const ObsOther& o, int mode) {
  ObsState* s = h->obs;
  ObsList& d = rows ? s->rows : s->cols;
  ObsSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = o.m; a.K = d.W; a.KP = s->stride;
  a.mode = mode; a.cond_k = -1; a.force_long = s->force_long ? 1 : 0; a.min_x = h->cur_min_x;
  a.lambda = d.lambda;
  a.X = d.X; a.XT = d.XT; a.ldT = d.ldT;
  a.Xo = o.X; a.XoT = o.XT; a.ldT_o = o.ldT;
  a.escratch = s->escratch;
  a.tau = h->tau_f;
  a.key0 = (uint32_t)h->seed; a.key1 = (uint32_t)(h->seed >> 32); a.it = (uint32_t)h->iteration;
  a.stream = rows ? kStreamRows : kStreamCols;
  return a;
}

// ... and the variational one (S2T: null where the direction owns none).  A tri-factorisation's caller adds its order and
// covariance fields and takes XT out: its instantiation writes neither transposed form.
static ObsVbSweepArgs obs_vb_sweep_args(bnmtf_model* h, bool rows, const ObsOther& o) {
  ObsState* s = h->obs;
  ObsList& d = rows ? s->rows : s->cols;
  ObsVbSweepArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d.ptr; a.idx = d.idx; a.val = d.val;
  a.n = d.n; a.m = o.m; a.K = d.W; a.KP = s->stride;
  a.only_k = -1; a.moments = 1; a.force_long = s->force_long ? 1 : 0;
  a.lambda = d.lambda;
  a.X = d.X; a.XT = d.XT; a.S2T = d.S2T; a.ldT = d.ldT;
  a.mu = d.mu; a.tauq = d.tauq; a.var = d.var;
  a.Xo = o.X; a.XoT = o.XT; a.S2oT = o.S2T; a.ldT_o = o.ldT;
  a.escratch = s->escratch;
  a.tau = h->tau_f;
  return a;
}

// tau and the record of iteration `it` of a run call, from the second half sweep's final residual
static ObsFinishArgs obs_finish_args(bnmtf_model* h, int update, int it) {
  ObsFinishArgs f; memset(&f, 0, sizeof(f));
  f.part = h->obs->part; f.nb = obs_sweep_blocks(h->J);
  f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
  f.update = update; f.gunit = update == BNMTF_UPDATE_DRAW ? h->gunit + it : nullptr;
  f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->rec + (size_t)it * 5;
  return f;
}
// ... and the variational finish's: update_tau, update_exp_tau and the record
static ObsVbFinishArgs obs_vb_finish_args(bnmtf_model* h, int it) {
  ObsState* s = h->obs;
  ObsVbFinishArgs f; memset(&f, 0, sizeof(f));
  f.stat_r = s->rows.vstat; f.nb_r = obs_sweep_blocks(h->I);
  f.stat_c = s->cols.vstat; f.part = s->part; f.nb_c = obs_sweep_blocks(h->J);
  f.n_obs = h->n_obs; f.sumR = h->sumR; f.sumR2 = h->sumR2; f.alpha = h->alpha; f.beta = h->beta;
  f.tau_d = h->tau_d; f.tau_f = h->tau_f; f.rec = h->vb_rec + (size_t)it * 16;
  return f;
}

// the sampler's record [n_iter][5] of a finished run call: tau, then MSE, R^2, Rp
static int obs_fetch_rec(bnmtf_model* h, int n_iter, double* tau_out, double* perf_out) {
  std::vector<double> rec((size_t)n_iter * 5);
  HIPCHK(hipMemcpy(rec.data(), h->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int it = 0; it < n_iter; ++it) {
    if (tau_out) tau_out[it] = rec[(size_t)it * 5];
    if (perf_out) for (int m = 0; m < 3; ++m) perf_out[(size_t)it * 3 + m] = rec[(size_t)it * 5 + 1 + m];
  }
  return BNMTF_OK;
}

// the cond_params hook of a direction: (numer, tau) of column k for the state the device holds, which stays as it is
static int obs_cond_params_dir(bnmtf_model* h, ObsList& d, ObsSweepArgs a, int k, double* numer_out, double* tau_out) {
  a.cond_k = k; a.numer_out = d.numer; a.tau_out = d.taup;
  launch_obs_sweep(a, h->stream);
  HIPCHK(hipMemcpyAsync(numer_out, d.numer, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tau_out, d.taup, sizeof(double) * d.n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
}

// the held-out launch pair of iteration `it` of a run call, behind the iteration's finish kernel on the handle's stream: the six
// sums of the factors the iteration ends with (a variational handle: the expectations) over the list of bnmtf_set_heldout_entries.
// No list: nothing is launched.
static void obs_heldout_enqueue(bnmtf_model* h, int it) {
  if (!h->held_n) return;
  ObsState* s = h->obs;
  ObsHeldoutArgs a; memset(&a, 0, sizeof(a));
  a.rowptr = h->held_rowptr; a.col = h->held_col; a.rval = h->held_val;
  a.A = s->rows.X; a.B = s->cols.X; a.I = h->I; a.K = h->K; a.stride = s->stride;
  a.part = h->held_part; a.rec = h->held_rec + (size_t)it * 8;
  launch_obs_heldout(a, h->stream);
}

// the six sums of metrics_from_sums of A B^T (A [I][W], B [J][W], fp64) over a list of entries in any order
static int obs_list_metric(bnmtf_model* h, const char* fn, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                           const double* A, const double* B, int W, double sums_out[6]) {
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("%s: between 1 and 2^31 - 1 entries (n=%llu)", fn, (unsigned long long)n); return BNMTF_EINVAL; }
  for (uint64_t e = 0; e < n; ++e)
    if (rows[e] < 0 || rows[e] >= h->I || cols[e] < 0 || cols[e] >= h->J) {
      set_error("%s: entry %llu (%d, %d) lies outside the %d x %d matrix", fn, (unsigned long long)e, rows[e], cols[e], h->I, h->J);
      return BNMTF_EINVAL;
    }
  const size_t nA = (size_t)h->I * W, nB = (size_t)h->J * W;
  DevBuf<uint32_t> dr, dc; DevBuf<float> dv; DevBuf<double> dA, dB, part;
  CHK(dr.alloc(n)); CHK(dc.alloc(n)); CHK(dv.alloc(n));
  CHK(dA.alloc(nA)); CHK(dB.alloc(nB)); CHK(part.alloc((size_t)obs_metric_blocks(n) * 8));
  HIPCHK(hipMemcpyAsync(dr.p, rows, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));      // (checked non-negative: the same bits as uint32)
  HIPCHK(hipMemcpyAsync(dc.p, cols, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dv.p, values, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dA.p, A, nA * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dB.p, B, nB * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ObsMetricArgs a; memset(&a, 0, sizeof(a));
  a.row = dr.p; a.col = dc.p; a.val = dv.p; a.n = (size_t)n; a.A = dA.p; a.B = dB.p; a.K = W; a.part = part.p;
  launch_obs_metric(a, h->obs->out8, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  double out8[8];
  HIPCHK(hipMemcpy(out8, h->obs->out8, sizeof(out8), hipMemcpyDeviceToHost));
  for (int m = 0; m < 6; ++m) sums_out[m] = out8[m];
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_obs_create(int I, int J, int K, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                     const double* lambda_rows, const double* lambda_cols, double alpha, double beta, uint64_t seed, int device,
                     bnmtf_handle* out) try {
  if (!out) { set_error("bnmtf_obs_create: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!rows || !cols || !values || !lambda_rows || !lambda_cols) { set_error("bnmtf_obs_create: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > BNMTF_OBS_MAX_RANK) {
    set_error("bnmtf_obs_create: unsupported shape I=%d J=%d K=%d (1 <= K <= %d)", I, J, K, BNMTF_OBS_MAX_RANK);
    return BNMTF_EINVAL;
  }
  ObsCreateGuard guard;
  CHK(obs_create_common(guard, I, J, K, 0, round_up(K, 4), n, rows, cols, values, lambda_rows, lambda_cols, alpha, beta, seed, device));
  bnmtf_model* h = guard.h;
  ObsState* s = h->obs;
  char buf[512];
  snprintf(buf, sizeof(buf), "bnmf layout=observed I=%d J=%d K=%d entries=%llu (%.3g %% of the matrix) longest_row=%u longest_column=%u "
           "long_form_units=%zu/%zu force_long=%d", I, J, K, (unsigned long long)n, 100.0 * (double)n / ((double)I * (double)J),
           s->rows.longest, s->cols.longest, s->rows.long_units, s->cols.long_units, (int)s->force_long);
  h->description = buf;
  *out = guard.release();
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_obs_build_lists(int I, int J, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                          uint32_t* row_ptr, uint32_t* row_col, float* row_val, uint32_t* col_ptr, uint32_t* col_row, float* col_val) try {
  if (!rows || !cols || !values) { set_error("bnmtf_obs_build_lists: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1) { set_error("bnmtf_obs_build_lists: unsupported shape I=%d J=%d", I, J); return BNMTF_EINVAL; }
  ObsLists ls;
  CHK(obs_lists(I, J, n, rows, cols, values, ls));
  if (row_ptr) memcpy(row_ptr, ls.rptr.data(), ls.rptr.size() * sizeof(uint32_t));
  if (row_col) memcpy(row_col, ls.ridx.data(), ls.ridx.size() * sizeof(uint32_t));
  if (row_val) memcpy(row_val, ls.rval.data(), ls.rval.size() * sizeof(float));
  if (col_ptr) memcpy(col_ptr, ls.cptr.data(), ls.cptr.size() * sizeof(uint32_t));
  if (col_row) memcpy(col_row, ls.cidx.data(), ls.cidx.size() * sizeof(uint32_t));
  if (col_val) memcpy(col_val, ls.cval.data(), ls.cval.size() * sizeof(float));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_set_state(bnmtf_handle h, const double* U, const double* V, double tau) try {
  CHK(obs_check(h, false, kObsNoState));
  if (!U || !V) { set_error("bnmf_obs_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(obs_put(h, h->obs->rows, U));
  CHK(obs_put(h, h->obs->cols, V));
  CHK(set_tau(h, tau));
  h->have_state = true;
  h->obs->vb_state = false;          // (the expectations were replaced: a variational state ends here)
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_get_state(bnmtf_handle h, double* U, double* V, double* tau) try {
  CHK(obs_check(h, false, kObsSamplerState));
  ObsState* s = h->obs;
  if (U) CHK(download_matrix(h, s->rows.X, h->I, h->K, s->stride, U));
  if (V) CHK(download_matrix(h, s->cols.X, h->J, h->K, s->stride, V));
  if (tau) {
    HIPCHK(hipMemcpyAsync(tau, h->tau_d, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_run(bnmtf_handle h, int n_iter, int update, float* U_out, float* V_out, double* tau_out, double* perf_out,
                 double* times_out) try {
  CHK(obs_check(h, false, kObsSamplerState));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (update < 0 || update > BNMTF_UPDATE_ICM) { set_error("unknown update rule"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsState* s = h->obs;
  CHK(ensure_rec(h, (size_t)n_iter));
  CHK(heldout_begin(h, n_iter));
  const int mode = update == BNMTF_UPDATE_DRAW ? kSweepDraw : kSweepMode;
  h->cur_min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
  if (mode == kSweepDraw) CHK(stage_gamma_variates(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  SampleSink sink;
  sink.add(s->rows.X, h->I, h->K, s->stride, U_out);
  sink.add(s->cols.X, h->J, h->K, s->stride, V_out);
  CHK(sink.begin(h, n_iter));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(sink.open_slot(it));
    ObsSweepArgs a = obs_sweep_args(h, true, obs_other(h, true), mode);
    a.snap = sink.slot_for(it, s->rows.X);
    launch_obs_sweep(a, h->stream);
    a = obs_sweep_args(h, false, obs_other(h, false), mode);
    a.snap = sink.slot_for(it, s->cols.X);
    a.part = s->part;
    launch_obs_sweep(a, h->stream);
    launch_obs_finish(obs_finish_args(h, update, it), h->stream);
    CHK(sink.close_slot(it));
    obs_heldout_enqueue(h, it);
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  CHK(sink.finish());
  HIPCHK(hipGetLastError());
  heldout_end(h, n_iter);
  CHK(obs_fetch_rec(h, n_iter, tau_out, perf_out));
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_obs_cond_params(bnmtf_handle h, int which, int k, double* numer_out, double* tau_out) try {
  CHK(obs_check(h, false, kObsSamplerState));
  if (which != 0 && which != 1) { set_error("bnmf_obs_cond_params: which is 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  if (k < 0 || k >= h->K) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  if (!numer_out || !tau_out) { set_error("bnmf_obs_cond_params: null argument"); return BNMTF_EINVAL; }
  const bool rows = which == 0;
  return obs_cond_params_dir(h, rows ? h->obs->rows : h->obs->cols, obs_sweep_args(h, rows, obs_other(h, rows), kSweepDraw), k, numer_out, tau_out);
} BNMTF_ABI_GUARD

int bnmf_obs_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                         const double* A, const double* B, double sums_out[6]) try {
  CHK(obs_check(h, false, kObsNoState));
  if (!rows || !cols || !values || !A || !B || !sums_out) { set_error("bnmf_obs_metric_sums: null argument"); return BNMTF_EINVAL; }
  return obs_list_metric(h, "bnmf_obs_metric_sums", n, rows, cols, values, A, B, h->K, sums_out);
} BNMTF_ABI_GUARD

// run(M_test=Entries) of the two-factor models on this layout: the held-out entries with their values, in any order, onto the
// handle (the row-sorted list bnmtf_set_heldout builds from a dense mask; this handle has no dense R to pick the values from)
int bnmtf_set_heldout_entries(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values) try {
  if (!h) { set_error("bnmtf_set_heldout_entries: null handle"); return BNMTF_EINVAL; }
  if (!h->obs || h->obs->np || obs_is_tri(h)) {
    set_error("bnmtf_set_heldout_entries: a call of the two-factor handle of bnmtf_obs_create (bnmf_obs_run, bnmf_vbo_run); this is a handle of %s",
              !h->obs ? (h->np ? "bnmtf_np_create" : "bnmtf_create: it takes a mask, bnmtf_set_heldout") : h->obs->np ? "bnmtf_onp_create" : "bnmtf_otri_create");
    return BNMTF_EINVAL;
  }
  CHK(obs_check(h, false, kObsNoState));
  const bool clear = n == 0 || !rows || !cols || !values;
  std::vector<uint32_t> ptr, idx; std::vector<float> val;
  if (!clear) {
    if (n >= ((uint64_t)1 << 31)) { set_error("bnmtf_set_heldout_entries: at most 2^31 - 1 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
    for (uint64_t e = 0; e < n; ++e)
      if (rows[e] < 0 || rows[e] >= h->I || cols[e] < 0 || cols[e] >= h->J) {
        set_error("bnmtf_set_heldout_entries: entry %llu (%d, %d) lies outside the %d x %d matrix", (unsigned long long)e, rows[e], cols[e], h->I, h->J);
        return BNMTF_EINVAL;
      }
    const long long dup = obs_sort(n, rows, cols, values, h->I, h->J, ptr, idx, val);
    if (dup >= 0) {
      const int i = (int)(std::upper_bound(ptr.begin(), ptr.end(), (uint32_t)dup) - ptr.begin()) - 1;
      set_error("bnmtf_set_heldout_entries: the entry (%d, %u) occurs twice (position %lld of the sorted list)", i, idx[(size_t)dup], dup);
      return BNMTF_EINVAL;
    }
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  heldout_free(h);
  if (clear) return BNMTF_OK;
  auto build = [&]() -> int {
    CHK(upload(&h->held_rowptr, ptr, h->stream));
    CHK(upload(&h->held_col, idx, h->stream));
    CHK(upload(&h->held_val, val, h->stream));
    CHK(dalloc(&h->held_part, (size_t)heldout_blocks(h->I) * 8));
    return BNMTF_OK;
  };
  int rc;
  try { rc = build(); } catch (...) { heldout_free(h); throw; }      // (a build that fails midway, by a status or by an exception, leaves no list behind)
  if (rc != BNMTF_OK) { heldout_free(h); return rc; }
  h->held_n = (size_t)n;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"

// ---- the variational two-factor model on the handle's lists (kernel_obs_vb.hip; DESIGN.md section 2.7) -----------------------
namespace bnmtf {

static int vbo_alloc(bnmtf_model* h) {
  ObsState* s = h->obs;
  if (s->vb_alloc) return BNMTF_OK;
  CHK(obs_alloc_q(h, s->rows, true));
  CHK(obs_alloc_q(h, s->cols, true));
  if (!s->esd_part) CHK(dalloc(&s->esd_part, (size_t)obs_vb_esd_blocks(h->I)));
  s->vb_alloc = true;
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmf_vbo_set_state(bnmtf_handle h, const double* muU, const double* tauU, const double* expU, const double* varU,
                       const double* muV, const double* tauV, const double* expV, const double* varV, double exptau) try {
  CHK(obs_check(h, false, kObsNoState));
  if (!muU || !tauU || !expU || !varU || !muV || !tauV || !expV || !varV) { set_error("bnmf_vbo_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(vbo_alloc(h));
  h->obs->vb_state = false;
  CHK(obs_put_q(h, h->obs->rows, muU, tauU, expU, varU));
  CHK(obs_put_q(h, h->obs->cols, muV, tauV, expV, varV));
  CHK(set_tau(h, exptau));
  h->have_state = true;
  h->obs->vb_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_get_state(bnmtf_handle h, double* muU, double* tauU, double* expU, double* varU,
                       double* muV, double* tauV, double* expV, double* varV) try {
  CHK(obs_check(h, false, kObsVbState));
  ObsState* s = h->obs;
  ObsList& r = s->rows; ObsList& c = s->cols;
  if (muU) CHK(download_matrix(h, r.mu, h->I, h->K, s->stride, muU));
  if (tauU) CHK(download_matrix(h, r.tauq, h->I, h->K, s->stride, tauU));
  if (expU) CHK(download_matrix(h, r.X, h->I, h->K, s->stride, expU));
  if (varU) CHK(download_matrix(h, r.var, h->I, h->K, s->stride, varU));
  if (muV) CHK(download_matrix(h, c.mu, h->J, h->K, s->stride, muV));
  if (tauV) CHK(download_matrix(h, c.tauq, h->J, h->K, s->stride, tauV));
  if (expV) CHK(download_matrix(h, c.X, h->J, h->K, s->stride, expV));
  if (varV) CHK(download_matrix(h, c.var, h->J, h->K, s->stride, varV));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_run(bnmtf_handle h, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out) try {
  CHK(obs_check(h, false, kObsVbState));
  if (n_iter < 0) { set_error("negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  ObsState* s = h->obs;
  CHK(vb_reserve_rec(h, n_iter));
  CHK(heldout_begin(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    ObsVbSweepArgs a = obs_vb_sweep_args(h, true, obs_other(h, true));
    a.stat = s->rows.vstat;
    launch_obs_vb_sweep(a, h->stream);
    a = obs_vb_sweep_args(h, false, obs_other(h, false));
    a.stat = s->cols.vstat; a.part = s->part;
    launch_obs_vb_sweep(a, h->stream);
    launch_obs_vb_finish(obs_vb_finish_args(h, it), h->stream);
    obs_heldout_enqueue(h, it);
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
    h->iteration++;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 16);
  HIPCHK(hipMemcpy(rec.data(), h->vb_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_vb_rec(rec.data(), n_iter, exptau_out, perf_out, elbo_terms_out);
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_update(bnmtf_handle h, int which, int k, int moments) try {
  CHK(obs_check(h, false, kObsVbState));
  if (which != 0 && which != 1) { set_error("bnmf_vbo_update: which is 0 (rows) or 1 (columns)"); return BNMTF_EINVAL; }
  if (k < 0 || k >= h->K) { set_error("column %d out of range", k); return BNMTF_EINVAL; }
  ObsVbSweepArgs a = obs_vb_sweep_args(h, which == 0, obs_other(h, which == 0));
  a.only_k = k; a.moments = moments ? 1 : 0;
  launch_obs_vb_sweep(a, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_vbo_exp_square_diff(bnmtf_handle h, double* out) try {
  CHK(obs_check(h, false, kObsVbState));
  if (!out) { set_error("bnmf_vbo_exp_square_diff: null argument"); return BNMTF_EINVAL; }
  ObsState* s = h->obs;
  ObsVbEsdArgs a; memset(&a, 0, sizeof(a));
  a.ptr = s->rows.ptr; a.idx = s->rows.idx; a.val = s->rows.val; a.n = h->I; a.K = h->K; a.KP = s->stride;
  a.X = s->rows.X; a.var = s->rows.var; a.Xo = s->cols.X; a.varo = s->cols.var; a.part = s->esd_part;
  launch_obs_vb_esd(a, s->out8, h->stream);
  HIPCHK(hipMemcpyAsync(out, s->out8, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
