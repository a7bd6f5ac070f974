// Non-probabilistic NMF / NMTF driver (C ABI part 5, nmf_np.py / nmtf_np.py) -- included at the end of api.hip.
// A handle of bnmtf_np_create holds R and the training mask on the device like any other handle (Rfull, Mtrain) and, in NpState,
// what the multiplicative updates need: the masked data in both layouts, the factors column major, S, the scratch of the
// products G S^T / (F S)^T, NMTF's P and the per-iteration records.  None of the samplers' layouts are built, so the ranks are
// not tied to wave lanes (K, L <= 256).  One GPU.

namespace bnmtf {

struct NpState {
  float* Rn = nullptr;      // [I][J] R where observed, NaN elsewhere
  float* RnT = nullptr;     // [J][I]
  float* Xr = nullptr;      // [K][I] U / F
  float* Xc = nullptr;      // [Kc][J] V / G  (Kc = K, or L for NMTF)
  float* S = nullptr;       // [K][L]
  float* S2 = nullptr;      // [K][L] the S step's output
  float* Y = nullptr;       // [max(K J, L I)] G S^T as [K][J] or (F S)^T as [L][I]
  float* P = nullptr;       // [I][J] NMTF's S step: P on the observed entries
  double* part = nullptr;   // [max blocks][8] per-block sums
  double* spart = nullptr;  // [2][S blocks][2] the S step's partials
  double* rec = nullptr; size_t rec_cap = 0;   // [iterations][8] the sums of each iteration
  uint8_t* Mp = nullptr;    // [I][J] predict()'s mask
  bool have_state = false;
};

static void np_free(bnmtf_model* h) {
  NpState* s = h->np;
  if (!s) return;
  dfree(s->Rn); dfree(s->RnT); dfree(s->Xr); dfree(s->Xc); dfree(s->S); dfree(s->S2); dfree(s->Y); dfree(s->P);
  dfree(s->part); dfree(s->spart); dfree(s->rec); dfree(s->Mp);
  delete s;
  h->np = nullptr;
}

static int np_check(bnmtf_model* h, bool tri, bool need_state) {
  if (!h || !h->np) { set_error("not a handle of bnmtf_np_create"); return BNMTF_EINVAL; }
  if (tri != (h->L > 0)) { set_error(tri ? "the NMTF calls need a handle with L > 0" : "the NMF calls need a handle with L = 0"); return BNMTF_EINVAL; }
  if (need_state && !h->np->have_state) { set_error("set_state has not been called"); return BNMTF_ESTATE; }
  HIPCHK(hipSetDevice(h->device));
  return BNMTF_OK;
}

// fp64 host [n][W] <-> fp32 device [W][n]
static int np_put(float* dst, const double* src, int n, int W, hipStream_t st) {
  std::vector<float> t((size_t)n * W);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < W; ++k) t[(size_t)k * n + i] = (float)src[(size_t)i * W + k];
  HIPCHK(hipMemcpyAsync(dst, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return BNMTF_OK;
}
static int np_get(double* dst, const float* src, int n, int W, hipStream_t st) {
  std::vector<float> t((size_t)n * W);
  HIPCHK(hipMemcpyAsync(t.data(), src, t.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < W; ++k) dst[(size_t)i * W + k] = (double)t[(size_t)k * n + i];
  return BNMTF_OK;
}

// MSE / R^2 / Rp of the eight sums (n, R, R^2, P, P^2, R P, I-div, SSE): _base.metrics_from_sums with the SSE summed directly
static void np_perf(const double* s, double* perf) {
  const double n = s[0], sr = s[1], srr = s[2], sp = s[3], spp = s[4], srp = s[5], sse = s[7];
  const double ss_tot = srr - sr * sr / n, cov = srp - sr * sp / n, vp = spp - sp * sp / n;
  perf[0] = sse / n;
  perf[1] = ss_tot != 0.0 ? 1.0 - sse / ss_tot : INFINITY;
  perf[2] = cov / (std::sqrt(std::max(ss_tot, 0.0)) * std::sqrt(std::max(vp, 0.0)));
}

// the half sweep of the rows (U / F: other factor Yt [W][J]) or of the columns (V / G: other factor Yt [W][I]), columns [k0, k1)
static void np_enqueue_sweep(bnmtf_model* h, bool rows, float* Xt, const float* Yt, int W, int k0, int k1, double* stats_out) {
  NpState* s = h->np;
  NpSweepArgs a; memset(&a, 0, sizeof(a));                   // (padding too: a recorded list compares argument bytes)
  a.Rn = rows ? s->Rn : s->RnT; a.n = rows ? h->I : h->J; a.m = rows ? h->J : h->I;
  a.Xt = Xt; a.Yt = Yt; a.K = W; a.k0 = k0; a.k1 = k1;
  a.stats = stats_out ? s->part : nullptr;
  launch_np_sweep(a, h->stream);
  if (stats_out) launch_np_stats_finish(s->part, np_sweep_blocks(a.n, a.m), stats_out, h->stream);
}

// NMTF products: Y = G S^T as [K][J] (the F step's other factor, the S step's P), or (F S)^T as [L][I] (the G step's)
static void np_gst(bnmtf_model* h) { NpState* s = h->np; launch_np_small_product(s->S, h->L, 1, s->Xc, h->L, h->K, h->J, s->Y, h->stream); }
static void np_fs(bnmtf_model* h) { NpState* s = h->np; launch_np_small_product(s->S, 1, h->L, s->Xr, h->K, h->L, h->I, s->Y, h->stream); }

// The launch sites of a recorded iteration (many.h: site_at; api_many.inc), as (phase, index): the records of the models of a batch
// are aligned by site, not by position -- phase 0 before the S step, phase 1 its passes (index = pass), phase 2 after it: (2, 0) S's
// copy, (2, 1) G S^T, (2, 2) the F sweep, (2, 3) (F S)^T, (2, 4) and (2, 5) the G sweep and its sums.  NMF's two sweeps meet NMTF's.
enum NpSite { kNpBeforeS, kNpSPass, kNpAfterS };

// S entries [e0, e1) in row-major order (nmtf_np.py:127-129 for the whole range), one pass per entry plus one that finishes
// the last; S2 receives the new values and becomes S.  Recorded (the whole range only): no copy of S into S2 beforehand --
// the passes finish every entry -- and S2 is copied back into S instead of the swap, so that the arguments of every
// iteration are the same.
static int np_s_step(bnmtf_model* h, int e0, int e1) {
  NpState* s = h->np;
  const int nb = np_s_blocks(h->I);
  const bool recording = g_recorder != nullptr;
  if (recording && (e0 != 0 || e1 != h->K * h->L)) { set_error("np_s_step: a recorded S step covers all of S"); return BNMTF_ESTATE; }
  site_at(kNpBeforeS);
  np_gst(h);
  launch_np_build_p(s->Rn, s->Xr, s->Y, h->I, h->J, h->K, s->P, h->stream);
  if (!recording) HIPCHK(hipMemcpyAsync(s->S2, s->S, (size_t)h->K * h->L * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  NpSPassArgs a; memset(&a, 0, sizeof(a));
  a.Rn = s->Rn; a.P = s->P; a.Ft = s->Xr; a.Gt = s->Xc; a.S_in = s->S; a.S_out = s->S2;
  a.I = h->I; a.J = h->J; a.K = h->K; a.L = h->L;
  for (int e = e0; e <= e1; ++e) {
    a.prev = e > e0 ? e - 1 : -1;
    a.cur = e < e1 ? e : -1;
    a.part_prev = s->spart + (size_t)((e + 1) & 1) * nb * 2;
    a.part_cur = s->spart + (size_t)(e & 1) * nb * 2;
    site_at(kNpSPass, e - e0);
    launch_np_s_pass(a, h->stream);
  }
  site_at(kNpAfterS);
  if (recording) record_np_copy(s->S2, s->S, h->K * h->L);
  else std::swap(s->S, s->S2);
  return BNMTF_OK;
}

// One iteration on h->stream -- or, while a Recorder is installed, into its records, each under its site (stats_out: then the
// run's first record; the list-form end-of-iteration kernel finds the iteration's own).
static int np_iteration(bnmtf_model* h, double* stats_out) {
  NpState* s = h->np;
  if (h->L == 0) {                                            // nmf_np.py:95-98
    site_at(kNpAfterS, 2);                                    // (the sites of NMTF's F and G sweeps)
    np_enqueue_sweep(h, true, s->Xr, s->Xc, h->K, 0, h->K, nullptr);
    site_at(kNpAfterS, 4);
    np_enqueue_sweep(h, false, s->Xc, s->Xr, h->K, 0, h->K, stats_out);
  } else {
    CHK(np_s_step(h, 0, h->K * h->L));                        // nmtf_np.py:127-135; the records behind it follow S's copy: (2, 1) ...
    np_gst(h);
    np_enqueue_sweep(h, true, s->Xr, s->Y, h->K, 0, h->K, nullptr);
    np_fs(h);
    np_enqueue_sweep(h, false, s->Xc, s->Y, h->L, 0, h->L, stats_out);
  }
  h->iteration++;
  return BNMTF_OK;
}

// The held-out sums (api_heldout.inc) of the factors iteration `it` of the call ends with, behind its last kernel -- or, while a
// Recorder is installed, recorded behind its records.  fp64 from the fp32 factors themselves, not through Y.
static void np_heldout_enqueue(bnmtf_model* h, int it) {
  if (!h->held_n) return;
  NpState* s = h->np;
  HeldoutNpArgs a; memset(&a, 0, sizeof(a));                  // (padding too: a recorded list compares argument bytes)
  a.rowptr = h->held_rowptr; a.col = h->held_col; a.rval = h->held_val;
  a.Xr = s->Xr; a.Xc = s->Xc; a.S = h->L > 0 ? s->S : nullptr;
  a.part = h->held_part; a.rec = g_recorder ? h->held_rec : h->held_rec + (size_t)it * 8;
  a.I = h->I; a.J = h->J; a.K = h->K; a.L = h->L;
  launch_heldout_np(a, h->stream);
}

// the record of n_iter iterations of 8 sums each; either output may be null
static void unpack_np_rec(const double* rec, int n_iter, double* perf, double* idiv) {
  for (int it = 0; it < n_iter; ++it) {
    if (perf) np_perf(rec + (size_t)it * 8, perf + (size_t)it * 3);
    if (idiv) idiv[it] = rec[(size_t)it * 8 + 6];
  }
}
// room on the device for the records of a run
static int np_reserve_rec(NpState* s, int n_iter) {
  if ((size_t)n_iter <= s->rec_cap) return BNMTF_OK;
  dfree(s->rec); s->rec_cap = 0;
  CHK(dalloc(&s->rec, (size_t)n_iter * 8, false));
  s->rec_cap = n_iter;
  return BNMTF_OK;
}

static int np_run(bnmtf_model* h, int n_iter, double* perf_out, double* idiv_out, double* times_out) {
  NpState* s = h->np;
  if (n_iter < 0) { set_error("run: negative iteration count"); return BNMTF_EINVAL; }
  if (n_iter == 0) return BNMTF_OK;
  CHK(np_reserve_rec(s, n_iter));
  CHK(heldout_begin(h, n_iter));
  EventList ev;
  CHK(ev.create(times_out ? n_iter + 1 : 0));
  if (times_out) HIPCHK(hipEventRecord(ev[0], h->stream));
  for (int it = 0; it < n_iter; ++it) {
    CHK(np_iteration(h, s->rec + (size_t)it * 8));
    np_heldout_enqueue(h, it);                   // (a mask set: on U, V or F, S, G of this iteration)
    if (times_out) HIPCHK(hipEventRecord(ev[it + 1], h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  heldout_end(h, n_iter);
  std::vector<double> rec((size_t)n_iter * 8);
  HIPCHK(hipMemcpy(rec.data(), s->rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unpack_np_rec(rec.data(), n_iter, perf_out, idiv_out);
  ev.seconds(n_iter, times_out);
  return BNMTF_OK;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_np_create(const float* R, const uint8_t* M, int I, int J, int K, int L, int device, bnmtf_handle* out) try {
  if (!out) { set_error("bnmtf_np_create: null argument"); return BNMTF_EINVAL; }
  *out = nullptr;
  if (!R || !M) { set_error("bnmtf_np_create: null argument"); return BNMTF_EINVAL; }
  if (I < 1 || J < 1 || K < 1 || K > BNMTF_NP_MAX_RANK || L < 0 || L > BNMTF_NP_MAX_RANK) {
    set_error("bnmtf_np_create: unsupported shape I=%d J=%d K=%d L=%d (1 <= K,L <= %d)", I, J, K, L, BNMTF_NP_MAX_RANK);
    return BNMTF_EINVAL;
  }
  const int Kc = L > 0 ? L : K;
  if (!np_sweep_supported(J, std::max(K, Kc)) || !np_sweep_supported(I, std::max(K, Kc))) {
    set_error("bnmtf_np_create: rows and columns of at most 16384 entries (I=%d J=%d)", I, J);
    return BNMTF_EINVAL;
  }
  double n_obs = 0, sR = 0, sR2 = 0;
  {
    std::vector<uint32_t> cc(J, 0);
    for (int i = 0; i < I; ++i) {
      uint32_t cnt = 0;
      for (int j = 0; j < J; ++j)
        if (M[(size_t)i * J + j]) { const double r = R[(size_t)i * J + j]; ++cnt; cc[j]++; sR += r; sR2 += r * r; }
      if (!cnt) { set_error("Fully unobserved row in R, row %d.", i); return BNMTF_EINVAL; }
      n_obs += cnt;
    }
    for (int j = 0; j < J; ++j) if (!cc[j]) { set_error("Fully unobserved column in R, column %d.", j); return BNMTF_EINVAL; }
  }
  HIPCHK(hipSetDevice(device));
  bnmtf_model* h = new bnmtf_model();
  h->I = I; h->J = J; h->K = K; h->L = L; h->device = device;
  h->n_obs = n_obs; h->sumR = sR; h->sumR2 = sR2;
  h->rows.nglob = I; h->rows.m = J; h->rows.W = K; h->cols.nglob = J; h->cols.m = I; h->cols.W = Kc;
  h->std_built = false;
  auto fail = [&](int rc) { bnmtf_destroy(h); return rc; };
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { h->stream = nullptr; set_error("hipStreamCreate failed"); return fail(BNMTF_EHIP); }
  h->np = new NpState();
  NpState* s = h->np;
  int rcode;
  {   // Rfull, Mtrain and the small scalars in one allocation, as bnmtf_create lays them out (bnmtf_destroy frees them so)
    const size_t bR = ((size_t)I * J * sizeof(float) + 255) & ~(size_t)255, bM = ((size_t)I * J + 255) & ~(size_t)255;
    char* base = nullptr;
    if ((rcode = dalloc(&base, bR + bM + 256, false))) return fail(rcode);
    h->Rfull = reinterpret_cast<float*>(base); h->Mtrain = reinterpret_cast<uint8_t*>(base + bR);
    h->out6 = reinterpret_cast<double*>(base + bR + bM); h->tau_d = h->out6 + 8; h->acc = h->out6 + 12; h->tau_f = reinterpret_cast<float*>(h->out6 + 16);
  }
  const size_t IJ = (size_t)I * J;
  if ((rcode = dalloc(&s->Rn, IJ, false)) || (rcode = dalloc(&s->RnT, IJ, false)) ||
      (rcode = dalloc(&s->Xr, (size_t)K * I)) || (rcode = dalloc(&s->Xc, (size_t)Kc * J)) ||
      (rcode = dalloc(&s->part, (size_t)std::max({np_sweep_blocks(I, J), np_sweep_blocks(J, I), I}) * 8, false)))
    return fail(rcode);
  if (L > 0) {
    if ((rcode = dalloc(&s->S, (size_t)K * L)) || (rcode = dalloc(&s->S2, (size_t)K * L)) ||
        (rcode = dalloc(&s->Y, std::max((size_t)K * J, (size_t)L * I))) || (rcode = dalloc(&s->P, IJ, false)) ||
        (rcode = dalloc(&s->spart, (size_t)2 * np_s_blocks(I) * 2)))
      return fail(rcode);
  }
  if (hipMemcpyAsync(h->Rfull, R, IJ * sizeof(float), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(h->Mtrain, M, IJ, hipMemcpyHostToDevice, h->stream) != hipSuccess) { set_error("bnmtf_np_create: uploads failed"); return fail(BNMTF_EHIP); }
  launch_np_prepare(h->Rfull, h->Mtrain, I, J, s->Rn, s->RnT, h->stream);
  if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess) { set_error("bnmtf_np_create: preparing the data failed"); return fail(BNMTF_EHIP); }
  h->description = L > 0 ? "nmtf_np" : "nmf_np";
  *out = h;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_np_set_state(bnmtf_handle h, const double* U, const double* V) try {
  CHK(np_check(h, false, false));
  if (!U || !V) { set_error("bnmf_np_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(np_put(h->np->Xr, U, h->I, h->K, h->stream));
  CHK(np_put(h->np->Xc, V, h->J, h->K, h->stream));
  h->np->have_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_np_get_state(bnmtf_handle h, double* U, double* V) try {
  CHK(np_check(h, false, true));
  if (U) CHK(np_get(U, h->np->Xr, h->I, h->K, h->stream));
  if (V) CHK(np_get(V, h->np->Xc, h->J, h->K, h->stream));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_np_update(bnmtf_handle h, int which, int k) try {
  CHK(np_check(h, false, true));
  if ((which != 0 && which != 1) || k < 0 || k >= h->K) { set_error("bnmf_np_update: which %d / column %d out of range", which, k); return BNMTF_EINVAL; }
  NpState* s = h->np;
  if (which == 0) np_enqueue_sweep(h, true, s->Xr, s->Xc, h->K, k, k + 1, nullptr);
  else np_enqueue_sweep(h, false, s->Xc, s->Xr, h->K, k, k + 1, nullptr);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmf_np_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out) try {
  CHK(np_check(h, false, true));
  return np_run(h, n_iter, perf_out, idiv_out, times_out);
} BNMTF_ABI_GUARD

int bnmtf_np_set_state(bnmtf_handle h, const double* F, const double* S, const double* G) try {
  CHK(np_check(h, true, false));
  if (!F || !S || !G) { set_error("bnmtf_np_set_state: null argument"); return BNMTF_EINVAL; }
  CHK(np_put(h->np->Xr, F, h->I, h->K, h->stream));
  CHK(np_put(h->np->Xc, G, h->J, h->L, h->stream));
  std::vector<float> s32((size_t)h->K * h->L);
  for (size_t q = 0; q < s32.size(); ++q) s32[q] = (float)S[q];
  HIPCHK(hipMemcpyAsync(h->np->S, s32.data(), s32.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->np->have_state = true;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_np_get_state(bnmtf_handle h, double* F, double* S, double* G) try {
  CHK(np_check(h, true, true));
  if (F) CHK(np_get(F, h->np->Xr, h->I, h->K, h->stream));
  if (G) CHK(np_get(G, h->np->Xc, h->J, h->L, h->stream));
  if (S) {
    std::vector<float> s32((size_t)h->K * h->L);
    HIPCHK(hipMemcpyAsync(s32.data(), h->np->S, s32.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t q = 0; q < s32.size(); ++q) S[q] = (double)s32[q];
  }
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_np_update(bnmtf_handle h, int which, int k, int l) try {
  CHK(np_check(h, true, true));
  const bool ok = (which == 0 && k >= 0 && k < h->K) || (which == 1 && k >= 0 && k < h->K && l >= 0 && l < h->L) || (which == 2 && l >= 0 && l < h->L);
  if (!ok) { set_error("bnmtf_np_update: which %d / entry (%d, %d) out of range", which, k, l); return BNMTF_EINVAL; }
  NpState* s = h->np;
  if (which == 0) { np_gst(h); np_enqueue_sweep(h, true, s->Xr, s->Y, h->K, k, k + 1, nullptr); }
  else if (which == 1) CHK(np_s_step(h, k * h->L + l, k * h->L + l + 1));
  else { np_fs(h); np_enqueue_sweep(h, false, s->Xc, s->Y, h->L, l, l + 1, nullptr); }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_np_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out) try {
  CHK(np_check(h, true, true));
  return np_run(h, n_iter, perf_out, idiv_out, times_out);
} BNMTF_ABI_GUARD

int bnmtf_np_metrics(bnmtf_handle h, const uint8_t* Mp, double* out) try {
  if (!h || !h->np) { set_error("not a handle of bnmtf_np_create"); return BNMTF_EINVAL; }
  CHK(np_check(h, h->L > 0, true));
  if (!out) { set_error("bnmtf_np_metrics: null argument"); return BNMTF_EINVAL; }
  NpState* s = h->np;
  const uint8_t* mask = h->Mtrain;
  if (Mp) {
    if (!s->Mp) CHK(dalloc(&s->Mp, (size_t)h->I * h->J, false));
    HIPCHK(hipMemcpyAsync(s->Mp, Mp, (size_t)h->I * h->J, hipMemcpyHostToDevice, h->stream));
    mask = s->Mp;
  }
  const float* Yt = s->Xc;
  if (h->L > 0) { np_gst(h); Yt = s->Y; }
  launch_np_metrics(h->Rfull, mask, s->Xr, Yt, h->I, h->J, h->K, s->part, h->stream);
  launch_np_stats_finish(s->part, h->I, h->out6, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, h->out6, 8 * sizeof(double), hipMemcpyDeviceToHost));
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
