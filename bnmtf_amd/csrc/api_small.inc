// Host side of the one-launch path for small models (kernel_small.hip): eligibility and layout at bnmtf_create, state
// hand-off, the run call for one model or a batch of models, and the switch-over to / from the multi-launch path.
// Included by api.hip.
namespace bnmtf {

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// One direction's entry-thread layout: unit u's missing inner indices dealt to g_u = ceil(cnt_u / em) consecutive entry threads
// (em = the smallest slot class -- 8, 16, 32, 40, 48, 64 -- with <= 1024 threads in all).  WHICH entry of the unit sits in which (thread, slot) is free, and
// a slot's gather reads LDS word 33 j + k: the 64 lanes of a wave hit 64 different banks iff their j differ mod 64.  So the slots
// are filled row by row (slot e of every thread of a wave), each thread taking an entry of its unit whose residue j mod 64 no
// lane of the wave has taken in this row yet, if there is one (random placement: ~4.5 lanes per busiest bank and read).
// idx holds 33 j (the factor row's first word; 33 m = the zero row), 16 bits.
struct SmallPlan {
  int n = 0, m = 0, em = 0, nthreads = 0;
  std::vector<uint16_t> idx, unit_of, seg;
  std::vector<uint32_t> sid;            // [I * J] slot id (e * 1024 + t) of every missing entry in this direction's layout
  bool ok = false;
};
static SmallPlan small_plan(const uint8_t* M, int I, int J, bool by_rows) {
  SmallPlan p;
  p.n = by_rows ? I : J; p.m = by_rows ? J : I;
  std::vector<std::vector<uint16_t>> miss(p.n);
  for (int i = 0; i < I; ++i)
    for (int j = 0; j < J; ++j)
      if (!M[(size_t)i * J + j]) { if (by_rows) miss[i].push_back((uint16_t)j); else miss[j].push_back((uint16_t)i); }
  for (int em : {8, 16, 32, 40, 48, 64}) {
    size_t tot = 0;
    for (int u = 0; u < p.n; ++u) tot += (miss[u].size() + em - 1) / em;
    if (tot <= (size_t)kSmallThreads) { p.em = em; p.nthreads = (int)tot; break; }
  }
  if (!p.em) return p;
  p.idx.assign((size_t)p.em * kSmallThreads, (uint16_t)(p.m * kSmallStride));
  p.unit_of.assign(kSmallThreads, 0);
  p.seg.assign((size_t)p.n * 2, 0);
  p.sid.assign((size_t)I * J, kSmallNone);
  std::vector<int> need(kSmallThreads, 0);          // entries thread t still has to take
  int t0 = 0;
  for (int u = 0; u < p.n; ++u) {
    const int cnt = (int)miss[u].size(), g = (cnt + p.em - 1) / p.em;
    p.seg[2 * u] = (uint16_t)t0; p.seg[2 * u + 1] = (uint16_t)g;
    for (int x = 0; x < g; ++x) { p.unit_of[t0 + x] = (uint16_t)u; need[t0 + x] = cnt / g + (x < cnt % g ? 1 : 0); }
    t0 += g;
  }
  for (int e = 0; e < p.em; ++e)
    for (int w0 = 0; w0 < p.nthreads; w0 += 64) {
      uint64_t used = 0;
      for (int t = w0; t < std::min(w0 + 64, p.nthreads); ++t) {
        if (need[t] == 0) continue;
        std::vector<uint16_t>& pool = miss[p.unit_of[t]];
        size_t pick = pool.size() - 1;
        for (size_t x = pool.size(); x-- > 0;) if (!((used >> (pool[x] & 63)) & 1ull)) { pick = x; break; }
        const uint16_t j = pool[pick];
        pool[pick] = pool.back(); pool.pop_back();
        used |= 1ull << (j & 63);
        --need[t];
        p.idx[(size_t)e * kSmallThreads + t] = (uint16_t)(j * kSmallStride);
        const int u = p.unit_of[t];
        const size_t cell = by_rows ? (size_t)u * J + j : (size_t)j * J + u;
        p.sid[cell] = (uint32_t)(e * kSmallThreads + t);
      }
    }
  p.ok = true;
  return p;
}

static void small_free(bnmtf_model* h) {
  if (!h->small) return;
  if (h->small->arena && h->stream) {
    (void)hipStreamSynchronize(h->stream);
    if (device_pool().give(h->device, h->small->arena_bytes, h->small->arena)) h->small->arena = nullptr;
  }
  dfree(h->small->arena); dfree(h->small->call_buf); dfree(h->small->smp);
  if (h->small->state_host) (void)hipHostFree(h->small->state_host);
  if (h->one_arena) {        // (they lived in the arena)
    h->Rfull = nullptr; h->Mtrain = nullptr; h->out6 = nullptr; h->tau_d = nullptr; h->tau_f = nullptr; h->acc = nullptr;
    h->exp_rows = h->exp_cols = h->exp_S = h->exp_tau = nullptr; h->Ad = h->Bd = nullptr;
  }
  delete h->small;
  h->small = nullptr;
}

// bnmtf_create: is this a model for the one-launch path?  (BNMF, one GPU, K <= 32, both dimensions <= 1024, every direction's
// missing entries in <= 1024 entry threads of <= 32 slots, factors + exchange areas within one CU's LDS.)  If so: its arena.
static int small_build(bnmtf_model* h, const float* R, const uint8_t* M) {
  if (const char* e = getenv("BNMTF_SMALL")) if (atoi(e) == 0) return BNMTF_OK;
  // (a switch of the multi-launch path's sweep kernels is set: whoever set it means that path)
  for (const char* v : {"BNMTF_WIDE", "BNMTF_HANDOVER", "BNMTF_TURNS", "BNMTF_TWIN", "BNMTF_FAST_NW", "BNMTF_SPLIT"}) if (getenv(v)) return BNMTF_OK;
  const int I = h->I, J = h->J, K = h->K, Lt = h->L;          // Lt > 0: tri-factorisation (rows = F: I x K, cols = G: J x L, S: K x L)
  const int Wc = Lt > 0 ? Lt : K;
  if (Lt > 0) if (const char* e = getenv("BNMTF_SMALL_TRI")) if (atoi(e) == 0) return BNMTF_OK;
  if (K > kSmallKP || Wc > kSmallKP || I > kSmallThreads || J > kSmallThreads || small_lds_bytes(I, J, kSmallThreads, K, Lt) > 160 * 1024) return BNMTF_OK;
  CreateLaps laps;
  SmallPlan pr = small_plan(M, I, J, true), pc = small_plan(M, I, J, false);
  if (!pr.ok || !pc.ok) return BNMTF_OK;
  laps.lap("  small: entry-thread layouts (host)");

  auto r64 = [](int v) { return (v + 63) & ~63; };
  const int ldbR = r64(I), ldbC = r64(J), m4R = (J + 31) & ~31, m4C = (I + 31) & ~31;      // (operand rows in steps of 32: kernel_small.hip small_contract)
  // arena: static part (filled on the host, one upload), then the state (zeroed)
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
  const size_t o_bigR = take((size_t)m4R * ldbR * 4), o_bigC = take((size_t)m4C * ldbC * 4);
  const size_t o_lamR = take((size_t)I * 32 * 4), o_lamC = take((size_t)J * 32 * 4);
  const size_t o_idxR = take(pr.idx.size() * 2), o_idxC = take(pc.idx.size() * 2);
  const size_t o_unR = take(kSmallThreads * 2), o_unC = take(kSmallThreads * 2);
  const size_t o_segR = take(pr.seg.size() * 2), o_segC = take(pc.seg.size() * 2);
  const size_t o_permR = take((size_t)pr.em * kSmallThreads * 4), o_permC = take((size_t)pc.em * kSmallThreads * 4);
  const size_t o_lamS = take((size_t)std::max(K * Lt, 1) * 4);
  const size_t static_bytes = off;
  const size_t o_XR = take((size_t)I * 32 * 4), o_XC = take((size_t)J * 32 * 4);
  const size_t o_XTR = take((size_t)32 * ldbR * 4), o_XTC = take((size_t)32 * ldbC * 4), o_PT = take((size_t)32 * ldbC * 4);
  const size_t o_qR = take((size_t)pr.em * kSmallThreads * 4), o_qC = take((size_t)pc.em * kSmallThreads * 4);
  const size_t o_C64R = take(1024 * 8), o_C64C = take(1024 * 8), o_csR = take(32 * 8), o_csC = take(32 * 8);
  const size_t o_tabR = take((size_t)32 * kSmallThreads * 8), o_tabC = take((size_t)32 * kSmallThreads * 8);     // K nc0 ldn <= 32 * 1024 entries
  // ... and what bnmtf_create and the first calls of other entry points would allocate one by one (a model search builds and
  // frees a model per candidate: every hipMalloc / hipFree is ~0.1-0.5 ms): the full matrix, the mask and the scalars, the
  // posterior sums, the metric kernel's factor operands
  const size_t o_exR = take((size_t)(I + 1) * 32 * 8), o_exC = take((size_t)(J + 1) * 32 * 8), o_exS = take((size_t)(K * Lt + 2) * 8);
  const size_t o_S = take((size_t)std::max(K * Lt, 1) * 4), o_ZT = take(Lt > 0 ? (size_t)32 * std::max(ldbR, ldbC) * 4 : 4), o_stab = take((size_t)std::max(K * Lt, 1) * 4 * 8);
  const size_t o_Wg = take(Lt > 0 ? (size_t)J * 56 * 4 : 4);
  const size_t dyn_end = off;
  const size_t o_Ad = take((size_t)I * 64 * 8), o_Bd = take((size_t)J * 64 * 8);
  const size_t o_R = take((size_t)I * J * 4), o_M = take((size_t)I * J), o_sc = take(256);
  const size_t total = off;

  std::vector<char> st(static_bytes, 0);
  float* bigR = reinterpret_cast<float*>(st.data() + o_bigR); float* bigC = reinterpret_cast<float*>(st.data() + o_bigC);
  for (int i = 0; i < I; ++i)
    for (int j = 0; j < J; ++j)
      if (M[(size_t)i * J + j]) { const float v = R[(size_t)i * J + j]; bigR[(size_t)j * ldbR + i] = v; bigC[(size_t)i * ldbC + j] = v; }
  float* lamR = reinterpret_cast<float*>(st.data() + o_lamR); float* lamC = reinterpret_cast<float*>(st.data() + o_lamC);
  for (int i = 0; i < I; ++i) for (int k = 0; k < K; ++k) lamR[i * 32 + k] = (float)h->lam_rows[(size_t)i * K + k];
  for (int j = 0; j < J; ++j) for (int k = 0; k < Wc; ++k) lamC[j * 32 + k] = (float)h->lam_cols[(size_t)j * Wc + k];
  if (Lt > 0) { float* lamS = reinterpret_cast<float*>(st.data() + o_lamS); for (int t = 0; t < K * Lt; ++t) lamS[t] = (float)h->lam_S[t]; }
  memcpy(st.data() + o_idxR, pr.idx.data(), pr.idx.size() * 2); memcpy(st.data() + o_idxC, pc.idx.data(), pc.idx.size() * 2);
  memcpy(st.data() + o_unR, pr.unit_of.data(), kSmallThreads * 2); memcpy(st.data() + o_unC, pc.unit_of.data(), kSmallThreads * 2);
  memcpy(st.data() + o_segR, pr.seg.data(), pr.seg.size() * 2); memcpy(st.data() + o_segC, pc.seg.data(), pc.seg.size() * 2);
  // where the OTHER direction keeps the q of each of this direction's slots
  uint32_t* permR = reinterpret_cast<uint32_t*>(st.data() + o_permR); uint32_t* permC = reinterpret_cast<uint32_t*>(st.data() + o_permC);
  for (size_t t = 0; t < (size_t)pr.em * kSmallThreads; ++t) permR[t] = kSmallNone;
  for (size_t t = 0; t < (size_t)pc.em * kSmallThreads; ++t) permC[t] = kSmallNone;
  for (size_t c = 0; c < (size_t)I * J; ++c)
    if (pr.sid[c] != kSmallNone) { permR[pr.sid[c]] = pc.sid[c]; permC[pc.sid[c]] = pr.sid[c]; }

  laps.lap("  small: operands, tables (host staging)");
  SmallModel* sm = new SmallModel();
  h->small = sm;
  sm->arena = static_cast<char*>(device_pool().take(h->device, total));
  if (!sm->arena) HIPCHK(hipMalloc((void**)&sm->arena, total));
  h->pool_stream = true;                     // (a small model's stream goes back to the pool, too)
  laps.lap("  small: arena (pool or hipMalloc)");
  sm->arena_bytes = total;
  HIPCHK(hipMemcpyAsync(sm->arena, st.data(), static_bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(sm->arena + static_bytes, 0, dyn_end - static_bytes, h->stream));
  HIPCHK(hipMemsetAsync(sm->arena + o_sc, 0, 256, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));                 // (st is a local)
  laps.lap("  small: upload + memsets");
  char* a = sm->arena;
  h->Rfull = reinterpret_cast<float*>(a + o_R); h->Mtrain = reinterpret_cast<uint8_t*>(a + o_M);
  h->out6 = reinterpret_cast<double*>(a + o_sc); h->tau_d = h->out6 + 8; h->acc = h->out6 + 12; h->tau_f = reinterpret_cast<float*>(h->out6 + 16);
  h->exp_rows = reinterpret_cast<double*>(a + o_exR); h->exp_cols = reinterpret_cast<double*>(a + o_exC);
  h->exp_S = reinterpret_cast<double*>(a + o_exS); h->exp_tau = h->exp_S + K * Lt + 1;
  h->Ad = reinterpret_cast<double*>(a + o_Ad); h->Bd = reinterpret_cast<double*>(a + o_Bd);
  h->one_arena = true;
  SmallLaunch& L = sm->dev;
  memset(&L, 0, sizeof(L));
  auto fill = [&](SmallDirDev& d, const SmallPlan& p, int ldb, size_t obig, size_t olam, size_t oidx, size_t oun, size_t oseg, size_t operm,
                  size_t oX, size_t oXT, size_t oq, size_t oC, size_t ocs, size_t otab) {
    d.n = p.n; d.m = p.m; d.ldb = ldb; d.ldn = ldb; d.nthreads = p.nthreads; d.em = p.em;
    d.big = reinterpret_cast<const float*>(a + obig); d.lambda = reinterpret_cast<const float*>(a + olam);
    d.idx = reinterpret_cast<const uint16_t*>(a + oidx); d.unit_of = reinterpret_cast<const uint16_t*>(a + oun);
    d.seg = reinterpret_cast<const uint16_t*>(a + oseg); d.perm = reinterpret_cast<const uint32_t*>(a + operm);
    d.X = reinterpret_cast<float*>(a + oX); d.XT = reinterpret_cast<float*>(a + oXT); d.q = reinterpret_cast<float*>(a + oq);
    d.C64 = reinterpret_cast<double*>(a + oC); d.colsum = reinterpret_cast<double*>(a + ocs); d.tab = reinterpret_cast<uint2*>(a + otab);
  };
  fill(L.rows, pr, ldbR, o_bigR, o_lamR, o_idxR, o_unR, o_segR, o_permR, o_XR, o_XTR, o_qR, o_C64R, o_csR, o_tabR);
  fill(L.cols, pc, ldbC, o_bigC, o_lamC, o_idxC, o_unC, o_segC, o_permC, o_XC, o_XTC, o_qC, o_C64C, o_csC, o_tabC);
  L.PT = reinterpret_cast<float*>(a + o_PT);
  L.L = Lt;
  if (Lt > 0) {
    L.S = reinterpret_cast<float*>(a + o_S); L.lambdaS = reinterpret_cast<const float*>(a + o_lamS);
    L.ZT = reinterpret_cast<float*>(a + o_ZT); L.stab = reinterpret_cast<uint2*>(a + o_stab);
    L.Wg = reinterpret_cast<float*>(a + o_Wg);
  }
  L.K = K; L.n_obs = h->n_obs; L.sumR = h->sumR; L.sumR2 = h->sumR2; L.alpha = h->alpha; L.beta = h->beta;
  L.tau_d = h->tau_d; L.tau_f = h->tau_f;
  sm->em = std::max(pr.em, pc.em);
  // threads per block: every unit and every entry thread of both directions (the smaller blocks run several to a CU)
  const int need = std::max(std::max(ldbR, ldbC), std::max(pr.nthreads, pc.nthreads));
  sm->nt = (need <= 256 && sm->em <= 32) ? 256 : ((need <= 512 && sm->em <= 32) ? 512 : 1024);
  sm->lds_bytes = small_lds_bytes(I, J, sm->nt, K, Lt);
  return BNMTF_OK;
}

// state hand-off: factors as [n][32] fp32 (the layout the multi-launch path keeps for K <= 32, too)
// (tri-factorisation: U = F [I][K], V = G [J][L], S [K][L] as on the multi-launch path)
static int small_upload_state(bnmtf_model* h, const double* U, const double* V, const double* S = nullptr) {
  SmallModel* sm = h->small;
  const int K = h->K, Wc = h->L > 0 ? h->L : h->K;
  std::vector<float> tmp((size_t)(h->I + h->J) * 32 + (size_t)K * h->L, 0.f);
  for (int i = 0; i < h->I; ++i) for (int k = 0; k < K; ++k) tmp[(size_t)i * 32 + k] = (float)U[(size_t)i * K + k];
  for (int j = 0; j < h->J; ++j) for (int k = 0; k < Wc; ++k) tmp[(size_t)(h->I + j) * 32 + k] = (float)V[(size_t)j * Wc + k];
  HIPCHK(hipMemcpyAsync(sm->dev.rows.X, tmp.data(), (size_t)h->I * 32 * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(sm->dev.cols.X, tmp.data() + (size_t)h->I * 32, (size_t)h->J * 32 * 4, hipMemcpyHostToDevice, h->stream));
  if (h->L > 0) {
    float* sf = tmp.data() + (size_t)(h->I + h->J) * 32;
    for (int t = 0; t < K * h->L; ++t) sf[t] = (float)S[t];
    HIPCHK(hipMemcpyAsync(sm->dev.S, sf, (size_t)K * h->L * 4, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  sm->q_valid = false;
  h->small_cur = true;
  return BNMTF_OK;
}
static int small_download_state(bnmtf_model* h, double* U, double* V, double* S = nullptr) {
  SmallModel* sm = h->small;
  const int K = h->K, Wc = h->L > 0 ? h->L : h->K;
  std::vector<float> tmp((size_t)(h->I + h->J) * 32 + (size_t)K * h->L);
  HIPCHK(hipMemcpyAsync(tmp.data(), sm->dev.rows.X, (size_t)h->I * 32 * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(tmp.data() + (size_t)h->I * 32, sm->dev.cols.X, (size_t)h->J * 32 * 4, hipMemcpyDeviceToHost, h->stream));
  if (S && h->L > 0) HIPCHK(hipMemcpyAsync(tmp.data() + (size_t)(h->I + h->J) * 32, sm->dev.S, (size_t)K * h->L * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (U) for (int i = 0; i < h->I; ++i) for (int k = 0; k < K; ++k) U[(size_t)i * K + k] = (double)tmp[(size_t)i * 32 + k];
  if (V) for (int j = 0; j < h->J; ++j) for (int k = 0; k < Wc; ++k) V[(size_t)j * Wc + k] = (double)tmp[(size_t)(h->I + j) * 32 + k];
  if (S && h->L > 0) for (int t = 0; t < K * h->L; ++t) S[t] = (double)tmp[(size_t)(h->I + h->J) * 32 + t];
  return BNMTF_OK;
}

// The multi-launch path is about to be used: build its structures if this model has lived on the small path so far, and hand
// it the current state if the small path holds it.
static int ensure_std(bnmtf_model* h) {
  if (h->np) { set_error("a handle of bnmtf_np_create runs only the bnmf_np_* / bnmtf_np_* calls"); return BNMTF_EINVAL; }
  CHK(refuse_obs(h, nullptr));
  if (!h->std_built) {
    HIPCHK(hipSetDevice(h->device));
    CHK(build_standard(h, h->L > 0 ? h->lam_S.data() : nullptr, nullptr));
    describe_model(h);
  }
  if (h->small && h->small_cur && !h->std_cur && h->have_state) {
    // [n][32] fp32 on both sides (K <= 32): device-to-device, then the relayout + Gram the other path's sweeps read
    HIPCHK(hipMemcpyAsync(h->rows.X, h->small->dev.rows.X, (size_t)h->I * 32 * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->cols.X, h->small->dev.cols.X, (size_t)h->J * 32 * 4, hipMemcpyDeviceToDevice, h->stream));
    if (h->L > 0) HIPCHK(hipMemcpyAsync(h->S, h->small->dev.S, (size_t)h->K * h->L * 4, hipMemcpyDeviceToDevice, h->stream));
    enqueue_post(h, h->rows); enqueue_post(h, h->cols);
    h->std_cur = true;
    h->ho_regions_current = false;
  }
  return BNMTF_OK;
}
static int ensure_small_state(bnmtf_model* h) {
  if (h->small_cur || !h->std_cur) return BNMTF_OK;
  HIPCHK(hipMemcpyAsync(h->small->dev.rows.X, h->rows.X, (size_t)h->I * 32 * 4, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->small->dev.cols.X, h->cols.X, (size_t)h->J * 32 * 4, hipMemcpyDeviceToDevice, h->stream));
  if (h->L > 0) HIPCHK(hipMemcpyAsync(h->small->dev.S, h->S, (size_t)h->K * h->L * 4, hipMemcpyDeviceToDevice, h->stream));
  h->small->q_valid = false;
  h->small_cur = true;
  return BNMTF_OK;
}
// Does this run call go down the one-launch path?  `batch`: models (of the one-launch kind, on this device) the call runs
// together.  A block is one CU: a model that fills it (1024-thread blocks: GDSC's 622 x 138 at 19 % missing) runs ~2.5 x slower
// alone on its CU than on the multi-launch path with the whole chip to itself, and wins from three models per call on; the
// models of 256- and 512-thread blocks win alone, too (toy 100 x 80: 15.7 k against 11.2 k iterations/s).
// bnmtf_set_small_path: 0 never, 1 by this rule (default), 2 always.
static bool small_wanted(const bnmtf_model* h, int batch = 1) {
  if (!(h->small && h->small_mode != 0 && h->use_fast && h->profiling == 0)) return false;
  if (h->held_n) return false;               // a held-out mask (bnmtf_set_heldout): its kernel follows each iteration of the multi-launch loop
  if (h->small_mode == 2) return true;
  // (the tri-factorisation: alone, a model that fills a CU runs 4.0 k iterations/s here against 6.5 k on the multi-launch path with the
  // whole chip to itself (622 x 138, K = L = 10); two of them in one call are already ahead.  Ranks above 10 take the S step's
  // sequential form, ~2 us per entry of S on the block against ~0.3 us on the multi-launch path's chain (K = L = 16 at the toy size:
  // 2.4 k against 6.4 k iterations/s alone; K = L = 32: 0.6 k against 4.3 k): only in a batch that is worth that many entries)
  if (h->L > 0 && !small_tri_dense(h->K, h->L) && h->K * h->L > 80 * batch - 50) return false;
  return h->small->nt <= 512 || batch >= (h->L > 0 ? 2 : 3);
}

struct SmallOut { float* U; float* V; double* tau; double* perf; double* times; double* U_final = nullptr; double* V_final = nullptr; double* tau_final = nullptr;
                  float* S = nullptr; double* S_final = nullptr; };     // (tri-factorisation: U = F, V = G)

// n models (all small, all on one device), n_iter iterations each, ONE launch: block b runs model b
static int small_run_many(bnmtf_model* const* hs, int n, int n_iter, int update, const SmallOut* outs) {
  if (n <= 0 || n_iter <= 0) return BNMTF_OK;
  bnmtf_model* h0 = hs[0];
  HIPCHK(hipSetDevice(h0->device));
  hipStream_t st = h0->stream;
  // per-call buffers of the whole batch, owned by the first model: [launch descriptors | per model: gunit, rec, clock]
  const size_t per = al256((size_t)n_iter * 8) + al256((size_t)n_iter * 5 * 8) + al256((size_t)(n_iter + 1) * 8);
  const size_t o_models = al256((size_t)n * sizeof(SmallLaunch));
  const size_t need = o_models + (size_t)n * per;
  SmallModel* s0 = h0->small;
  if (s0->call_cap < need) { dfree(s0->call_buf); s0->call_cap = 0; HIPCHK(hipMalloc((void**)&s0->call_buf, need)); s0->call_cap = need; }
  std::vector<char> stage(o_models + (size_t)n * per, 0);
  SmallLaunch* Ls = reinterpret_cast<SmallLaunch*>(stage.data());
  int em = 8, nt = 256; size_t lds = 0;
  const bool draw = update == BNMTF_UPDATE_DRAW;
  for (int b = 0; b < n; ++b) {
    bnmtf_model* h = hs[b];
    if (!h->small || h->device != h0->device) { set_error("small_run_many: model %d is not a small model of device %d", b, h0->device); return BNMTF_EINVAL; }
    if ((h->L > 0) != (h0->L > 0)) { set_error("small_run_many: two- and three-factor models in one batch"); return BNMTF_EINVAL; }
    if (!h->have_state) { set_error("run before set_state (model %d)", b); return BNMTF_ESTATE; }
    if (h != h0 && hipStreamQuery(h->stream) != hipSuccess) { (void)hipGetLastError(); HIPCHK(hipStreamSynchronize(h->stream)); }   // (its uploads, if any are still on their way)
    if (!h->small_cur) { CHK(ensure_small_state(h)); HIPCHK(hipStreamSynchronize(h->stream)); }
    SmallModel* sm = h->small;
    SmallLaunch& L = Ls[b];
    L = sm->dev;
    char* mb = s0->call_buf + o_models + (size_t)b * per;
    L.gunit = reinterpret_cast<const double*>(mb);
    L.rec = reinterpret_cast<double*>(mb + al256((size_t)n_iter * 8));
    L.clock = reinterpret_cast<unsigned long long*>(mb + al256((size_t)n_iter * 8) + al256((size_t)n_iter * 5 * 8));
    L.n_iter = n_iter; L.update = update; L.min_x = update == BNMTF_UPDATE_ICM ? (float)h->min_tn : 0.f;
    L.key0 = (uint32_t)h->seed; L.key1 = (uint32_t)(h->seed >> 32); L.it0 = h->iteration;
    L.q_valid = sm->q_valid ? 1 : 0; L.refresh = (uint32_t)h->ho_refresh;
    L.U_s = L.V_s = L.S_s = nullptr;
    const int Wc = h->L > 0 ? h->L : h->K;
    if (outs[b].U || outs[b].V || outs[b].S) {
      const size_t fl = (size_t)n_iter * ((size_t)h->I * h->K + (size_t)h->J * Wc + (size_t)h->K * h->L);
      if (sm->smp_cap < fl) { dfree(sm->smp); sm->smp_cap = 0; HIPCHK(hipMalloc((void**)&sm->smp, fl * 4)); sm->smp_cap = fl; }
      if (outs[b].U) L.U_s = sm->smp;
      if (outs[b].V) L.V_s = sm->smp + (size_t)n_iter * h->I * h->K;
      if (outs[b].S) L.S_s = sm->smp + (size_t)n_iter * ((size_t)h->I * h->K + (size_t)h->J * Wc);
    }
    L.expR = L.expC = L.exp_tau = L.expS = nullptr; L.exp_burn = -1; L.exp_thin = 1;
    if (h->exp_burn >= 0) {
      HIPCHK(hipMemsetAsync(h->exp_rows, 0, sizeof(double) * h->I * 32, st));
      HIPCHK(hipMemsetAsync(h->exp_cols, 0, sizeof(double) * h->J * 32, st));
      HIPCHK(hipMemsetAsync(h->exp_tau, 0, sizeof(double), st));
      if (h->L > 0) { HIPCHK(hipMemsetAsync(h->exp_S, 0, sizeof(double) * h->K * h->L, st)); L.expS = h->exp_S; }
      L.expR = h->exp_rows; L.expC = h->exp_cols; L.exp_tau = h->exp_tau; L.exp_burn = h->exp_burn; L.exp_thin = h->exp_thin;
      h->exp_count = h->exp_burn < n_iter ? (uint64_t)((n_iter - 1 - h->exp_burn) / h->exp_thin + 1) : 0;
    }
    em = std::max(em, sm->em); nt = std::max(nt, sm->nt);
  }
  if (draw) {
    // the Gamma(alpha_s, 1) variates of every (model, iteration): they depend on the seed and the iteration number only, so
    // the fp64 Marsaglia-Tsang loops run on the host -- 256 models x 1 000 iterations are 256 k of them: on all host cores
    parallel_chunks(n * n_iter, 2048, [&](int a, int b_) {
      for (int t = a; t < b_; ++t) {
        const int b = t / n_iter, it = t - b * n_iter;
        const bnmtf_model* h = hs[b];
        double* g = reinterpret_cast<double*>(stage.data() + o_models + (size_t)b * per);
        g[it] = gamma_unit_draw(h->alpha + 0.5 * h->n_obs, (uint32_t)(h->iteration + it), kStreamTau, (uint32_t)h->seed, (uint32_t)(h->seed >> 32));
      }
    });
  }
  HIPCHK(hipMemcpyAsync(s0->call_buf, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
  for (int b = 0; b < n; ++b) lds = std::max(lds, small_lds_bytes(hs[b]->I, hs[b]->J, nt, hs[b]->K, hs[b]->L));
  launch_small_gibbs(reinterpret_cast<const SmallLaunch*>(s0->call_buf), n, em, nt, lds, st, h0->L > 0);
  HIPCHK(hipMemcpyAsync(stage.data(), s0->call_buf, stage.size(), hipMemcpyDeviceToHost, st));
  for (int b = 0; b < n; ++b) {
    bnmtf_model* h = hs[b];
    if (outs[b].U) HIPCHK(hipMemcpyAsync(outs[b].U, Ls[b].U_s, (size_t)n_iter * h->I * h->K * 4, hipMemcpyDeviceToHost, st));
    if (outs[b].V) HIPCHK(hipMemcpyAsync(outs[b].V, Ls[b].V_s, (size_t)n_iter * h->J * (h->L > 0 ? h->L : h->K) * 4, hipMemcpyDeviceToHost, st));
    if (outs[b].S) HIPCHK(hipMemcpyAsync(outs[b].S, Ls[b].S_s, (size_t)n_iter * h->K * h->L * 4, hipMemcpyDeviceToHost, st));
  }
  // the state every model ends with (what get_state would fetch model by model, each with its own synchronisation): one
  // page-locked staging buffer of the first model, every copy asynchronous, one synchronisation for all
  size_t state_floats = 0;
  std::vector<size_t> state_off(n, 0);
  for (int b = 0; b < n; ++b)
    if (outs[b].U_final || outs[b].V_final || outs[b].S_final) { state_off[b] = state_floats; state_floats += (size_t)(hs[b]->I + hs[b]->J) * 32 + (size_t)hs[b]->K * hs[b]->L; }
  if (state_floats) {
    if (s0->state_host_cap < state_floats) {
      if (s0->state_host) (void)hipHostFree(s0->state_host);
      s0->state_host = nullptr; s0->state_host_cap = 0;
      HIPCHK(hipHostMalloc((void**)&s0->state_host, state_floats * sizeof(float), hipHostMallocDefault));
      s0->state_host_cap = state_floats;
    }
    for (int b = 0; b < n; ++b)
      if (outs[b].U_final || outs[b].V_final || outs[b].S_final) {
        bnmtf_model* h = hs[b];
        HIPCHK(hipMemcpyAsync(s0->state_host + state_off[b], h->small->dev.rows.X, (size_t)h->I * 32 * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s0->state_host + state_off[b] + (size_t)h->I * 32, h->small->dev.cols.X, (size_t)h->J * 32 * 4, hipMemcpyDeviceToHost, st));
        if (h->L > 0) HIPCHK(hipMemcpyAsync(s0->state_host + state_off[b] + (size_t)(h->I + h->J) * 32, h->small->dev.S, (size_t)h->K * h->L * 4, hipMemcpyDeviceToHost, st));
      }
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  for (int b = 0; b < n; ++b) {
    bnmtf_model* h = hs[b];
    if (outs[b].U_final || outs[b].V_final || outs[b].S_final) {
      const float* sp = s0->state_host + state_off[b];
      const int K = h->K, Wc = h->L > 0 ? h->L : h->K;
      if (outs[b].U_final) for (int i = 0; i < h->I; ++i) for (int k = 0; k < K; ++k) outs[b].U_final[(size_t)i * K + k] = (double)sp[(size_t)i * 32 + k];
      sp += (size_t)h->I * 32;
      if (outs[b].V_final) for (int j = 0; j < h->J; ++j) for (int k = 0; k < Wc; ++k) outs[b].V_final[(size_t)j * Wc + k] = (double)sp[(size_t)j * 32 + k];
      sp += (size_t)h->J * 32;
      if (outs[b].S_final) for (int t = 0; t < K * h->L; ++t) outs[b].S_final[t] = (double)sp[t];
    }
    const char* mb = stage.data() + o_models + (size_t)b * per;
    const double* rec = reinterpret_cast<const double*>(mb + al256((size_t)n_iter * 8));
    const unsigned long long* clk = reinterpret_cast<const unsigned long long*>(mb + al256((size_t)n_iter * 8) + al256((size_t)n_iter * 5 * 8));
    for (int it = 0; it < n_iter; ++it) {
      if (outs[b].tau) outs[b].tau[it] = rec[(size_t)it * 5];
      if (outs[b].perf) for (int m = 0; m < 3; ++m) outs[b].perf[(size_t)it * 3 + m] = rec[(size_t)it * 5 + 1 + m];
      if (outs[b].times) outs[b].times[it] = (double)(clk[it + 1] - clk[0]) * 1e-8;      // wall_clock64: 100 MHz
    }
    if (outs[b].tau_final) *outs[b].tau_final = rec[(size_t)(n_iter - 1) * 5];
    h->iteration += (uint64_t)n_iter;
    h->small->q_valid = true;
    h->small_cur = true; h->std_cur = false;
    h->ho_regions_current = false;
  }
  return BNMTF_OK;
}

}  // namespace bnmtf
