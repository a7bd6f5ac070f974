// Fold new units into a fitted model (C ABI part 12: bnmtf_amd.fold_in, bnmtf_amd/fold_in.py; DESIGN.md section 2.10) -- included
// in api.hip behind api_top.inc, on which it does not depend.  bnmtf_fold_in takes no handle: the fixed
// factor in fp64 as the host holds it, the new units' entries as a list sorted by (unit, index), and per unit its prior rates, its
// start and its id.  Before its first device call it checks everything, makes the units' offsets and casts the fixed factor to fp32
// twice: row major with the row stride rounded up to four, and transposed with a zero word behind every column.  Then it makes a
// stream, three events and its buffers on the device, uploads, and launches launch_foldin (kernel_foldin.hip) once: every unit's
// whole chain.  Everything is owned by objects of this function: whichever way it leaves, nothing stays.

namespace bnmtf {

constexpr int kFoldInMaxDim = 1 << 30;               // m: an index and the zero word behind a column stay inside an int

}  // namespace bnmtf

extern "C" {

int bnmtf_fold_in(int device, int n_units, int m, int W, const double* other,
                  uint64_t n, const int32_t* unit, const int32_t* idx, const float* values,
                  const double* lambda, double tau, const double* init, const uint32_t* ids, uint64_t seed,
                  int iterations, int first_iteration, int discard, int keep_every, int update, double min_x, int form,
                  double* first_out, double* sum_d_out, double* sum_d2_out, float* samples_out) try {
  if (!other || !unit || !idx || !values || !lambda || !init || !first_out || !sum_d_out || !sum_d2_out) {
    set_error("bnmtf_fold_in: null argument");
    return BNMTF_EINVAL;
  }
  if (n_units < 1 || m < 1 || m > kFoldInMaxDim || W < 1 || W > kFoldInMaxRank) {
    set_error("bnmtf_fold_in: unsupported shape n_units=%d m=%d W=%d (1 <= n_units, 1 <= m <= 2^30, 1 <= W <= %d: BNMTF_FOLDIN_MAX_RANK)", n_units, m, W, kFoldInMaxRank);
    return BNMTF_EINVAL;
  }
  if (n < 1 || n >= ((uint64_t)1 << 31)) { set_error("bnmtf_fold_in: 1 <= n < 2^31 entries (n=%llu)", (unsigned long long)n); return BNMTF_EINVAL; }
  if (n < (uint64_t)n_units) { set_error("bnmtf_fold_in: every unit needs an entry (%llu entries, %d units)", (unsigned long long)n, n_units); return BNMTF_EINVAL; }
  if (iterations < 1 || first_iteration < 0 || (long long)iterations + first_iteration > 0x7fffffffLL) {
    set_error("bnmtf_fold_in: iterations >= 1, first_iteration >= 0 and their sum below 2^31 (iterations=%d, first_iteration=%d)", iterations, first_iteration);
    return BNMTF_EINVAL;
  }
  if (update != 0 && update != 1) { set_error("bnmtf_fold_in: update is 0 (draw) or 1 (mode) (update=%d)", update); return BNMTF_EINVAL; }
  if (keep_every < 1) { set_error("bnmtf_fold_in: keep_every >= 1 (keep_every=%d)", keep_every); return BNMTF_EINVAL; }
  if (discard < 0 || discard >= iterations) { set_error("bnmtf_fold_in: 0 <= discard < iterations (discard=%d, iterations=%d)", discard, iterations); return BNMTF_EINVAL; }
  if (update == 1 && (discard != 0 || keep_every != 1)) {
    set_error("bnmtf_fold_in: a mode chain has one answer, its final state: discard = 0 and keep_every = 1 (discard=%d, keep_every=%d)", discard, keep_every);
    return BNMTF_EINVAL;
  }
  if (form != 0 && form != 1) { set_error("bnmtf_fold_in: form is 0 (by the unit's entry count) or 1 (the long form for every unit) (form=%d)", form); return BNMTF_EINVAL; }
  if (!(tau > 0.0) || !std::isfinite(tau) || !std::isfinite((float)tau)) { set_error("bnmtf_fold_in: tau is positive and finite (tau=%g)", tau); return BNMTF_EINVAL; }
  if (!(min_x >= 0.0) || !std::isfinite(min_x)) { set_error("bnmtf_fold_in: min_x is finite and not negative (min_x=%g)", min_x); return BNMTF_EINVAL; }

  // ---- the list: sorted by (unit, index), no entry twice, every unit at least once, every index inside the fixed factor
  std::vector<uint32_t> ptr((size_t)n_units + 1, 0u);
  for (uint64_t e = 0; e < n; ++e) {
    if (unit[e] < 0 || unit[e] >= n_units || idx[e] < 0 || idx[e] >= m) {
      set_error("bnmtf_fold_in: entry %llu (%d, %d) lies outside the %d units x %d indices", (unsigned long long)e, unit[e], idx[e], n_units, m);
      return BNMTF_EINVAL;
    }
    if (e > 0 && (unit[e] < unit[e - 1] || (unit[e] == unit[e - 1] && idx[e] <= idx[e - 1]))) {
      if (unit[e] == unit[e - 1] && idx[e] == idx[e - 1]) set_error("bnmtf_fold_in: entry %llu (%d, %d) is given twice", (unsigned long long)e, unit[e], idx[e]);
      else set_error("bnmtf_fold_in: the list is sorted by (unit, index): entry %llu (%d, %d) follows (%d, %d)", (unsigned long long)e, unit[e], idx[e], unit[e - 1], idx[e - 1]);
      return BNMTF_EINVAL;
    }
    if (!std::isfinite(values[e])) { set_error("bnmtf_fold_in: the value of entry %llu (%d, %d) is not finite", (unsigned long long)e, unit[e], idx[e]); return BNMTF_EINVAL; }
    ptr[(size_t)unit[e] + 1]++;
  }
  bool any_long = form == 1;
  for (int u = 0; u < n_units; ++u) {
    if (ptr[(size_t)u + 1] == 0) { set_error("bnmtf_fold_in: unit %d has no entry", u); return BNMTF_EINVAL; }
    if (ptr[(size_t)u + 1] > (uint32_t)kFoldInMaxSlots * 64u) any_long = true;
    ptr[(size_t)u + 1] += ptr[u];
  }

  // ---- finite values everywhere; the fixed factor, the rates and the start in fp32
  const int KP = round_up(W, 4), ldT = round_up(m + 1, 4);
  const size_t nW = (size_t)n_units * W;
  std::vector<float> Xo((size_t)m * KP, 0.f), XoT((size_t)W * ldT, 0.f), lam(nW), x0(nW);
  for (int j = 0; j < m; ++j)
    for (int k = 0; k < W; ++k) {
      const double b = other[(size_t)j * W + k];
      if (!std::isfinite(b) || !std::isfinite((float)b)) { set_error("bnmtf_fold_in: the fixed factor holds a value that is not finite in fp32 (row %d, column %d)", j, k); return BNMTF_EINVAL; }
      Xo[(size_t)j * KP + k] = (float)b; XoT[(size_t)k * ldT + j] = (float)b;
    }
  for (size_t t = 0; t < nW; ++t) {
    if (!(lambda[t] >= 0.0) || !std::isfinite((float)lambda[t])) { set_error("bnmtf_fold_in: the prior rates are finite and not negative (unit %d, column %d)", (int)(t / W), (int)(t % W)); return BNMTF_EINVAL; }
    if (!std::isfinite(init[t]) || !std::isfinite((float)init[t])) { set_error("bnmtf_fold_in: the start holds a value that is not finite (unit %d, column %d)", (int)(t / W), (int)(t % W)); return BNMTF_EINVAL; }
    lam[t] = (float)lambda[t]; x0[t] = (float)init[t];
  }
  std::vector<uint32_t> idu((size_t)n), own_ids;
  for (uint64_t e = 0; e < n; ++e) idu[e] = (uint32_t)idx[e];
  if (!ids) {
    own_ids.resize((size_t)n_units);
    for (int u = 0; u < n_units; ++u) own_ids[u] = (uint32_t)u;
  }
  const uint32_t* const use_ids = ids ? ids : own_ids.data();

  // ---- the device's side: all of it owned here
  CallScope cs;
  DevBuf<uint32_t> d_ptr, d_idx, d_ids;
  DevBuf<float> d_val, d_Xo, d_XoT, d_lam, d_x0, d_es, d_samples;
  DevBuf<double> d_stats;
  CHK(cs.open(device));
  const size_t nsamp = samples_out ? (size_t)iterations * nW : 0;
  CHK(d_ptr.alloc(ptr.size())); CHK(d_idx.alloc((size_t)n)); CHK(d_val.alloc((size_t)n)); CHK(d_ids.alloc((size_t)n_units));
  CHK(d_Xo.alloc(Xo.size())); CHK(d_XoT.alloc(XoT.size())); CHK(d_lam.alloc(nW)); CHK(d_x0.alloc(nW));
  CHK(d_es.alloc(any_long ? (size_t)n : 1));
  CHK(d_stats.alloc(3 * nW));
  if (nsamp) CHK(d_samples.alloc(nsamp));

  CHK(cs.mark(0));
  HIPCHK(hipMemcpyAsync(d_ptr.p, ptr.data(), ptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_idx.p, idu.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_val.p, values, (size_t)n * sizeof(float), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_ids.p, use_ids, (size_t)n_units * sizeof(uint32_t), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_Xo.p, Xo.data(), Xo.size() * sizeof(float), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_XoT.p, XoT.data(), XoT.size() * sizeof(float), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_lam.p, lam.data(), nW * sizeof(float), hipMemcpyHostToDevice, cs.s));
  HIPCHK(hipMemcpyAsync(d_x0.p, x0.data(), nW * sizeof(float), hipMemcpyHostToDevice, cs.s));
  CHK(cs.mark(1));

  FoldInArgs a; memset(&a, 0, sizeof(a));
  a.ptr = d_ptr.p; a.idx = d_idx.p; a.val = d_val.p;
  a.n = n_units; a.m = m; a.W = W; a.KP = KP;
  a.Xo = d_Xo.p; a.XoT = d_XoT.p; a.ldT = ldT;
  a.lambda = d_lam.p; a.init = d_x0.p; a.ids = d_ids.p;
  a.tau = (float)tau; a.min_x = (float)min_x;
  a.key0 = (uint32_t)seed; a.key1 = (uint32_t)(seed >> 32); a.it0 = (uint32_t)first_iteration;
  a.T = iterations;
  a.discard = update == 1 ? iterations - 1 : discard;          // (a mode chain: the final state is the one kept sweep)
  a.keep_every = keep_every;
  a.mode = update == 1 ? kSweepMode : kSweepDraw;
  a.force_long = form;
  a.escratch = d_es.p;
  a.stats = d_stats.p;
  a.samples = nsamp ? d_samples.p : nullptr;
  launch_foldin(a, cs.s);
  HIPCHK(hipGetLastError());
  CHK(cs.mark(2));
  HIPCHK(hipStreamSynchronize(cs.s));
  HIPCHK(hipGetLastError());
  double up = 0.0, kn = 0.0;
  CHK(cs.elapsed(&up, &kn));

  HIPCHK(hipMemcpy(first_out, d_stats.p, nW * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sum_d_out, d_stats.p + nW, nW * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(sum_d2_out, d_stats.p + 2 * nW, nW * sizeof(double), hipMemcpyDeviceToHost));
  if (nsamp) HIPCHK(hipMemcpy(samples_out, d_samples.p, nsamp * sizeof(float), hipMemcpyDeviceToHost));
  g_call_ms[kCallFoldIn][0] = up; g_call_ms[kCallFoldIn][1] = kn;
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_fold_in_times(double* upload_ms, double* kernel_ms) try {
  return call_times("bnmtf_fold_in_times", kCallFoldIn, upload_ms, kernel_ms);
} BNMTF_ABI_GUARD

}  // extern "C"
