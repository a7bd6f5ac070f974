// Held-out performance per iteration (run(M_test=)): the mask's entries as a row-sorted device list, the hooks the run loops call
// (heldout_begin / heldout_enqueue / heldout_end) and the two entry points bnmtf_set_heldout / bnmtf_get_heldout.  The kernel:
// kernel_heldout.hip.  Included by api.hip.
namespace bnmtf {

static void heldout_free(bnmtf_model* h) {
  dfree(h->held_rowptr); dfree(h->held_col); dfree(h->held_val); dfree(h->held_part); dfree(h->held_rec);
  h->held_n = 0; h->held_rec_cap = 0; h->held_iters = 0;
}

// a run call of n_iter iterations begins: room for its record (no mask: the handle holds no record of this call)
static int heldout_begin(bnmtf_model* h, int n_iter) {
  h->held_iters = 0;
  if (!h->held_n) return BNMTF_OK;
  if (h->held_rec_cap < (size_t)n_iter) {
    dfree(h->held_rec); h->held_rec_cap = 0;
    CHK(dalloc(&h->held_rec, (size_t)n_iter * 8));
    h->held_rec_cap = (size_t)n_iter;
  }
  return BNMTF_OK;
}

// behind the last kernel of iteration `it` of the call, on the stream that ran it: the sums of the state the iteration ends with.
// While a Recorder is installed (a lock-step run_many) the pair is recorded behind the iteration's records; its arguments are then
// the same bytes in every iteration.  A handle of bnmtf_np_create: np_heldout_enqueue (api_np.inc).
static void heldout_enqueue(bnmtf_model* h, int it, hipStream_t st) {
  if (!h->held_n) return;
  HeldoutArgs a;
  memset(&a, 0, sizeof(a));                              // (padding too: a recorded list compares argument bytes)
  a.rowptr = h->held_rowptr; a.col = h->held_col; a.rval = h->held_val; a.I = h->I;
  a.A = h->rows.X; a.KPa = h->rows.KP; a.Wa = h->rows.W;
  a.B = h->cols.X; a.KPb = h->cols.KP; a.Wb = h->cols.W;
  a.S = h->L > 0 ? h->S : nullptr; a.K = h->K; a.L = h->L;
  a.part = h->held_part; a.rec = g_recorder ? h->held_rec : h->held_rec + (size_t)it * 8;
  launch_heldout(a, st);
}

// the call has drained its streams
static void heldout_end(bnmtf_model* h, int n_iter) {
  if (h->held_n) h->held_iters = n_iter;
}

// the one-launch *_gibbs_run_many entry points take no model with a mask (their kernel has no per-iteration hook)
static int heldout_refuse_many(const bnmtf_model* h, const char* entry, int b) {
  if (!h->held_n) return BNMTF_OK;
  set_error("%s: model %d has a held-out mask (bnmtf_set_heldout): clear it, or run the model by its own run call", entry, b);
  return BNMTF_EINVAL;
}

}  // namespace bnmtf

extern "C" {

int bnmtf_set_heldout(bnmtf_handle h, const double* M_test) try {
  if (!h) { set_error("bnmtf_set_heldout: null handle"); return BNMTF_EINVAL; }
  CHK(refuse_obs(h, "bnmtf_set_heldout"));
  if (h->world > 1) { set_error("bnmtf_set_heldout: a sharded model (world = %d) keeps no held-out record: one GPU only", h->world); return BNMTF_EINVAL; }
  if (h->block_mode) { set_error("bnmtf_set_heldout: a block of a wider factorisation keeps no held-out record"); return BNMTF_EINVAL; }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  heldout_free(h);
  if (!M_test) return BNMTF_OK;
  const int I = h->I, J = h->J;
  std::vector<uint32_t> rowptr((size_t)I + 1, 0), col;
  for (int i = 0; i < I; ++i) {
    const double* m = M_test + (size_t)i * J;
    for (int j = 0; j < J; ++j) if (m[j] != 0.0) col.push_back((uint32_t)j);
    rowptr[(size_t)i + 1] = (uint32_t)col.size();
  }
  if (col.empty()) { set_error("bnmtf_set_heldout: the mask has no entries"); return BNMTF_EINVAL; }
  int rc = BNMTF_OK;
  auto build = [&]() -> int {
    CHK(dalloc(&h->held_rowptr, rowptr.size(), false));
    CHK(dalloc(&h->held_col, col.size(), false));
    CHK(dalloc(&h->held_val, col.size(), false));
    CHK(dalloc(&h->held_part, (size_t)heldout_blocks(I) * 8));
    HIPCHK(hipMemcpyAsync(h->held_rowptr, rowptr.data(), rowptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->held_col, col.data(), col.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    launch_heldout_values(h->Rfull, I, J, h->held_rowptr, h->held_col, h->held_val, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));      // (rowptr, col are this call's)
    HIPCHK(hipGetLastError());
    return BNMTF_OK;
  };
  if ((rc = build()) != BNMTF_OK) { heldout_free(h); return rc; }
  h->held_n = col.size();
  return BNMTF_OK;
} BNMTF_ABI_GUARD

int bnmtf_get_heldout(bnmtf_handle h, int n_iter, double* sums_out) try {
  if (!h || !sums_out || n_iter < 0) { set_error("bnmtf_get_heldout: null argument or negative count"); return BNMTF_EINVAL; }
  if (!h->held_n) { set_error("bnmtf_get_heldout: no held-out mask set"); return BNMTF_ESTATE; }
  if (n_iter > h->held_iters) { set_error("bnmtf_get_heldout: the last run call recorded %d iterations, %d asked for", h->held_iters, n_iter); return BNMTF_ESTATE; }
  if (n_iter == 0) return BNMTF_OK;
  HIPCHK(hipSetDevice(h->device));
  std::vector<double> rec((size_t)n_iter * 8);
  HIPCHK(hipMemcpy(rec.data(), h->held_rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int it = 0; it < n_iter; ++it)
    for (int m = 0; m < 6; ++m) sums_out[(size_t)it * 6 + m] = rec[(size_t)it * 8 + m];
  return BNMTF_OK;
} BNMTF_ABI_GUARD

}  // extern "C"
