/*
 * bnmtf_hip.h -- C ABI of libbnmtf_hip.so: the MI355X (gfx950) implementation of
 * the Gibbs / VB inference hot path of ThomasBrouwer/BNMTF.
 *
 * The reference has no FFI layer: its boundary is the duck-typed Python class
 * contract of code/models/ bnmf_gibbs_optimised.py, bnmtf_gibbs_optimised.py, bnmf_vb_optimised.py.
 * Each entry point below names the reference method(s) it replaces (file:line,
 * relative to the reference checkout).  The Python package bnmtf_amd binds these with ctypes
 * and reproduces the class surface; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C, no exceptions; every function returns 0 on success or a negative
 *     BNMTF_E* code; bnmtf_last_error() gives the message (thread-local).
 *   - host pointers are caller-owned, C-contiguous (row-major) and only touched
 *     during the call; every call is synchronous at return.
 *   - factor matrices cross the boundary as double (what the reference's
 *     attributes hold); the device computes the O(I*J*K) contractions with
 *     fp32-exact products on the bf16 matrix cores (every fp32 operand split
 *     into three bf16 terms, six products per fp32 product, fp32 accumulation)
 *     and every reduction that feeds tau / metrics in fp64.
 *   - one host thread per handle; a handle owns its device buffers and stream.
 *   - multi-GPU = one process (and one handle) per GPU, rows of R split over
 *     `world` ranks for the U/F sweep, columns for the V/G sweep, freshly drawn
 *     factor blocks exchanged with an RCCL all-gather.
 */
#ifndef BNMTF_HIP_H
#define BNMTF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden: these are its only dynamic symbols */
#define BNMTF_API __attribute__((visibility("default")))

#define BNMTF_OK 0
#define BNMTF_EINVAL (-1)   /* bad argument / unsupported shape */
#define BNMTF_EHIP (-2)     /* HIP runtime error */
#define BNMTF_ENOMEM (-3)
#define BNMTF_ECOMM (-4)    /* RCCL error */
#define BNMTF_ESTATE (-5)   /* call order (e.g. run before set_state) */

#define BNMTF_MAX_RANK 64   /* K and L <= 64 (one wave lane per latent factor) */

typedef struct bnmtf_model* bnmtf_handle;

/* update rule applied to each conditional: Gibbs draw (the path), or the
 * deterministic mode max(0,mu) = the ICM update of nmf_icm.py:124-134, which
 * shares all tau/mu kernels and serves as an exact end-to-end parity harness. */
#define BNMTF_UPDATE_DRAW 0
#define BNMTF_UPDATE_MODE 1
#define BNMTF_UPDATE_ICM 2        /* nmf_icm / nmtf_icm: TN mode max(0, mu), clamped from below by minimum_TN; tau = gamma_mode */

typedef struct bnmtf_problem {
  int32_t I, J;              /* shape of R */
  int32_t K;                 /* latent factors (rows factor U / F) */
  int32_t L;                 /* 0: BNMF  R ~ U.V^T ;  >0: BNMTF  R ~ F.S.G^T */
  const float* R;            /* I x J, full matrix; entries with M==0 are kept only for predict() */
  const uint8_t* M;          /* I x J, 1 = observed, 0 = missing */
  const double* lambda_rows; /* I x K   lambdaU / lambdaF */
  const double* lambda_cols; /* J x K (lambdaV) or J x L (lambdaG) */
  const double* lambda_S;    /* K x L, BNMTF only (else NULL) */
  double alpha, beta;        /* Gamma prior of tau */
  uint64_t seed;             /* Philox key */
  int32_t device;            /* HIP device ordinal */
  int32_t rank, world;       /* this process' shard; world == 1: single GPU */
  const uint8_t* comm_id;    /* 128-byte id from bnmtf_comm_unique_id (world > 1) */
} bnmtf_problem;

/* ---- library ---------------------------------------------------------- */
BNMTF_API int bnmtf_version(void);
BNMTF_API const char* bnmtf_last_error(void);
BNMTF_API int bnmtf_device_count(int* count);
/* the contiguous block of `n` units (rows for the U/F sweep, columns for V/G) owned by `rank`:
 * first = n*rank/world, count = n*(rank+1)/world - first.  Pure function, no GPU needed. */
BNMTF_API int bnmtf_shard_range(int64_t n, int rank, int world, int64_t* first, int64_t* count);
/* rank 0 makes the id, the host code ships it to the other ranks */
BNMTF_API int bnmtf_comm_unique_id(uint8_t out[128]);

/* ---- life cycle: bnmf_gibbs_optimised.__init__ (bnmf_gibbs_optimised.py:54-78),
 *      bnmtf_gibbs_optimised.__init__ (bnmtf_gibbs_optimised.py:56-84).  Shape /
 *      empty-row assertions stay in the Python class (exact messages); create
 *      re-checks them and fails with BNMTF_EINVAL. ---------------------- */
BNMTF_API int bnmtf_create(const bnmtf_problem* p, bnmtf_handle* out);
BNMTF_API int bnmtf_destroy(bnmtf_handle h);
BNMTF_API int bnmtf_sync(bnmtf_handle h);
/* A TEST HOOK, not an interface to build on (it changes with the handle's layout): the host half of bnmtf_create's work on one
 * direction -- the slot layout of the on-chip sweeps and the choice of their block shape (csrc/slot_layout.hip) -- on its own, so
 * that the tables every sweep kernel gathers through can be tested without a GPU (tests/test_slot_layout_cpu.py).  No handle, no
 * device call; deterministic, with the BNMTF_* layout switches of the environment applied as bnmtf_create applies them.
 * n local units of inner extent m, KP = 32 or 64 (the factor width's padding), world ranks; unit u's missing inner indices,
 * ascending, are miss_idx[miss_ptr[u] .. miss_ptr[u + 1]) (miss_ptr [n + 1]).
 * info [BNMTF_SLOT_INFO_LEN]: mz, pw, nch, mh, pw_chunk, pw1, pair_ok, wide_can, use_wide, use_turns, use_twin, f_nw, vb_path,
 * uw_ok, u_nw, ho_ppb, stats_blocks, npairs, emax, slots, u_emax, then the element counts of the eleven tables in argument
 * order.  A table is copied where its pointer is not NULL: a first call with NULL tables gives the sizes, a second one fills
 * the caller's buffers.  unit_map [2 npairs], pair_E / pair_base [npairs], off [max(slots, 1)][64], off16
 * [max(slots / 2, 1)][64], gen_units (the units left to the generic kernel), row_blk [max(slots, 1)] when ho_ppb > 0, else
 * empty; the unit-per-wave tables u_* when uw_ok, else empty. */
#define BNMTF_SLOT_INFO_LEN 32
BNMTF_API int bnmtf_slot_layout(int n, int m, int KP, int world, const uint32_t* miss_ptr, const uint32_t* miss_idx, int64_t* info,
                                int32_t* unit_map, uint32_t* pair_E, uint32_t* pair_base, uint32_t* off, uint32_t* off16,
                                int32_t* gen_units, uint16_t* row_blk, int32_t* u_unit_map, uint32_t* u_pair_E,
                                uint32_t* u_pair_base, uint32_t* u_off16);
/* A TEST HOOK like bnmtf_slot_layout: the q hand-over tables of one direction (which = 0 rows, 1 cols; csrc/kernel_handover.hip)
 * and what its region holds now, copied to the host so that the routing can be tested entry by entry
 * (tests/test_handover_exact_gpu.py).  Synchronises the handle's stream, launches nothing, changes no state; BNMTF_ESTATE when
 * the handle has no hand-over tables (describe(): handover=0).
 * info [BNMTF_HANDOVER_INFO_LEN]: the direction's blocks, the other direction's blocks, ho_lds_floats, ho_ppb (pairs per block =
 * waves of the block shape), ho_filled, ho_regions_current, then the element counts of the five arrays in argument order.  An
 * array is copied where its pointer is not NULL (a first call with NULL arrays gives the sizes).  t_in / t_out [(slot rows + 1)
 * / 2][64] words of two 16-bit places (rows 2r and 2r + 1 of a lane) in the block's region / staging area, pk [blocks][other
 * blocks][3] (staging start, entries, start in the other direction's regions), region_ofs [blocks + 1], region [region_ofs[blocks]
 * + 256] floats. */
#define BNMTF_HANDOVER_INFO_LEN 11
BNMTF_API int bnmtf_handover_dump(bnmtf_handle h, int which, int64_t* info, uint32_t* t_in, uint32_t* t_out, uint32_t* pk,
                                  uint32_t* region_ofs, float* region);

/* A TEST HOOK like bnmtf_handover_dump: what the relayout and Gram kernels behind a half sweep or a state upload (post_kernel,
 * gram_reduce_kernel, gram_cast_kernel; csrc/kernel_post.hip) read and wrote for one direction (which = 0 rows, 1 cols) of a
 * dense-layout handle, copied to the host so that every output can be restated bit for bit (tests/test_post_exact_gpu.py).
 * Synchronises the compute stream, the tail stream and the exchange stream, waits for a summed Gram that is still on its way as the
 * loop would, launches nothing, changes no state; BNMTF_ESTATE for a handle without these buffers (layout='observed',
 * bnmtf_np_create, a model whose state lives on the one-launch small path).
 * info [BNMTF_POST_INFO_LEN]: rows (of the whole factor), KP, W, ldT, nblk (blocks of 32 rows), whether the handle is a
 * variational one, whether its relayout writes XS, whether it posts the column maxima (umax), this rank's first row and row
 * count, then the element counts of the ten arrays in argument order (0: the handle has none).  An array is copied where its
 * pointer is not NULL and its count is not 0 (a first call with NULL arrays gives the sizes).  X, S2 [rows][KP] as the kernels
 * read them; XT, S2T [KP][ldT]; XT2 [KP / 2][ldT][2]; XS [KP][ldT][2]; C64, C32 [KP][KP]; colsum, colsum2 [KP]. */
#define BNMTF_POST_INFO_LEN 20
BNMTF_API int bnmtf_post_dump(bnmtf_handle h, int which, int64_t* info, float* X, float* S2, float* XT, float* XT2, float* S2T,
                              float* XS, double* C64, float* C32, double* colsum, double* colsum2);

/* size_Omega and the per-row / per-column observed counts (bit-exact integers;
 * size_Omega = M.sum(), bnmf_gibbs_optimised.py:65; counts :83-84).
 * row/col may be NULL. */
BNMTF_API int bnmtf_omega_counts(bnmtf_handle h, uint64_t* total, uint32_t* row, uint32_t* col);

/* Page-locked host memory for the sample arrays run() fills (all_U, all_V, ...; bnmf_gibbs_optimised.py:125-127,
 * 146-148).  *_gibbs_run accepts ANY host pointer for its sample outputs; buffers from here (or registered by the
 * caller with hipHostRegister) are written by asynchronous device-to-host copies that overlap the following
 * iterations, pageable ones go through an internal pinned ring and a host memcpy. */
BNMTF_API int bnmtf_host_alloc(size_t bytes, void** out);
BNMTF_API int bnmtf_host_free(void* p);

/* approx_expectation(burn_in, thinning) (bnmf_gibbs_optimised.py:182-187, bnmtf_gibbs_optimised.py:216-223) on the
 * device: with burn_in >= 0 every *_gibbs_run call sums (fp64) the samples of its iterations burn_in, burn_in +
 * thinning, ... and bnmtf_get_expectation returns their means -- no iterations x I x K array crosses to the host (the
 * model-selection drivers of code/cross_validation/ only need these means).  burn_in < 0 switches it off (default).
 * A: I x K, S: K x L (BNMTF, else ignored), B: J x K (or J x L); any may be NULL. */
BNMTF_API int bnmtf_set_expectation(bnmtf_handle h, int burn_in, int thinning);
BNMTF_API int bnmtf_get_expectation(bnmtf_handle h, double* A, double* S, double* B, double* tau, uint64_t* count);

/* Gibbs iteration counter = RNG counter word 2 (continues across run calls). */
BNMTF_API int bnmtf_set_iteration(bnmtf_handle h, uint64_t it);
/* tau alone (self.tau = ... between half sweeps: the factors on the device stay as they are) */
BNMTF_API int bnmtf_set_tau(bnmtf_handle h, double tau);
BNMTF_API int bnmtf_get_iteration(bnmtf_handle h, uint64_t* it);

/* ---- BNMF Gibbs state: attributes U, V, tau (bnmf_gibbs_optimised.py:102-117) */
BNMTF_API int bnmf_set_state(bnmtf_handle h, const double* U, const double* V, double tau);
BNMTF_API int bnmf_get_state(bnmtf_handle h, double* U, double* V, double* tau);

/* tauU(k)/muU(tauUk,k) (which=0, :167-171) and tauV(k)/muV (which=1, :173-177) for
 * the current state, through the same kernels the sampler uses.  numer_out is
 * (-lambda[:,k] + tau * sum(...)), so that mu = numer / tau_k as the reference
 * divides by the caller-supplied tauUk; tau_out is tauU(k). Length I (or J). */
BNMTF_API int bnmf_cond_params(bnmtf_handle h, int which, int k, double* numer_out, double* tau_out);

/* beta_s() (:164-165) for the current state: beta + 0.5 * masked SSE */
BNMTF_API int bnmtf_beta_s(bnmtf_handle h, double* out);

/* run(iterations) (:121-157): n_iter full sweeps (U columns, V columns, tau draw,
 * metrics on the training mask).  Outputs, each may be NULL:
 *   U_out [n_iter][I][K], V_out [n_iter][J][K]   (all_U / all_V, fp32 samples)
 *   tau_out [n_iter]                             (all_tau)
 *   perf_out [n_iter][3]  MSE, R^2, Rp           (all_performances)
 *   times_out [n_iter]    cumulative seconds     (all_times)           */
BNMTF_API int bnmf_gibbs_run(bnmtf_handle h, int n_iter, int update, float* U_out, float* V_out,
                   double* tau_out, double* perf_out, double* times_out);

/* The same call for n_models independent models at once -- the folds x ranks x restarts a model search fits one after the
 * other (code/cross_validation/line_search_cross_validation.py:54-131, line_search_bnmf.py:53-76,
 * parallel_matrix_cross_validation.py:40-74).  Models on the one-launch path (small models: DESIGN.md section 4,
 * kernel_small.hip -- one block per model, the whole run in one launch) that share a device go down in ONE grid; any other
 * handle in the list is run by bnmf_gibbs_run in turn.  Every model draws exactly the chain its own bnmf_gibbs_run call
 * would draw.  The output arrays are arrays of n_models pointers (or NULL), each as in bnmf_gibbs_run; U_final [I][K], V_final [J][K],
 * tau_final [1] (doubles): the state each model ends with -- what bnmf_get_state would return, fetched for the whole batch with one
 * synchronisation. */
BNMTF_API int bnmf_gibbs_run_many(const bnmtf_handle* hs, int n_models, int n_iter, int update, float* const* U_outs, float* const* V_outs,
                        double* const* tau_outs, double* const* perf_outs, double* const* times_outs,
                        double* const* U_final, double* const* V_final, double* const* tau_final);

/* ---- ranks above 64: a BNMF factorisation as column blocks (round 6) -------
 * The reference takes any K (code/models/bnmf_gibbs_optimised.py:54-78).  The kernels hold a latent factor per wave lane
 * (K <= BNMTF_MAX_RANK), so a wider model runs as ceil(K / 64) column blocks, one handle each, driven by the host class
 * (bnmtf_amd/_blocked.py): the conditionals of block b's columns given the other blocks are those of a rank-K_b model on
 * the residual data R - sum_{b' != b} U_b' V_b'^T, so the blocks' half sweeps in turn -- all blocks' rows (:134-137), then
 * all blocks' columns (:139-142) -- are the reference's sequential column order.  One GPU, BNMF Gibbs / ICM. */
/* this handle holds columns [col0, col0 + K) of the wider model: the Philox column word of its column k is col0 + k (the
 * draws are keyed by the wide model's column index: oracle/rng.py); no one-launch path, no q hand-over */
BNMTF_API int bnmf_set_column_block(bnmtf_handle h, int col0);
/* the contraction operands of h become M . (R - sum_b U_b V_b^T) over the n_others (<= 4) BNMF handles' current factors
 * (n_others = 0: M . R again); predict() / metric entry points keep the full R.  h itself may be a BNMTF handle (a block of
 * the S of a wider tri-factorisation, below) */
BNMTF_API int bnmf_set_residual_data(bnmtf_handle h, const bnmtf_handle* others, int n_others);
/* one half of an iteration of run(): contraction, the K sequential column updates of U (which = 0, :134-137) or V
 * (which = 1, :139-142) with the handle's current tau and iteration counter, then the relayout + Gram the other half reads.
 * tau, metrics, samples and the iteration counter are the caller's. */
BNMTF_API int bnmf_half_sweep(bnmtf_handle h, int which, int update);
/* bnmtf_metric_sums for explicit factors of ANY width Kc: A [I][Kc], B [J][Kc] (compute_MSE / R2 / Rp, :208-223, and
 * beta_s, :164-165, of a column-blocked model) */
BNMTF_API int bnmtf_metric_sums_wide(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* B, int Kc, double sums_out[6]);

/* the variational model (bnmf_vb_optimised.py) as column blocks: one half of an iteration (:134-141) -- update_U(k) +
 * update_exp_U(k) for every k (which = 0) or the same for V -- with the handle's current exptau (bnmtf_set_tau); and
 * exp_square_diff() (:185-187) in its two parts, out[0] = sum_Omega (R - E[U] E[V]^T)^2, out[1] = the second-moment sum
 * over the handle's own columns (additive over blocks) */
BNMTF_API int bnmf_vb_half_sweep(bnmtf_handle h, int which);
BNMTF_API int bnmf_vb_esd_terms(bnmtf_handle h, double out[2]);

/* the tri-factorisation with K or L above 64 (bnmtf_gibbs_optimised.py:56-84 takes any; bnmtf_amd/_blocked.py: TriBlocks).  F's
 * column blocks and G's are BNMF handles against the effective factors (G S_b^T, F S_c), driven through the entry points above;
 * block (b, c) of S is a BNMTF handle (F_b, S_bc, G_c) on the data minus what every other block of S explains:
 * this handle is rows row0.., columns col0.. of a K x L_wide S -- its draws are keyed by their place there (oracle/rng.py: the
 * Philox column word of S_kl is k L + l); its S step runs row by row, no one-launch path, no dense system */
BNMTF_API int bnmtf_set_s_block(bnmtf_handle h, int row0, int col0, int L_wide);
/* rows k0 .. k1-1 of the handle's S, every l in order (:157-160), for its current F, G, tau, iteration counter and data */
BNMTF_API int bnmtf_s_rows(bnmtf_handle h, int k0, int k1, int update);

/* ---- BNMTF Gibbs (bnmtf_gibbs_optimised.py) ---------------------------- */
BNMTF_API int bnmtf_set_state(bnmtf_handle h, const double* F, const double* S, const double* G, double tau);
BNMTF_API int bnmtf_get_state(bnmtf_handle h, double* F, double* S, double* G, double* tau);
/* which = 0: tauF(k)/muF (:195-199), length I; 1: tauS(k,l)/muS (:201-205), length 1;
 * 2: tauG(l)/muG (:207-211), length J (k ignored). */
BNMTF_API int bnmtf_cond_params(bnmtf_handle h, int which, int k, int l, double* numer_out, double* tau_out);
/* run(iterations) (:138-180): F columns, S row-major, G columns, tau. */
BNMTF_API int bnmtf_gibbs_run(bnmtf_handle h, int n_iter, int update, float* F_out, float* S_out, float* G_out,
                    double* tau_out, double* perf_out, double* times_out);

/* bnmtf_gibbs_run for n_models independent tri-factorisations at once: the folds and the (K, L) neighbours a greedy model search
 * fits one after the other (code/cross_validation/greedy_search_cross_validation.py:60-130,
 * experiments/experiments_gdsc/cross_validation/gibbs_nmtf/greedysearch_xval_gibbs.py:17-60).  Models of the one-launch path
 * (K, L <= 32, I, J <= 1024, factors within one CU's LDS: kernel_small.hip) that share a device go down in ONE grid, a block per
 * model -- F sweep, the K L entries of S, G sweep, tau, the metrics of every iteration inside the launch; any other handle is run
 * by bnmtf_gibbs_run in turn.  Every model draws the chain its own bnmtf_gibbs_run call would draw.  Arrays of n_models pointers
 * (or NULL), each as in bnmtf_gibbs_run; F_final [I][K], S_final [K][L], G_final [J][L], tau_final [1] (doubles): the state each
 * model ends with, fetched for the whole batch with one synchronisation. */
BNMTF_API int bnmtf_gibbs_run_many(const bnmtf_handle* hs, int n_models, int n_iter, int update, float* const* F_outs, float* const* S_outs,
                         float* const* G_outs, double* const* tau_outs, double* const* perf_outs, double* const* times_outs,
                         double* const* F_final, double* const* S_final, double* const* G_final, double* const* tau_final);

/* ---- BNMF VB (bnmf_vb_optimised.py) ------------------------------------ */
/* all eight q-parameter matrices + exptau; any pointer may be NULL (left as is) */
BNMTF_API int bnmf_vb_set_state(bnmtf_handle h, const double* muU, const double* tauU, const double* expU, const double* varU,
                      const double* muV, const double* tauV, const double* expV, const double* varV, double exptau);
BNMTF_API int bnmf_vb_get_state(bnmtf_handle h, double* muU, double* tauU, double* expU, double* varU,
                      double* muV, double* tauV, double* expV, double* varV);
/* update_U(k)+update_exp_U(k) (which=0, :189-191,199-204) or update_V/update_exp_V
 * (which=1, :193-195,206-211) for one column; moments=0 skips the update_exp part. */
BNMTF_API int bnmf_vb_update(bnmtf_handle h, int which, int k, int moments);
/* exp_square_diff() (:185-187) */
BNMTF_API int bnmf_vb_exp_square_diff(bnmtf_handle h, double* out);
/* Hook (tests): the two chain-independent masked sums that update_U(k) / update_V(k) use for every (unit, column) of one
 * direction (which = 0: rows i, other factor V; which = 1: columns j, other factor U), formed the way run() forms them on its
 * on-chip path (csrc/kernel_maskgemm.hip: the mask's bits x fixed-point digit planes of the moments on the int8 matrix cores):
 *   asq[u][k] = sum_{r: M = 0} (varO[r][k] + expO[r][k]^2)     (tauU[i][k] = exptau * (sum_j S2V[j][k] - asq[i][k]),  :189-199)
 *   vsq[u][k] = sum_{r: M = 0} expO[r][k]^2                     (the unit's own term of the numerator of muU)
 * for the rank's local units, [n][K] doubles each. */
BNMTF_API int bnmf_vb_masked_sums(bnmtf_handle h, int which, double* asq, double* vsq);
/* Hook (tests), read-only: the column maxima of [S2 | E^2] of the factor U (which = 0) or V (which = 1) that fix the fixed-point
 * grid of the masked product's digit planes, as fp32 bit patterns, 2 KP words each (KP = 32 for K <= 32, else 64; columns
 * [0, K) of S2 = var + exp^2, then [KP, KP + K) of exp^2, padding columns zero): posted = what the factor's last relayout left
 * (its Gram blocks see every row), *was_posted = 1 when the next on-chip half sweep would take them as they are; own = a pass of
 * the fall-back kernel over the factor into a scratch buffer.  The model's state is left as it is.  Any pointer may be NULL. */
BNMTF_API int bnmf_vb_column_maxima(bnmtf_handle h, int which, uint32_t* posted, uint32_t* own, int* was_posted);
/* run(iterations) (:121-153).  exptau_out[n_iter] (all_exp_tau), perf_out[n_iter][3], times_out[n_iter],
 * elbo_terms_out[n_iter][10] = the O(I*J) / O((I+J)K) pieces of elbo() (:163-177) that live on the device:
 *   {exp_square_diff, beta_s,
 *    sum tauU/2 (varU+(expU-muU)^2), sum log(0.5 erfc(-muU sqrt(tauU/2))), sum log tauU, sum lambdaU expU,
 *    the same four for V};  the host finishes the scalar algebra (digamma, gammaln). */
BNMTF_API int bnmf_vb_run(bnmtf_handle h, int n_iter, double* exptau_out, double* perf_out,
                double* elbo_terms_out, double* times_out);
/* run(iterations) of n_models variational models on one device, walked in lock-step: every kernel of an iteration is ONE launch
 * for all of them (csrc/many.h, api_many.inc) -- the reference's model searches (experiments_gdsc/cross_validation/vb_nmf/
 * linesearch_xval_vb.py:17-52) are dozens of independent models of 622 x 138.  Every model ends with the bits of its own
 * bnmf_vb_run.  Outputs model-major ([n_models][n_iter]..., as bnmf_vb_run's; times = the batch's clock); any may be null.  Models
 * that cannot share launches (several GPUs, the 16-wave shapes of large problems, kernel timers on) run one after the other.
 * launch_info (optional, 2 ints): the models that shared launches, the argument-list uploads. */
BNMTF_API int bnmf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* exptau_out, double* perf_out,
                     double* elbo_terms_out, double* times_out, int* launch_info);

/* ---- BNMTF VB (bnmtf_vb_optimised.py); K, L <= 32, one GPU ---------------- */
/* the twelve q-parameter matrices (F: I x K, S: K x L, G: J x L) + exptau; any pointer may be NULL (left as is) */
BNMTF_API int bnmtf_vb_set_state(bnmtf_handle h, const double* muF, const double* tauF, const double* expF, const double* varF,
                       const double* muS, const double* tauS, const double* expS, const double* varS,
                       const double* muG, const double* tauG, const double* expG, const double* varG, double exptau);
BNMTF_API int bnmtf_vb_get_state(bnmtf_handle h, double* muF, double* tauF, double* expF, double* varF,
                       double* muS, double* tauS, double* expS, double* varS,
                       double* muG, double* tauG, double* expG, double* varG);
/* update_F(k) (which = 0, :241-250), update_S(k,l) (which = 1, :252-262), update_G(l) (which = 2, :264-273) for the
 * current state; moments != 0 also runs the matching update_exp_* (:276-285). */
BNMTF_API int bnmtf_vb_update(bnmtf_handle h, int which, int k, int l, int moments);
/* exp_square_diff() (:235-239); sums_out (may be NULL): n, sum R, sum R^2, sum P, sum P^2, sum R P over the training
 * mask with P = E[F] E[S] E[G]^T */
BNMTF_API int bnmtf_vb_exp_square_diff(bnmtf_handle h, double* esd_out, double sums_out[6]);
/* run(iterations) (:160-205).  orders [n_iter][K L + K + L]: per iteration the update order of the S entries (k L + l),
 * the F columns and the G columns (the reference shuffles them with random.shuffle, :171-186; the host class draws the
 * same shuffles).  exptau_out [n_iter]; perf_out [n_iter][3]; times_out [n_iter]; elbo_terms_out [n_iter][10] =
 * {exp_square_diff, beta_s, then for F and for G: sum tau/2 (var+(exp-mu)^2), sum log(0.5 erfc(-mu sqrt(tau/2))),
 * sum log tau, sum lambda exp} -- the K L terms of S and the scalar algebra are the host's. */
BNMTF_API int bnmtf_vb_run(bnmtf_handle h, int n_iter, const int32_t* orders, double* exptau_out, double* perf_out,
                 double* elbo_terms_out, double* times_out);
/* run(iterations) of n_models tri-factorisations on one device, walked in lock-step: every launch site of an iteration is ONE launch
 * for all of them (csrc/many.h, api_many.inc) -- the reference's model searches (experiments_gdsc/cross_validation/vb_nmtf/
 * greedysearch_xval_vb.py: folds x a greedy walk over K, L) are dozens to hundreds of independent models of 622 x 138.  Models may
 * differ in shape and in K, L; every model ends with the bits of its own bnmtf_vb_run.  orders[b]: model b's [n_iter][K L + K + L]
 * update orders (bnmtf_vb_run's).  Outputs model-major ([n_models][n_iter]..., as bnmtf_vb_run's; times = the batch's clock); any
 * may be null.  Models that cannot share launches (several GPUs, kernel timers on, the 16-wave sweeps of large problems, an A/B
 * switch) run one after the other.  launch_info (optional, 2 ints): the models that shared launches, the argument-list uploads. */
BNMTF_API int bnmtf_vb_run_many(bnmtf_handle* hs, int n_models, int n_iter, const int32_t* const* orders, double* exptau_out,
                      double* perf_out, double* elbo_terms_out, double* times_out, int* launch_info);

/* ---- metrics: predict()/predict_while_running()/quality('MSE')/log_likelihood
 *      (:191-223,247-251).  Six fp64 sums over mask Mp (I x J bytes; NULL = the
 *      training mask): n, sum R, sum R^2, sum P, sum P^2, sum R*P with
 *      P = A.B^T (S == NULL, A: I x K, B: J x K) or A.S.B^T (S: K x L, B: J x L).
 *      A == NULL uses the handle's current state. */
BNMTF_API int bnmtf_metric_sums(bnmtf_handle h, const uint8_t* Mp, const double* A, const double* S,
                      const double* B, double sums_out[6]);

/* ---- held-out performance per iteration -----------------------------------
 * The reference's convergence experiments follow the test error over the iterations by predict(M_test) on stored samples
 * (experiments/experiments_toy/convergence/); here the run loops evaluate the state each iteration ends with -- the sample of a
 * Gibbs run, the point estimate of ICM, E[.] of the variational models -- on a sparse list of held-out entries, on the device
 * (csrc/kernel_heldout.hip: fp64 products of the fp32 factors, fixed summation order, no pass over R).
 * M_test [I][J]: nonzero = held out (it may overlap the training mask, as predict() allows); NULL clears.  Any handle of
 * bnmtf_create or bnmtf_np_create; one created with world > 1 or as a block of a wider factorisation is refused with BNMTF_EINVAL,
 * as is a mask without entries.  While a mask is set, bnmf_gibbs_run, bnmtf_gibbs_run, bnmf_vb_run, bnmtf_vb_run, bnmf_np_run and
 * bnmtf_np_run record the six sums of every iteration, and so do bnmf_vb_run_many, bnmtf_vb_run_many and bnmtf_np_run_many for
 * each of their models that has one (the held-out kernels join the models' shared launches; models with and without a mask mix).
 * A model of the one-launch kind runs the multi-launch path, and bnmf_gibbs_run_many / bnmtf_gibbs_run_many refuse the handle:
 * their kernel has no per-iteration hook. */
BNMTF_API int bnmtf_set_heldout(bnmtf_handle h, const double* M_test);
/* the records of the last run call: sums_out [n_iter][6] = n, sum R, sum R^2, sum P, sum P^2, sum R P per iteration (R as the
 * device holds it, fp32).  BNMTF_ESTATE if that call ran fewer than n_iter iterations or no mask was set. */
BNMTF_API int bnmtf_get_heldout(bnmtf_handle h, int n_iter, double* sums_out);
/* run(M_test=Entries) of bnmf_gibbs_optimised(layout='observed'), nmf_icm(layout='observed') and bnmf_vb_observed: the held-out
 * entries of a two-factor handle of bnmtf_obs_create as lists (rows, cols, values) of n entries in any order -- the handle keeps
 * no copy of R, so the values arrive with the entries; they may overlap the training entries.  n == 0 or a NULL list clears.
 * While a list is set, bnmf_obs_run and bnmf_vbo_run record the six sums of every iteration for bnmtf_get_heldout
 * (csrc/kernel_obs_heldout.hip: fp64 products of the handle's fp32 factor rows -- the variational model's expectations --, fixed
 * summation order); without one they launch and allocate nothing more.  BNMTF_EINVAL: an entry outside the matrix, an entry that
 * occurs twice (named by its position in the sorted list), and any other handle -- this is a two-factor call: bnmtf_otri_create's
 * and bnmtf_onp_create's handles keep no held-out record yet, bnmtf_create's and bnmtf_np_create's take bnmtf_set_heldout, which
 * keeps refusing the handles of this layout. */
BNMTF_API int bnmtf_set_heldout_entries(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values);

/* ---- distributions (stand-alone hooks; code/models/distributions/) ----- */
/* TN_vector_draw (truncated_normal_vector.py:37-50): out[e] ~ TN(mu[e],tau[e]) on
 * [0,inf); RNG counter (elem0+e, col, it, STREAM_HOOK). */
BNMTF_API int bnmtf_tn_sample(const double* mu, const double* tau, size_t n, uint64_t seed, uint64_t it,
                    uint32_t col, uint32_t elem0, int device, double* out);
/* TN_vector_expectation / TN_vector_variance (:53-73) */
BNMTF_API int bnmtf_tn_moments(const double* mu, const double* tau, size_t n, int device,
                     double* exp_out, double* var_out);
/* gamma_draw (gamma.py:11-14), shape alpha, rate beta */
BNMTF_API int bnmtf_gamma_sample(double alpha, double beta, uint64_t seed, uint64_t it, int device, double* out);

/* ---- masked K-means for initialise(init_FG='kmeans') (code/models/kmeans/kmeans.py): the two O(points x coordinates x K)
 *      passes of an iteration; X [n_points][n_coords] fp64 (as the reference computes), M 0/1 bytes; the handle is a plain pointer of its own kind. */
BNMTF_API int bnmtf_kmeans_create(const double* X, const uint8_t* M, int n_points, int n_coords, int K, int device, void** out);
BNMTF_API int bnmtf_kmeans_destroy(void* h);
/* assignment() (kmeans.py:87-119): closest centroid by MSE over the shared observed coordinates (none: infinitely far;
 * ties: lowest index); dist_out = that MSE (+inf without overlap) */
BNMTF_API int bnmtf_kmeans_assign(void* h, const double* centroids, const uint8_t* mask_centroids, int32_t* assign_out, double* dist_out);
/* the sums update() needs (kmeans.py:126-182): cnt_out / tot_out [K][n_coords] = number / sum of the values of the
 * cluster's members that observe the coordinate (assign < 0: the point belongs to no cluster) */
BNMTF_API int bnmtf_kmeans_sums(void* h, const int32_t* assign, double* cnt_out, double* tot_out);
/* X[index][:] = values: `self.centroids[c] = self.X[index]` (kmeans.py:141) makes the refilled centroid a view of the data
 * point, so the means written into the centroid afterwards (:158-163) change the point; the host class mirrors that */
BNMTF_API int bnmtf_kmeans_set_row(void* h, int index, const double* values);
/* The same handle from the n observed entries (point, coordinate, value), given in any order: device memory and the work of a
 * pass follow n (28 bytes an entry; nothing of size n_points x n_coords), for the data of the observed-entry layout.  assign, sums,
 * set_row (still n_coords values: the point's observed entries take theirs) and destroy serve it unchanged, and every output
 * equals, bit for bit, that of a bnmtf_kmeans_create handle of the same (X, M).  A point or a coordinate may be empty.  Refused
 * with BNMTF_EINVAL before any device call: a null argument, a shape below 1 x 1, K outside 1 .. 1024, n >= 2^31, an entry outside
 * the matrix, an entry given twice. */
BNMTF_API int bnmtf_kmeans_create_list(int n_points, int n_coords, uint64_t n, const int32_t* points, const int32_t* coords, const double* values,
                             int K, int device, void** out);
/* The host half of bnmtf_kmeans_create_list on its own (no GPU needed), its checks included: point_ptr [n_points + 1], point_coord /
 * point_val [n] -- a point's entries ordered by (coordinate & 63, coordinate) --, coord_ptr [n_coords + 1], coord_point / coord_val
 * [n] -- a coordinate's entries ordered by (point & 3, point) -- and point_to_coord [n], the place in the coordinate list of the
 * entry at each place of the point list.  Any output may be null. */
BNMTF_API int bnmtf_kmeans_build_lists(int n_points, int n_coords, uint64_t n, const int32_t* points, const int32_t* coords, const double* values,
                             uint32_t* point_ptr, uint32_t* point_coord, double* point_val, uint32_t* coord_ptr, uint32_t* coord_point,
                             double* coord_val, uint32_t* point_to_coord);

/* ---- measurement aids (bench.py) --------------------------------------- */
#define BNMTF_KERNEL_GEMM_ROWS 0   /* P  = R~ . V      (U/F step numerators)        */
#define BNMTF_KERNEL_GEMM_COLS 1   /* Pv = R~^T . U    ("the U^T.R step")          */
#define BNMTF_KERNEL_SWEEP_ROWS 2
#define BNMTF_KERNEL_SWEEP_COLS 3
#define BNMTF_KERNEL_SWEEP_S 4      /* BNMTF: the K*L sequential S entries */
#define BNMTF_KERNEL_COUNT 8
/* enable = 1: run() brackets each launch of the listed kernels with hipEvents on the handle's
 * stream; enable = 2 + k (+ 32 (n - 1)): only kernel k (BNMTF_KERNEL_*), in every n-th iteration (an event record
 * costs the queue a few microseconds: a timed run samples); 0: off.  Totals are read back with bnmtf_kernel_stats. */
BNMTF_API int bnmtf_set_profiling(bnmtf_handle h, int enable);
/* ICM: the lower clamp run(iterations, minimum_TN) applies to every updated entry (nmf_icm.py:129,135;
 * nmtf_icm.py:147,153,159).  Used by *_gibbs_run with update = BNMTF_UPDATE_ICM.  Default 0. */
BNMTF_API int bnmtf_set_minimum_tn(bnmtf_handle h, double minimum_TN);
/* sweep kernel selection: 1 (default) = register/LDS-resident fast path when the shape
 * fits, 0 = always the generic kernel (any mask, q in global memory).  Same results. */
BNMTF_API int bnmtf_set_sweep_path(bnmtf_handle h, int fast);
/* the one-launch path for small models, two- and three-factor (K, L <= 32, I, J <= 1024, factors within one CU's LDS; run() = one
 * launch, one block per model).  mode 1 (default): taken when it is the faster way to run the call -- always for the models of
 * 256- and 512-thread blocks, for the ones that fill a CU (1024-thread blocks) from three models per bnmf_gibbs_run_many call on
 * (two per bnmtf_gibbs_run_many call; a tri-factorisation with a rank above 10 -- the sequential form of its S step -- only in a batch of at
 * least (K L + 50) / 80 models); 0: never (the multi-launch path); 2: always.  Same chain either way up to fp32 summation order.
 * bnmtf_is_small: would a bnmf_gibbs_run / bnmtf_gibbs_run of this handle alone take it? */
BNMTF_API int bnmtf_set_small_path(bnmtf_handle h, int mode);
/* the handle's communicator as it reports itself: kind 0 none (one GPU), 1 RCCL (ranks = ncclCommCount), 2 the in-process test
 * transport; bench.py prints both next to its own world size */
BNMTF_API int bnmtf_comm_info(bnmtf_handle h, int* kind, int* ranks);
/* 1 when the library was built with `make EXPERIMENTS=1`: the measured-and-not-adopted kernels (two unit groups taking turns,
 * BNMTF_TURNS=1; two 8-wave blocks per CU, BNMTF_TWIN=1; the f32-MFMA contraction, BNMTF_GEMM=f32 -- DESIGN.md section 7) are
 * compiled in and their switches honoured.  The shipped build has none of them. */
BNMTF_API int bnmtf_has_experiments(void);
BNMTF_API int bnmtf_is_small(bnmtf_handle h, int* out);
BNMTF_API int bnmtf_kernel_stats(bnmtf_handle h, int kernel, double* total_ms, uint64_t* launches);
/* geometry of the last create: padded shapes, split factor, slot counts (for DESIGN/bench) */
BNMTF_API int bnmtf_describe(bnmtf_handle h, char* buf, size_t buflen);

/* ---- non-probabilistic NMF / NMTF (nmf_np.py, nmtf_np.py: multiplicative updates) ---------------------
 * A handle of its own kind: R ([I][J] fp32) and the 0/1 mask M ([I][J]) go to the device, nothing of the samplers' layouts is
 * built, so K and L are not tied to wave lanes (1 <= K, L <= BNMTF_NP_MAX_RANK; rows and columns of at most 16 384 entries).
 * L = 0: NMF (R ~ U V^T), L > 0: NMTF (R ~ F S G^T).  One GPU.  Such a handle takes the calls below, bnmtf_sync,
 * bnmtf_describe and bnmtf_destroy; the sampler and variational calls refuse it.  Factors cross as double, live as fp32. */
#define BNMTF_NP_MAX_RANK 256
BNMTF_API int bnmtf_np_create(const float* R, const uint8_t* M, int I, int J, int K, int L, int device, bnmtf_handle* out);
/* U [I][K], V [J][K] */
BNMTF_API int bnmf_np_set_state(bnmtf_handle h, const double* U, const double* V);
BNMTF_API int bnmf_np_get_state(bnmtf_handle h, double* U, double* V);
/* update_U(k) (which = 0) or update_V(k) (which = 1): nmf_np.py:117-121 */
BNMTF_API int bnmf_np_update(bnmtf_handle h, int which, int k);
/* run(n_iter), nmf_np.py:84-107: per iteration the K columns of U, then the K columns of V.  perf_out [n][3] (MSE, R^2, Rp on the
 * training mask), idiv_out [n] (compute_I_div), times_out [n] (seconds since the call began, device clock); any may be null */
BNMTF_API int bnmf_np_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out);
/* F [I][K], S [K][L], G [J][L] */
BNMTF_API int bnmtf_np_set_state(bnmtf_handle h, const double* F, const double* S, const double* G);
BNMTF_API int bnmtf_np_get_state(bnmtf_handle h, double* F, double* S, double* G);
/* update_F(k) (which = 0), update_S(k, l) (which = 1), update_G(l) (which = 2): nmtf_np.py:152-174 */
BNMTF_API int bnmtf_np_update(bnmtf_handle h, int which, int k, int l);
/* run(n_iter), nmtf_np.py:116-144: per iteration the K L entries of S row by row, the K columns of F, the L columns of G */
BNMTF_API int bnmtf_np_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out);
/* run(n_iter) of n_models handles of bnmtf_np_create on one device (NMF and NMTF, any shapes and ranks), walked in lock-step: every
 * launch site of an iteration -- before the S step, S pass t, after it -- is ONE launch for all of them (csrc/many.h,
 * api_many.inc).  Every model ends with the bits of its own bnmf_np_run / bnmtf_np_run.  Outputs model-major: perf_out
 * [n_models][n_iter][3], idiv_out [n_models][n_iter], times_out [n_models][n_iter] (the batch's clock); any may be null.
 * launch_info (optional, 2 ints): the models that shared launches, the argument-list uploads.  Refuses a null handle, one given
 * twice, handles of several devices and a handle without state. */
BNMTF_API int bnmtf_np_run_many(bnmtf_handle* hs, int n_models, int n_iter, double* perf_out, double* idiv_out, double* times_out,
                      int* launch_info);
/* the current point's sums over the entries of Mp ([I][J] 0/1; null: the training mask), fp64: out[8] = n, sum R, sum R^2,
 * sum P, sum P^2, sum R P, the I-divergence sum R log(R / P) - R + P (nmf_np.py:146-148), sum (R - P)^2 */
BNMTF_API int bnmtf_np_metrics(bnmtf_handle h, const uint8_t* Mp, double* out);

/* ---- observed-entry layout of the two-factor Gibbs / ICM models (layout='observed') ---------
 * A handle of its own kind for matrices that are mostly missing: the device holds the OBSERVED entries as a row list and a column
 * list, both factors in fp32 and the residual R_ij - U_i.V_j on the observed entries; cost and memory are proportional to the
 * number of observed entries and nothing of size I x J exists.  The entries come as three lists of length n, in any order, no
 * entry twice, every row and every column of R at least once: rows[e] in [0, I), cols[e] in [0, J), values[e] = R[rows[e]][cols[e]].
 * 1 <= K <= BNMTF_OBS_MAX_RANK, one GPU.  Same conditionals, same Philox keying and candidate sequence as bnmf_gibbs_run.  Such a
 * handle takes the calls below, bnmtf_set_minimum_tn, bnmtf_set_iteration / bnmtf_get_iteration, bnmtf_sync, bnmtf_describe and
 * bnmtf_destroy; every other call refuses it.  BNMTF_OBS_LONG=1 in the environment at creation sends every unit down the kernel's
 * long form (a test switch: the results are the same bits). */
#define BNMTF_OBS_MAX_RANK 256
BNMTF_API int bnmtf_obs_create(int I, int J, int K, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                     const double* lambda_rows, const double* lambda_cols, double alpha, double beta, uint64_t seed, int device,
                     bnmtf_handle* out);
/* A TEST HOOK, not an interface to build on (it may change with the handle's layout): the host half of bnmtf_obs_create on its
 * own, so that the builder the device data come from can be tested without a GPU (tests/test_obs_cpu.py).  Pure function: the
 * same checks -- an entry outside the matrix, an entry twice, a row or column without entries are refused -- and the two lists
 * the device would hold: row_ptr [I + 1], row_col [n] (columns ascending within a row), row_val [n]; col_ptr [J + 1], col_row [n]
 * (rows ascending within a column), col_val [n].  Any output may be null. */
BNMTF_API int bnmtf_obs_build_lists(int I, int J, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                          uint32_t* row_ptr, uint32_t* row_col, float* row_val, uint32_t* col_ptr, uint32_t* col_row, float* col_val);
/* U [I][K], V [J][K], tau */
BNMTF_API int bnmf_obs_set_state(bnmtf_handle h, const double* U, const double* V, double tau);
BNMTF_API int bnmf_obs_get_state(bnmtf_handle h, double* U, double* V, double* tau);
/* run(n_iter) with the arguments of bnmf_gibbs_run: update = BNMTF_UPDATE_*; U_out [n][I][K], V_out [n][J][K] (fp32 samples),
 * tau_out [n], perf_out [n][3] (MSE, R^2, Rp on the observed entries), times_out [n]; any output may be null */
BNMTF_API int bnmf_obs_run(bnmtf_handle h, int n_iter, int update, float* U_out, float* V_out, double* tau_out, double* perf_out,
                 double* times_out);
/* as bnmf_cond_params: numerator and precision of column k's conditional for every row (which = 0) or column (which = 1) */
BNMTF_API int bnmf_obs_cond_params(bnmtf_handle h, int which, int k, double* numer_out, double* tau_out);
/* the six sums of metrics_from_sums -- n, sum R, sum R^2, sum P, sum P^2, sum R P with P = A_i . B_j -- over a list of entries
 * (any order; they need not be observed ones), A [I][K] and B [J][K] in fp64; fp64 throughout, fixed summation order */
BNMTF_API int bnmf_obs_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                         const double* A, const double* B, double sums_out[6]);

/* ---- the variational two-factor model on the observed-entry layout (class bnmf_vb_observed) -----
 * The calls of bnmf_vb_* above with the same arguments and the same meaning, on a handle of bnmtf_obs_create: the iteration is two
 * half sweeps over the entry lists and an end-of-iteration kernel (csrc/kernel_obs_vb.hip), cost and memory proportional to the
 * number of observed entries.  The q parameters' buffers are allocated by the first bnmf_vbo_set_state: a handle that only
 * samples holds none.  A null handle or one of bnmtf_create is refused with BNMTF_EINVAL, a call ahead of bnmf_vbo_set_state
 * with BNMTF_ESTATE.  Fixed summation order: the same call gives the same bits, run(a) then run(b) those of run(a + b). */
/* all eight q-parameter matrices ([I][K] four times, [J][K] four times) and exptau; none may be null */
BNMTF_API int bnmf_vbo_set_state(bnmtf_handle h, const double* muU, const double* tauU, const double* expU, const double* varU,
                       const double* muV, const double* tauV, const double* expV, const double* varV, double exptau);
/* any pointer may be null */
BNMTF_API int bnmf_vbo_get_state(bnmtf_handle h, double* muU, double* tauU, double* expU, double* varU,
                       double* muV, double* tauV, double* expV, double* varV);
/* run(n_iter) with the outputs of bnmf_vb_run: exptau_out [n], perf_out [n][3] (MSE, R^2, Rp on the observed entries),
 * elbo_terms_out [n][10] (exp_square_diff, beta_s, the four sums of U, the four of V), times_out [n]; any may be null */
BNMTF_API int bnmf_vbo_run(bnmtf_handle h, int n_iter, double* exptau_out, double* perf_out, double* elbo_terms_out, double* times_out);
/* update_U(k) (which = 0) or update_V(k) (which = 1): mu and tau of column k; moments != 0: also its expectation and variance */
BNMTF_API int bnmf_vbo_update(bnmtf_handle h, int which, int k, int moments);
/* exp_square_diff() of the state the device holds, fp64 over the observed entries */
BNMTF_API int bnmf_vbo_exp_square_diff(bnmtf_handle h, double* out);

/* ---- the tri-factorisation on the observed-entry layout (bnmtf_gibbs_optimised / nmtf_icm, layout='observed') ----
 * A handle of its own kind again: the entry lists of bnmtf_obs_create (same arguments, same refusals), F [I][K], S [K][L] and
 * G [J][L] in fp32, the two effective factors G S^T and F S, and the buffers of the dense K.L x K.L system of the S step; cost and
 * memory are proportional to the number of observed entries and nothing of size I x J exists.  1 <= K, L <= BNMTF_OTRI_MAX_RANK (one
 * 32 x 32 tile per column Gram), one GPU.  The iteration is bnmtf_gibbs_run's -- F columns, S row-major, G columns, tau -- with the
 * same Philox keying, so the same seed gives the dense layout's chain up to fp32 rounding.  Such a handle takes the calls below,
 * bnmtf_set_minimum_tn, bnmtf_set_iteration / bnmtf_get_iteration, bnmtf_sync, bnmtf_describe and bnmtf_destroy; every other call
 * refuses it, and these refuse every other handle.  BNMTF_OBS_LONG=1 at creation: as for bnmtf_obs_create. */
#define BNMTF_OTRI_MAX_RANK 32
BNMTF_API int bnmtf_otri_create(int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                      const double* lambda_F, const double* lambda_S, const double* lambda_G, double alpha, double beta,
                      uint64_t seed, int device, bnmtf_handle* out);
/* F [I][K], S [K][L], G [J][L], tau; get: any pointer may be null */
BNMTF_API int bnmtf_otri_set_state(bnmtf_handle h, const double* F, const double* S, const double* G, double tau);
BNMTF_API int bnmtf_otri_get_state(bnmtf_handle h, double* F, double* S, double* G, double* tau);
/* run(n_iter) with the arguments of bnmtf_gibbs_run: update = BNMTF_UPDATE_*; F_out [n][I][K], S_out [n][K][L], G_out [n][J][L]
 * (fp32 samples), tau_out [n], perf_out [n][3] (MSE, R^2, Rp on the observed entries), times_out [n]; any output may be null */
BNMTF_API int bnmtf_otri_run(bnmtf_handle h, int n_iter, int update, float* F_out, float* S_out, float* G_out, double* tau_out,
                   double* perf_out, double* times_out);
/* as bnmtf_cond_params: which = 0: column k of F, numerator and precision for every row; 1: entry (k, l) of S, one value each;
 * 2: column l of G, for every column of R.  The state is left as it is. */
BNMTF_API int bnmtf_otri_cond_params(bnmtf_handle h, int which, int k, int l, double* numer_out, double* tau_out);
/* the six sums of metrics_from_sums over a list of entries (any order; they need not be observed ones) with P = (F S)_i . G_j:
 * F [I][K], S [K][L], G [J][L] in fp64, F S formed in fp64 too; fp64 throughout, fixed summation order */
BNMTF_API int bnmtf_otri_metric_sums(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                           const double* F, const double* S, const double* G, double sums_out[6]);

/* ---- the variational tri-factorisation on the observed-entry layout (class bnmtf_vb_observed) -----
 * The calls of bnmtf_vb_* above with the same arguments and the same meaning, on a handle of bnmtf_otri_create (K, L <= 32, one GPU):
 * per iteration the S entries on the second-moment K.L x K.L system, then the F and the G half sweep over the entry lists with the
 * covariance term, in the orders handed over (csrc/kernel_obs_trivb.hip, kernel_obs_vb.hip, kernel_obs_tri.hip); cost and memory
 * proportional to the number of observed entries.  The variational buffers are allocated by the first bnmtf_otvb_set_state.  A
 * handle holds a sampler's state or a variational one: bnmtf_otvb_set_state ends the state of bnmtf_otri_set_state and the reverse,
 * and bnmtf_otri_run / _get_state / _cond_params refuse a variational state as these refuse a sampler's (BNMTF_ESTATE);
 * bnmtf_otri_metric_sums takes its factors as arguments and serves both.  Fixed summation order, no atomics: the same call gives
 * the same bits, run(a) then run(b) those of run(a + b).  (The names: bnmtf_otri_* is the closed set of the sampler's calls.) */
/* all twelve q-parameter matrices ([I][K] x 4, [K][L] x 4, [J][L] x 4) and exptau; none may be null */
BNMTF_API int bnmtf_otvb_set_state(bnmtf_handle h, const double* muF, const double* tauF, const double* expF, const double* varF,
                         const double* muS, const double* tauS, const double* expS, const double* varS,
                         const double* muG, const double* tauG, const double* expG, const double* varG, double exptau);
/* any pointer may be null */
BNMTF_API int bnmtf_otvb_get_state(bnmtf_handle h, double* muF, double* tauF, double* expF, double* varF,
                         double* muS, double* tauS, double* expS, double* varS,
                         double* muG, double* tauG, double* expG, double* varG);
/* update_F(k) (which = 0), update_S(k, l) (1), update_G(l) (2): mu and tau of the target; moments != 0: also its expectation and variance */
BNMTF_API int bnmtf_otvb_update(bnmtf_handle h, int which, int k, int l, int moments);
/* exp_square_diff() of the state the device holds: fp64, all four terms per observed entry */
BNMTF_API int bnmtf_otvb_exp_square_diff(bnmtf_handle h, double* out);
/* run(n_iter) with the arguments of bnmtf_vb_run: orders [n][K L + K + L] (S entries k L + l, F columns, G columns; required, every
 * index in range), exptau_out [n], perf_out [n][3], elbo_terms_out [n][10] (exp_square_diff, beta_s, the four sums of F, the four of
 * G), times_out [n]; any output may be null */
BNMTF_API int bnmtf_otvb_run(bnmtf_handle h, int n_iter, const int32_t* orders, double* exptau_out, double* perf_out,
                   double* elbo_terms_out, double* times_out);

/* ---- the non-probabilistic NMF / NMTF on the observed-entry layout (nmf_np.NMF / nmtf_np.NMTF with layout='observed';
 * DESIGN.md section 2.7) ------------------------------------------------------------------------------------------------------
 * The multiplicative updates of the bnmf_np_* / bnmtf_np_* calls above with P = U V^T (or F S G^T) kept on the observed entries
 * only (csrc/kernel_obs_np.hip): cost and memory proportional to the number of observed entries, nothing of size I x J, no limit on
 * the length of a row or column.  1 <= K <= BNMTF_ONP_MAX_RANK; L = 0: NMF, else NMTF with 1 <= L <= BNMTF_ONP_MAX_RANK; one GPU.
 * The handle is one of its own kind: the bnmf_obs_*, bnmf_vbo_*, bnmtf_otri_* and bnmtf_otvb_* calls refuse it and these refuse
 * theirs.  Fixed summation order, no atomics: the same call gives the same bits, run(a) then run(b) those of run(a + b). */
#define BNMTF_ONP_MAX_RANK 256
/* the entries as bnmtf_obs_create takes them, with its checks and messages (before any device call); no priors, no seed */
BNMTF_API int bnmtf_onp_create(int I, int J, int K, int L, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values,
                     int device, bnmtf_handle* out);
/* A [I][K], S [K][L], B [J][K] (NMF) or [J][L] (NMTF), fp64 on the host, fp32 on the device; S: null for NMF, required for NMTF */
BNMTF_API int bnmtf_onp_set_state(bnmtf_handle h, const double* A, const double* S, const double* B);
/* any pointer may be null */
BNMTF_API int bnmtf_onp_get_state(bnmtf_handle h, double* A, double* S, double* B);
/* n_iter iterations (NMF: U then V; NMTF: S, F, G); perf_out [n][3] MSE / R^2 / Rp, idiv_out [n], times_out [n]; any may be null */
BNMTF_API int bnmtf_onp_run(bnmtf_handle h, int n_iter, double* perf_out, double* idiv_out, double* times_out);
/* one column: which = 0 column k of U / F, 1 entry (k, l) of S (NMTF), 2 column l of V / G.  The columns of a factor called in
 * order continue one half sweep: together they give its bits */
BNMTF_API int bnmtf_onp_update(bnmtf_handle h, int which, int k, int l);
/* the eight sums n, sum R, sum R^2, sum P, sum P^2, sum R P, I-divergence, SSE of the handle's factors over the entries given, in
 * any order (n = 0: the training entries); P in fp64 from the fp32 factors, NMTF: (F_i S) . G_j with F_i S in fp64 */
BNMTF_API int bnmtf_onp_metrics(bnmtf_handle h, uint64_t n, const int32_t* rows, const int32_t* cols, const float* values, double* out8);

/* ---- posterior predictive statistics of stored samples over an entry list (bnmtf_amd.posterior_predictive; DESIGN.md section
 * 2.8) -------------------------------------------------------------------------------------------------------------------------
 * No handle: the call makes its own stream and buffers on `device` and frees all of them on every path.  Per entry e = (rows[e],
 * cols[e]) -- any order, an entry may occur more than once, 1 <= n < 2^31 -- and per sample s = 0 .. T - 1 (array index
 * first + s step, step >= 1, T >= 1) the prediction p_s: L = 0, S null: A [.][I][K] . B [.][J][K]; L >= 1: (A [.][I][K] S [.][K][L]) .
 * B [.][J][L]; 1 <= K <= 256, 0 <= L <= 256.  Host arrays, fp32, contiguous, row stride exactly K (or L).  Outputs [n] in the given
 * order: p_first = p_0, sum_d = sum_s (p_s - p_0), sum_d2 = sum_s (p_s - p_0)^2; the caller finishes mean = p_first + sum_d / T and
 * variance = max(0, sum_d2 / T - (sum_d / T)^2).  Every fp32 value is widened to fp64, p_s is the fma chain over the inner index
 * ascending ((A S)_l first, over k ascending), the samples are added in ascending s: an entry's three numbers depend on that entry
 * and the samples alone -- not on chunk_samples (samples uploaded per kernel launch; 0: as many as fit the library's staging size,
 * at least one), not on the list's order or on what else is in it.  Everything is checked before the first device call. */
BNMTF_API int bnmtf_predictive_samples(int device, int I, int J, int K, int L, uint64_t n,
    const int32_t* rows, const int32_t* cols, const float* A, const float* S, const float* B,
    uint64_t first, uint64_t step, int T, int chunk_samples,
    double* p_first, double* sum_d, double* sum_d2);
/* upload and kernel time (ms, from events on the call's stream, summed over its chunks) of the calling host thread's last
 * bnmtf_predictive_samples that returned BNMTF_OK; zeros before one did (tools/predictive_rates.py) */
BNMTF_API int bnmtf_predictive_times(double* upload_ms, double* kernel_ms);

/* ---- the n best predicted entries per row, selected on the device (bnmtf_amd.top_entries) --------------
 * No handle: the call makes its own stream and buffers on `device` and frees all of them on every path.  Score of (i, j): L = 0,
 * S null: A [I][K] . B [J][K]; L >= 1: (A [I][K] S [K][L]) . B [J][L]; 1 <= I, J <= 2^30, 1 <= K <= 256, 0 <= L <= 256, every
 * value finite.  A score is the fp64 fma chain over the inner index ascending from 0.0 ((A S)_l first, over k ascending): its bits
 * depend on the pair's factor rows alone.  rows: n_rows distinct rows of the matrix, any order; null: all I rows (n_rows is then
 * not read).  ex_rows, ex_cols: n_excl < 2^32 entries inside the matrix that are no candidates, any order, repeats allowed; those of
 * rows not asked for are dropped.  Per row asked for, in the order given, the BNMTF_TOP_MAX_N >= n >= 1 best candidates under the
 * total order "higher score first (largest = 1; lower first with largest = 0), equal scores: lower column first, -0.0 equal to
 * 0.0": cols_out [.][n] best first and -1 where the row has fewer than n candidates, scores_out [.][n] with nan there, counts_out
 * [.] the valid slots.  split: column segments per row, each taken by a wave of its own and merged under the same order (0: the
 * library chooses; at most 1024); the answer is unique, so its bytes depend on neither split nor the launch.  Everything is
 * checked, the exclusion list sorted by row and the rows asked for gathered before the first device call. */
#define BNMTF_TOP_MAX_N 128
BNMTF_API int bnmtf_top_entries(int device, int I, int J, int K, int L,
    const double* A, const double* S, const double* B,
    uint64_t n_rows, const int32_t* rows,
    uint64_t n_excl, const int32_t* ex_rows, const int32_t* ex_cols,
    int n, int largest, int split,
    int32_t* cols_out, double* scores_out, int32_t* counts_out);
/* upload and kernel time (ms, from events on the call's stream) of the calling host thread's last bnmtf_top_entries that returned
 * BNMTF_OK; zeros before one did (tools/top_entries_rates.py) */
BNMTF_API int bnmtf_top_entries_times(double* upload_ms, double* kernel_ms);

/* ---- fold new rows or columns into a fitted model, the chains on the device (bnmtf_amd.fold_in) --------
 * No handle: the call makes its own stream and buffers on `device` and frees all of them on every path.  other [m][W]: the factor
 * that stays fixed, 1 <= m <= 2^30, 1 <= W <= BNMTF_FOLDIN_MAX_RANK; the device takes it in fp32.  The new units' entries: 1 <= n <
 * 2^31 triples (unit[e], idx[e], values[e]) with 0 <= unit < n_units and 0 <= idx < m, sorted by (unit, idx), no entry twice, every
 * unit at least once.  lambda, init [n_units][W]: each unit's prior rates (>= 0) and the start of its chain; tau > 0; ids [n_units]:
 * the element word of each unit's Philox counter (null: 0 .. n_units - 1).  Per unit, for t = 0 .. iterations - 1 and then k = 0 ..
 * W - 1, the conditional of x_k given the fixed factor, fp32: update 0 draws from TN(mu, tau_p) -- counter
 * (id, k, first_iteration + t, stream 4 | candidate), key = seed, first accepted candidate --, update 1 sets max(max(0, mu), min_x).
 * Outputs [n_units][W] over the kept sweeps discard, discard + keep_every, ... < iterations, in that order: first_out = x of the
 * first kept sweep, sum_d_out = sum (x_t - first), sum_d2_out = sum (x_t - first)^2, in fp64; the caller finishes mean = first +
 * sum_d / count and variance = max(0, sum_d2 / count - (sum_d / count)^2).  update 1 takes discard = 0 and keep_every = 1 and keeps
 * the final state alone.  samples_out: null, or [iterations][n_units][W] fp32, every sweep's x.  One launch, a wave per unit.  form:
 * 0 -- a unit of at most 512 entries keeps its residual in registers, a longer one in device memory --, 1 -- every unit the second
 * way; a unit's numbers depend on its own entries, rates, start, id, tau, seed, the fixed factor and the chain's parameters alone:
 * not on form, not on the other units or its place among them.  Everything is checked before the first device call. */
#define BNMTF_FOLDIN_MAX_RANK 256
BNMTF_API int bnmtf_fold_in(int device, int n_units, int m, int W, const double* other,
    uint64_t n, const int32_t* unit, const int32_t* idx, const float* values,
    const double* lambda, double tau, const double* init, const uint32_t* ids, uint64_t seed,
    int iterations, int first_iteration, int discard, int keep_every, int update, double min_x, int form,
    double* first_out, double* sum_d_out, double* sum_d2_out, float* samples_out);
/* upload and kernel time (ms, from events on the call's stream) of the calling host thread's last bnmtf_fold_in that returned
 * BNMTF_OK; zeros before one did (tools/fold_in_rates.py) */
BNMTF_API int bnmtf_fold_in_times(double* upload_ms, double* kernel_ms);

/* ---- closed-form predictive mean and variance under a mean-field q over an entry list (bnmtf_amd.variational_predictive;
 * DESIGN.md section 2.8a) -------------------------------------------------------------------------------------------------------
 * No handle: the call makes its own stream and buffers on `device` and frees all of them on every path.  The means E* and
 * variances V* of q, fp64, contiguous: EA, VA [I][K]; L = 0: ES and VS null, EB, VB [J][K]; L >= 1: ES, VS [K][L], EB, VB [J][L];
 * 1 <= K <= BNMTF_PREDICTIVE_Q_MAX_RANK, 0 <= L <= BNMTF_PREDICTIVE_Q_MAX_RANK.  Any of VA, VS, VB may be null: that factor is
 * fixed, its variance zero.  Every mean is finite, every variance finite and >= 0.  Per entry e = (rows[e], cols[e]) -- any
 * order, an entry may occur more than once, 1 <= n < 2^31 -- with f, a = EA[i], VA[i]; s, b = ES, VS; g, c = EB[j], VB[j]:
 *   L = 0   mean_out[e] = sum_k f_k g_k          var_out[e] = sum_k [ a_k g_k^2 + c_k (f_k^2 + a_k) ]
 *   L >= 1  mean_out[e] = sum_l (f S)_l g_l      var_out[e] = sum_k a_k (S g)_k^2 + sum_l [ c_l ((f S)_l^2 + u_l) + (g_l^2 + c_l) w_l ]
 *           u_l = sum_k a_k s_kl^2,  w_l = sum_k b_kl (f_k^2 + a_k)
 * the variance of the product under q, whose entries are independent; the noise of an observation is not in it.  All fp64, every
 * sum an fma chain over its index ascending from 0.0: an entry's two numbers depend on that entry and the moments alone, not on the
 * list's order or on what else is in it.  Device memory is O((I + J)(K + L) + K L + n).  Everything is checked before the first
 * device call. */
#define BNMTF_PREDICTIVE_Q_MAX_RANK 256
BNMTF_API int bnmtf_predictive_moments(int device, int I, int J, int K, int L, uint64_t n,
    const int32_t* rows, const int32_t* cols,
    const double* EA, const double* VA, const double* ES, const double* VS, const double* EB, const double* VB,
    double* mean_out, double* var_out);
/* upload and kernel time (ms, from events on the call's stream) of the calling host thread's last bnmtf_predictive_moments that
 * returned BNMTF_OK; zeros before one did (tools/predictive_q_rates.py) */
BNMTF_API int bnmtf_predictive_moments_times(double* upload_ms, double* kernel_ms);

/* ---- log predictive density of known values under stored samples over an entry list (bnmtf_amd.log_predictive; DESIGN.md
 * section 2.8b) -----------------------------------------------------------------------------------------------------------------
 * bnmtf_predictive_samples' arguments, checks and walk, and with them values [n], fp64 and finite: the known value r_e of entry e;
 * c, h [T], per selected sample s = 0 .. T - 1: c_s = (log tau_s - log 2 pi) / 2, finite, and h_s = tau_s / 2, finite and > 0,
 * formed by the caller (the device takes no logarithm).  Per entry and sample, with p_s as bnmtf_predictive_samples forms it, the
 * Gaussian log-likelihood l_s = fma(-(h_s d), d, c_s), d = r_e - p_s, in fp64.  Outputs [n] in the given order: l_first = l_0,
 * sum_d = sum_s (l_s - l_0), sum_d2 = sum_s (l_s - l_0)^2 (fma), l_max = max_s l_s and sum_exp = sum_s exp(l_s - l_max), kept as a
 * running maximum: from l_max = l_0, sum_exp = 1, in ascending s, l_s > l_max: sum_exp = fma(sum_exp, exp(l_max - l_s), 1), l_max =
 * l_s; else sum_exp += exp(l_s - l_max).  The caller finishes lpd_e = l_max + log(sum_exp) - log(T), the mean l_first + sum_d / T
 * and the variance (sum_d2 - sum_d^2 / T) / (T - 1).  An entry's five numbers depend on that entry, its value and the samples
 * alone -- not on chunk_samples, not on the list's order or on what else is in it.  Everything is checked before the first device
 * call. */
BNMTF_API int bnmtf_log_predictive_samples(int device, int I, int J, int K, int L, uint64_t n,
    const int32_t* rows, const int32_t* cols, const double* values, const float* A, const float* S, const float* B,
    uint64_t first, uint64_t step, int T, int chunk_samples, const double* c, const double* h,
    double* l_first, double* sum_d, double* sum_d2, double* l_max, double* sum_exp);
/* upload and kernel time (ms, from events on the call's stream, summed over its chunks) of the calling host thread's last
 * bnmtf_log_predictive_samples that returned BNMTF_OK; zeros before one did (tools/log_predictive_rates.py) */
BNMTF_API int bnmtf_log_predictive_times(double* upload_ms, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* BNMTF_HIP_H */
