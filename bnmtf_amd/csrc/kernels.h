// Kernel launch interface shared by api.hip and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bnmtf {

// RNG stream ids (counter word 3, low 4 bits) -- same numbers as oracle/rng.py
constexpr uint32_t kStreamRows = 0, kStreamCols = 1, kStreamS = 2, kStreamTau = 3, kStreamFoldIn = 4, kStreamHook = 8;

// ---------------------------------------------------------------------------
// K1/K2: masked contraction  out[n][KP] = sum_inner big[inner][n] * X[inner][KP]
//   big  : R~ shard stored so that the OUTPUT index is the contiguous one
//          (rows step:  big[j][i] = R~[i][j];   cols step: big[i][j] = R~[i][j])
//   X    : the other factor, row-major, padded rows are zero
//   slabs: [split][n_pad][KP] partial sums, summed by the consumer (sweep prologue)
// ---------------------------------------------------------------------------
struct GemmArgs {
  const float* big; int ld;          // leading dimension of big (= n_pad)
  const float* X;                    // [inner_pad][KP]
  float* slabs;                      // [split][n_pad][KP]
  int n_pad, split, inner_per_wave;  // inner range of wave w in split s: [(s*4+w)*ipw, +ipw)
  int tw;                            // 32-column tiles per wave: 4 (128 columns) or 2 (64 columns, short output sides)
  int split0 = 0, nsplit = 0;        // this launch's inner slices [split0, split0 + nsplit) (nsplit = 0: all `split` of them)
};
void launch_gemm(const GemmArgs& a, int KP, hipStream_t st);

// ---------------------------------------------------------------------------
// VB (kernel_maskgemm.hip): out[u][0:2KP] = sum_{r in miss(u)} [S2o | Eo^2][r][:] as a product with the mask's bits
//   bits : [ldw][n_pad] u32, bit b of word w = entry (unit, inner 32 w + b) is missing (zero beyond the inner extent)
//   XB   : the moments of the other factor on a per-column fixed-point grid (2^(cexp[c] - 22)) as three planes of balanced
//          base-256 digits in fragment layout [3][rows_pad / 16][2 KP][16 bytes]; umax: scratch of vb_colmax_kernel
//   slabs: [split][n_pad][2 KP] fp32 partial sums (one per inner slice; integer inside), added by the consumer in slab order
// ---------------------------------------------------------------------------
struct MaskGemmArgs {
  const uint32_t* bits; int ldw;
  const uint32_t* XB; int rows_pad; const int* cexp;
  float* slabs;
  int n_pad, split, inner_per_wave;      // inner_per_wave: inner rows of a BLOCK's slice here (its four waves share the slice and split the columns)
  int ncol = 0;                  // 2 KP (set by launch_maskgemm)
};
void launch_maskgemm(const MaskGemmArgs& a, int KP, hipStream_t st);
// umax [2 KP]: the column maxima's bits.  have_max: already there (the relayout's Gram blocks and gram_reduce_kernel: PostArgs::umax);
// otherwise a pass of its own takes them first
void launch_vb_planes(const float* S2, const float* E, int rows, int rows_pad, int KP, unsigned* umax, bool have_max, int* cexp, uint32_t* XB, hipStream_t st);
void launch_mask_bits(const uint8_t* M, int I, int J, int by_rows, int unit0, int n, int m, int n_pad, int ldw, uint32_t* bits, hipStream_t st);

// ---------------------------------------------------------------------------
// Gram: C[a][b] = sum_r X[r][a] X[r][b] (fp64 accumulate), colsum[a] = sum_r X[r][a]
//   also for VB: colsum2[a] = sum_r S2[r][a] when S2 != nullptr
// ---------------------------------------------------------------------------
struct GramArgs {
  const float* X; const float* S2; int rows, KP;
  double* C64; float* C32; double* colsum; double* colsum2;
};
void launch_gram(const GramArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// K3: sequential-k conditional update of one factor (one half sweep)
// ---------------------------------------------------------------------------
enum SweepMode { kSweepDraw = 0, kSweepMode = 1, kSweepVB = 2 };

struct SweepArgs {
  int n, n0;                 // local units, global index of the first
  const int* unit_list;      // generic kernel: when non-null, the n units to process (local indices)
  int K, KP;                 // true and padded width
  int mode;                  // SweepMode
  int cond_k;                // >= 0: only evaluate column cond_k, write numer/tau, change nothing
  int qinit_only;            // generic kernel: compute q = X_i . Xo_j on the missing entries and stop
  int only_k;                // >= 0 (VB hooks): update only this column (update_U(k) / update_V(k))
  uint32_t col0;             // this factor holds columns [col0, col0 + K) of a wider factorisation (ranks above 64 run as column blocks:
                             // bnmf_set_column_block): the Philox column word of local column k is col0 + k
  float min_x;               // mode updates: lower clamp of the new value (ICM minimum_TN; 0 otherwise)
  int vb_moments;            // VB: also refresh exp/var from the new mu/tau (update_exp_U(k))
  double* vb_stats;          // VB: [n][8] per-unit ELBO / exp_square_diff partial sums (may be null)
  // numerators
  const float* slabs; int split, n_pad;
  const float* lambda;       // [n][KP] local
  // own factor (global, row-major [*][KP]) and its transposed copy [KP][ldT]
  float* Xself; float* XselfT; int ldT_self;
  // other factor, transposed [KP][ldT_o]; index m_sentinel reads 0
  const float* XoT; int ldT_o;
  const float* C32;          // Gram of other factor [KP][KP]
  // missing-entry slots (64 per unit row-step)
  const uint32_t* slot_ptr; const uint32_t* idx; float* q;
  // precision
  const float* tau;          // device scalar
  // RNG
  uint32_t key0, key1, it, stream;
  // outputs
  double* acc;               // [0] += sum P.X', [1] += sum_miss q, [2] += sum_miss q^2 (may be null)
  double* numer_out; double* tau_out;   // cond mode, length n
  // VB extras (mode == kSweepVB)
  float* mu_self; float* tau_self; float* var_self; float* S2self; float* S2selfT;
  const float* S2oT; const double* colsum2_o;   // other's var+exp^2 (transposed) and its column sums
  // variational tri-factorisation (kernel_trivb.hip): covariance term of update_F / update_G and the column order
  const float* cov_S;        // E[S]; element (column c of this factor, inner t) at cov_S[c * cov_sc + t * cov_st]; null: no term
  int cov_sc, cov_st, cov_n; // strides and inner extent (L for the F step, K for the G step)
  const float* cov_mv;       // [n][32] masked variance sums of the other factor (mvG / mvF), local units
  const int* order;          // K column indices in update order, or null (0 .. K-1)
};
void launch_sweep(const SweepArgs& a, hipStream_t st);

// on-chip path (sweep_chip.inc): bank-aware slot layout, q in registers, panels in LDS
struct FastArgs {
  const int* unit_map;         // [2*npairs] local unit of each half wave, or -1
  const uint32_t* pair_E;      // [npairs] slots of the pair (max of its two units)
  const uint32_t* pair_base;   // [npairs] first slot row of the pair
  const uint32_t* off;         // [(base+s)*64 + lane] inner index j (j mod 32 == lane mod 32) or mz + lane%32
  const uint32_t* off16;       // [(base/2+h)*64 + lane] slots 2h (low 16 bits) and 2h+1 (high) packed, or null
  int nw;                      // unit waves per block (2, 4, 8 or 16)
  int npairs;                  // pairs in descending slot-count order
  int mz, pw;                  // inner extent rounded up to 32 (sentinel zero words at mz..mz+31); panel floats pw = round_up(mz+32, 256)
  // an inner extent too long for one LDS panel (round 3): the inner indices are cut in TWO chunks, [0, mh) and [mh, m); a
  // unit's slots are its chunk-0 entries (first half of its slot rows) then its chunk-1 entries, inner indices LOCAL to the
  // chunk; a column is staged and gathered chunk by chunk (nch = 2, sweep_chip.inc); pw = the longer chunk's panel floats.
  int nch, mh, pw1;            // chunks (1 or 2), first inner index of chunk 1 (multiple of 256), panel floats of chunk 1
  // q hand-over between the half sweeps (16-wave kernel, one GPU; model.h Dir::ho_*): read q from the block's region instead of
  // the pre-pass / write q sorted by the other direction's blocks at the end
  int twin;                    // the twin shape: 8-wave blocks, two to a CU, on the 16-wave layout (sweep_chip.inc)
  int ho_lds_floats;           // floats behind the Gram in LDS that the hand-over's region / staging area needs (0: none)
  int ho_read, ho_write, ho_nb_other, ho_rows_total;       // ho_rows_total: slot rows of the whole direction (= the end of the last block's slice)
  const uint32_t* ho_in; const float* ho_region; const uint32_t* ho_region_ofs;
  const uint32_t* ho_out; const uint32_t* ho_pk; float* ho_dst;
  const float* XoT; int ldT_o;   // other factor transposed [KP][ldT_o]
  const float* XoT2; int ld2_o;  // other factor, column pairs interleaved [KP/2][ld2_o][2]
  const float* Xo; int Xo_rows;  // other factor row major [Xo_rows][KP] (kernel_sweep_unit.hip: q rebuilt from its rows)
  double* stats;               // [blocks][4] partial (sum P.X', sum_miss q, sum_miss q^2) or null
  // VB sweep (kernel_sweep_vb.hip)
  const float* XoS;            // other factor's (E, S2) pair panels [KP][ld2_o][2]
  float* vb_asq; float* vb_vsq;  // [rows][KP] per (unit, column): sum_miss S2other, sum_miss Eother^2 (for VbPieces)
  // VB on the on-chip kernels (sweep_chip.inc, MODE = kSweepVB): the two masked sums of every (unit, column), from
  // kernel_maskgemm.hip: [msplit][n_pad][2 KP] slabs, columns [0, KP) = sum_miss S2other, [KP, 2 KP) = sum_miss Eother^2
  const float* mslabs; int msplit;
};
// 2/4/8-wave instantiations (kernel_sweep_fast.hip): pairs that need more than kFastMaxSlots slots per lane go to the generic kernel
constexpr int kFastMaxSlots = 56;
bool sweep_fast_supported(int KP, int pw);
// an inner extent m too long for one LDS panel: can it be cut in two chunks [0, mh) and [mh, m) that fit one each?  Then mh (a
// multiple of 256), the panel floats of the longer chunk (pw: LDS sizing) and of chunk 1 (pw1).
bool sweep_two_chunks_plan(int KP, int m, int* mh, int* pw, int* pw1);
void launch_sweep_fast(const SweepArgs& a, const FastArgs& f, hipStream_t st);
void launch_sweep_small(const SweepArgs& a, const FastArgs& f, hipStream_t st);   // nw = 2, 4 (kernel_sweep_small.hip)
// one unit per 64-lane wave, f.nw = 4 or 8 unit waves + a staging wave per block (kernel_sweep_unit.hip): few units per CU --
// shards of a multi-GPU run, small problems.  The layout: Dir::u_* (both halves of a pair hold entries of the same unit)
constexpr int kUnitMaxUnits = 2048;          // local units of a direction up to which the shape is used: eight per CU
constexpr int kUnitMaxSlots = 32;            // ... and slots per lane (2 048 missing entries per unit); a direction with a fuller unit keeps the pair layout's kernels
bool sweep_unit_supported(int KP, int pw);
void launch_sweep_unit(const SweepArgs& a, const FastArgs& f, hipStream_t st);
// 16-wave instantiation (kernel_sweep_wide.hip): at most kWideMaxSlots slots per lane, 16 pairs per block
constexpr int kWideMaxSlots = 32;
constexpr int kTwinPanelStride = 8448;       // the twin shape (sweep_chip.inc, TW = 1): floats between its two panel buffers = the largest panel it takes
bool sweep_wide_supported(int KP, int pw);
void launch_sweep_wide(const SweepArgs& a, const FastArgs& f, hipStream_t st);
// the same pair layout run by 8-wave blocks of four units per wave, two groups of units taking turns so that a group's draw
// is made during the other group's slot work (kernel_sweep_turns.hip; an experiment kept behind BNMTF_TURNS=1: correct,
// slower than the 16-wave kernel -- DESIGN.md section 7.3)
bool sweep_turns_supported(int KP, int pw);
void launch_sweep_turns(const SweepArgs& a, const FastArgs& f, hipStream_t st);
// VB sweep in the 16-wave shape (kernel_sweep_vb.hip) and the ELBO pieces it leaves to a second pass
bool sweep_vb_supported(int KP, int pw);
bool sweep_vb_cov_supported(int KP, int pw);   // ... with SweepArgs::cov_S / order: the tri-factorisation's F / G sweeps (K, L <= 32)
int sweep_vb_blocks(int npairs, int nw = 8);  // blocks (= rows of FastArgs::stats) of a VB sweep over npairs pairs with nw unit waves per block (16 or 8)
// order_step (recording, many.h; the tri-factorisation's sweeps): entries between the column orders of consecutive iterations
void launch_sweep_vb(const SweepArgs& a, const FastArgs& f, hipStream_t st, int order_step = 0);
void launch_vb_pieces(int n, int n0, int KP, int K, const float* mu, const float* tauq, const float* ex, const float* var,
                      const float* lambda, const float* asq, const float* vsq, double* out, hipStream_t st);
// the same pieces with the two masked sums taken from the slabs of kernel_maskgemm.hip (the on-chip VB sweep)
void launch_vb_pieces_slabs(int n, int n0, int KP, int K, const float* mu, const float* tauq, const float* ex, const float* var,
                            const float* lambda, const float* mslabs, int msplit, int n_pad, double* out, hipStream_t st);

// relayout + Gram after a sweep / state upload: X -> XT, XT2, partial Gram slabs; then the reduction
struct PostArgs {
  const float* X; int rows, KP;
  float* XT; int ldT; float* XT2; int ld2;
  double* Cpart; double* spart;          // [blocks][KP*KP], [blocks][KP]
  double* C64; float* C32; double* colsum;
  // VB: second moment matrix S2 = var + exp^2
  const float* S2; float* S2T; double* s2part; double* colsum2;
  float* XS;                             // VB: [KP][ldT][2] (E, S2) interleaved per row: pair panels of the fast VB sweep, or null
  float* mpart; unsigned* umax;          // VB, whole-factor launches (or null): per-block and final column maxima of [S2 | E^2] (kernel_maskgemm.hip)
  // which half of the work a launch does (launch_post: both, every row).  Several GPUs: the Gram partial is formed over the
  // rank's OWN rows [own0, own1) only (blocks blk0 .. of 32 rows; rows outside the range count as zero) and the partial
  // C64 | colsum is summed over the ranks by one all-reduce; the layouts are written for all rows once they are gathered.
  int do_layout, do_gram, blk0, own0, own1;
  // the sample hand-off of run(): the layout blocks also write the rows packed [rows][snapW] into a snapshot slot (what a
  // separate compaction kernel did), or null
  float* snap; int snapW;
};
void launch_post(const PostArgs& a, hipStream_t st);
void launch_post_layout(const PostArgs& a, hipStream_t st);                       // XT / XT2 (/ S2T / XS) of every row
void launch_post_gram_rows(const PostArgs& a, int own0, int own1, hipStream_t st);   // C64, colsum (, colsum2) of the rows [own0, own1) only
// bnmtf_create's passes over the I x J data, on the device (kernel_layout.hip): the masked (and, for the rows direction, transposed)
// contraction operand big[r][ul], and every unit's missing inner indices in order (64-wide slots, padded with m)
void launch_masked_operand(const float* R, const uint8_t* M, int I, int J, int by_rows, int unit0, int n, int m, float* out, int ld, hipStream_t st);
// the same operand for the RESIDUAL data of a column block: M ? R - sum_b A_b[i] . B_b[j] : 0 (up to kMaxOtherBlocks products of
// width W_b, row-major [.][KP_b] factors): what the other column blocks of a wider factorisation explain is taken off the data
constexpr int kMaxOtherBlocks = 4;      // (a model of four column blocks has three others; the S blocks of a wide tri-factorisation take four carriers)
struct ResidualSpec { int n; const float* A[kMaxOtherBlocks]; const float* B[kMaxOtherBlocks]; int KP[kMaxOtherBlocks]; int W[kMaxOtherBlocks]; };
void launch_residual_operand(const float* R, const uint8_t* M, int I, int J, int by_rows, int unit0, int n, int m, float* out, int ld,
                             const ResidualSpec& rs, hipStream_t st);
void launch_missing_lists(const uint8_t* M, int I, int J, int by_rows, int unit0, int n, int m, const uint32_t* ptr, uint32_t* idx, hipStream_t st);
// q hand-over tables of one writer / reader pair of directions, built on the device (kernel_handover.hip)
struct HandoverArgs {
  // the writer's and the reader's slot layouts (FastArgs::off, pair_base, pair_E, unit_map), pairs, pairs per block (the sweep
  // kernel's unit waves: 16 or 8), blocks, inner extents
  const uint32_t* w_off; const uint32_t* w_pB; const uint32_t* w_pE; const int* w_umap; int w_npairs, w_ppb, w_nb; uint32_t w_inner;
  const uint32_t* r_off; const uint32_t* r_pB; const uint32_t* r_pE; const int* r_umap; int r_npairs, r_ppb, r_nb; uint32_t r_inner;
  const uint16_t* r_row_blk;                 // reader: block of every slot row
  const uint32_t* r_ptr; const uint32_t* r_idx;   // reader: sorted missing inner indices per unit (Dir::slot_ptr, Dir::idx)
  // scratch
  uint32_t* inv; uint32_t* dst_slot; uint32_t* dst_rank; uint32_t* count;
  uint32_t* sbase; uint32_t* stotal; uint32_t* rbase; uint32_t* rdata; uint32_t* rsize;
  // results
  uint32_t* rofs; uint16_t* t_out; uint16_t* t_in; uint32_t* pk;
  uint32_t* limits;                          // [0] longest staging area, [1] largest region, [2] entries without a partner, [3] all regions (entries)
};
void launch_handover_build(const HandoverArgs& a, hipStream_t st);
void launch_gram_cast(const double* C64, float* C32, int n, hipStream_t st);      // C32 = (float) C64 after the partial sums were all-reduced
constexpr int kPostRows = 32;
inline int post_blocks(int rows) { return (rows + kPostRows - 1) / kPostRows; }
// threads per block of the kernels behind a half sweep (post_kernel, gram_reduce_kernel) and of the end of a Gibbs iteration
// (finish_kernel): with their register counts, what lets them run beside the contraction (tests/test_tail_resources_cpu.py)
constexpr int kPostThreads = 256, kGramReduceThreads = 1024, kFinishThreads = 512;

// ---------------------------------------------------------------------------
// end of iteration: masked SSE from Gram identities, tau draw, metrics record
// ---------------------------------------------------------------------------
struct FinishArgs {
  const double* Cr64; const double* Cc64; const double* sr; const double* sc; int KP;
  const double* acc;          // [3] atomically accumulated sums (generic sweep)
  const double* stats; int nstats;   // [nstats][4] per-block partial sums (fast sweep), may be null
  double n_obs, sumR, sumR2;  // over the training mask
  double alpha, beta;
  int update;                 // 0 draw, 1 mode (tau = alpha_s/beta_s), 2 ICM (tau = (alpha_s - 1)/beta_s, gamma_mode)
  uint32_t key0, key1, it;
  const double* gunit;        // update 0: the Gamma(alpha_s, 1) variate of this iteration, computed ahead on the host (stage_gamma_variates); else unused
  double* tau_d; float* tau_f;
  double* rec;                // [5]: tau, MSE, R2, Rp, SSE  (slot of this iteration)
  const float* copy_src; float* copy_dst; int copy_n;     // a small array that rides along (the tri-factorisation's sample of S into its slot), or null
};
void launch_finish(const FinishArgs& a, hipStream_t st);
struct VbFinishArgs {
  const double* Cr64; const double* Cc64; const double* sr; const double* sc; const double* s2r; const double* s2c; int KP;
  const double* acc;                   // [3] sum P.X', sum_miss q, sum_miss q^2 (cols sweep)
  const double* stats_r; int nr;       // [nr][8] rows-sweep per-unit sums
  const double* stats_c; int nc;       // [nc][8] cols-sweep per-unit sums
  double n_obs, sumR, sumR2, alpha, beta;
  double* tau_d; float* tau_f;         // exptau
  double* rec;                         // [16]: exptau, MSE, R2, Rp, ESD, beta_s, then 4 ELBO sums for U and 4 for V
  const double* extra; int n_extra;    // (tri-factorisation: partial sums of exp_square_diff's third term, added to ESD; null: none)
  const double* sweep_stats; int n_sweep_stats;    // [n][4] per-block sums of the on-chip cols sweep, added to acc here (null: acc holds everything)
};
void launch_vb_finish(const VbFinishArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// direct masked metric sums in fp64 (predict / validation path)
// ---------------------------------------------------------------------------
struct MetricArgs {
  const float* R; const uint8_t* Mp; int I, J;
  const double* A; const double* B; int K;     // A [I][K], B [J][K]
  const double* A2; const double* B2;          // optional (VB): second-moment factors; out[6] = sum_mask (A2_i.B2_j - sum_k A_ik^2 B_jk^2)
  double* out6;                                // 8 doubles
  double* part;                                // metric_tiles(I, J) x 8 doubles: the tiles' partial sums
};
inline size_t metric_tiles(int I, int J) { return (size_t)((I + 31) / 32) * (size_t)((J + 31) / 32); }
void launch_metric_sums(const MetricArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// BNMTF (kernel_bnmtf.hip)
// ---------------------------------------------------------------------------
struct SmallProductArgs {   // out = X . S (transposeS = 0, out width L) or X . S^T (transposeS = 1, out width K)
  const float* X; int rows, KPin; const float* S; int K, L; int transposeS; float* out; int KPout;
};
void launch_small_product(const SmallProductArgs& a, hipStream_t st);
struct SlabProductArgs {    // out[n][KPout] = (sum of the `split` slabs [n_pad][KPin]) . S: contraction slabs times S (kernel_bnmtf.hip)
  const float* slabs; int split, n_pad, KPin; const float* S; int K, L; int n; float* out; int KPout;
  int transposeS = 0;          // 1: out[n][K] = slabs[n][L] . S^T (the F side: R~ (G S^T) = (R~ G) S^T); out may be slab 0 of `slabs` when KPout == 32
};
void launch_slab_product(const SlabProductArgs& a, hipStream_t st);
void launch_cfs(const double* Cf64, int KPk, const float* S, int K, int L, float* CfS, hipStream_t st);
struct SRowArgs {           // one row k of S: J-vectors h_k, w_k and per-block partial eta / Omega
  int n, n0, k, K, L, KPk, KPl;
  const float* G;                      // [J][KPl]
  const float* FT; int ldT;            // F transposed [KPk][ldT]
  const float* slabs; int split, n_pad;   // Pv = R~^T F partial slabs, width KPk
  const uint32_t* slot_ptr; const uint32_t* idx; float* q;   // generic (64-wide) slots of the cols direction
  const float* CfS;                    // [K][L] current Cf.S
  const float* delta_prev; int apply_prev;   // delta of row k-1: q += F_{i,k-1} (G_j . delta) before use
  float* partial;                      // [blocks][L]: per-block share of eta
};
constexpr int kSOmegaChunks = 8;       // column chunks of the Omega^k partial sums
struct SOmegaArgs {         // w[j][k] and the chunk partials of Omega^k for every k (once per iteration)
  int n, n0, K, L, KPk, KPl, nch, zero_row;
  const float* F;                      // [I+][KPk] row major (row zero_row is zero)
  const float* G;                      // [J][KPl]
  const float* Cf32;                   // F^T F [KPk][KPk]
  const uint32_t* slot_ptr; const uint32_t* idx;
  float* w;                            // [J][KPk]
  float* omp;                          // [K][nch][LP*LP]
};
void launch_srow_omega(const SOmegaArgs& a, hipStream_t st);
void launch_srow_qinit(const SOmegaArgs& a, const float* Ueff, float* q, hipStream_t st);   // q = (F S)_i . G_j on the column slots (KPl == 32)
void launch_srow_gather(const SRowArgs& a, int blocks, hipStream_t st);
struct SDrawArgs {
  int k, K, L, KPk, nblocks, update, cond_l, LP, nch;
  float min_x;                         // mode updates: lower clamp (ICM minimum_TN)
  const float* partial; const float* omp; float* S; const float* lambdaS; const float* tau;
  const double* Cf64; float* CfS; float* delta_out;
  uint32_t key0, key1, it;
  uint32_t word0; int ldword;          // the Philox column word of entry (k, l) is word0 + k ldword + l: (0, L) for a whole S, (row0 Lw + col0, Lw) for a block of a wider one
  double* numer_out; double* tau_out;
};
void launch_srow_draw(const SDrawArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// BNMTF S step as a dense K.L x K.L system (kernel_ssys.hip); K, L <= 32
// ---------------------------------------------------------------------------
// packed upper triangle of a symmetric index pair (k <= k' < K): p = k K - k (k - 1) / 2 + (k' - k); rows of the packed
// arrays are padded to a multiple of 64 (the GEMM's 2 x 2 MFMA tiles) with zeros
__host__ __device__ inline int tri_count(int K) { return K * (K + 1) / 2; }
__host__ __device__ inline int tri_padded(int K) { return (tri_count(K) + 63) / 64 * 64; }
__host__ __device__ inline int tri_index(int k, int kp, int K) { return k * K - k * (k - 1) / 2 + (kp - k); }
// where packed entry p sits in its row: the two 32-entry tiles of a 64-group are interleaved word by word, so that one
// 8-byte load gives a lane its element of both tiles
__host__ __device__ inline int tri_pos(int p) { return (p & ~63) + 2 * (p & 31) + ((p >> 5) & 1); }
__host__ __device__ inline int tri_unpos(int pos) { return (pos & ~63) + 32 * (pos & 1) + ((pos & 63) >> 1); }   // inverse of tri_pos
__host__ __device__ inline void tri_unindex(int p, int K, int* k, int* kp) {
  int kk = 0;
  while (p >= K - kk) { p -= K - kk; ++kk; }
  *k = kk; *kp = kk + p;
}
struct SColGramArgs {       // W~_j = C~f - sum_{i in miss(j)} (F_i F_i^T + diag varF_i) for the local columns
  int n, K;
  const float* F;                      // [I+][32] row major, padding slots of idx point at a zero row
  const float* varF;                   // [I+][32] or null (Gibbs)
  const double* Cf64;                  // F^T F [32][32]
  const double* cf_diag_extra;         // VB: sum_i (E[F_ik]^2 + varF_ik) [32] (replaces the diagonal of Cf64), or null
  const uint32_t* slot_ptr; const uint32_t* idx;   // 64-wide slots of the cols direction
  float* Wc;                           // [n + 2][tri_padded(K)]: the packed upper triangle of W~_j (pads and the two extra rows stay zero)
  float* var_obs_out = nullptr;        // VB with varF: [n][32] the observed rows' variance sums (total minus the gathered missing ones) go here -- the G step's mv
  const float* var_obs = nullptr;      // VB, instead of varF: [n][32] sum_{i in Omega_j} varF_ik (the G step's masked variance sums) -- the diagonal's sum over the MISSING rows is the total minus this
};
struct GammaPackArgs;
struct SSysBArgs;
// pack_too.n > 0: the packing of G's second moments in the same launch; b_too != nullptr: and the blocks of b = sum_j Pv_j (x) G_j
void launch_scol_gram(const SColGramArgs& a, const GammaPackArgs& pack_too, hipStream_t st, const SSysBArgs* b_too = nullptr);
struct GammaPackArgs {      // Gc[j][r(l, l')] = G_jl G_jl' (+ varG_jl when l = l': the second moment, VB) for the local columns
  int n, n0, L;
  const float* G; const float* varG;   // [J][32] (global rows n0 + j); varG null for Gibbs
  float* Gc;                           // [n + 2][tri_padded(L)]
};
void launch_gamma_pack(const GammaPackArgs& a, hipStream_t st);
struct SSysGemmArgs {       // slabs[s][p][r] = sum_{j in range s} Wc[j][p] Gc[j][r]: A on the packed pairs p = (k <= k'), r = (l <= l')
  int n, K, L, nsplit;
  const float* Wc; const float* Gc;
  float* slabs;                        // [nsplit][tri_padded(K)][tri_padded(L)]
};
__host__ __device__ inline int ssys_gemm_wave_tiles(int K, int L) { return (tri_padded(K) / 64) * (tri_padded(L) / 64); }
__host__ __device__ inline int ssys_gemm_range(int n, int nsplit) { return ((n + nsplit - 1) / nsplit + 15) & ~15; }     // columns per range of SSysGemmBf16: a multiple of a step
void launch_ssys_gemm(const SSysGemmArgs& a, hipStream_t st);
bool ssys_ab_switch_set();          // an A/B switch of kernel_ssys.hip that has no list form is set (BNMTF_SCOL_GRAM=f32, BNMTF_SSYS_GEMM=f32)
struct SSysBArgs { int n, n0, K, L; const float* slabs; int split, n_pad; const float* G; float* b; };   // b[block][K L]: per 64-column block partials of sum_j Pv_jk G_jl
__host__ __device__ inline int ssys_b_blocks(int n) { return (n + 63) / 64 > 0 ? (n + 63) / 64 : 1; }
void launch_ssys_b(const SSysBArgs& a, hipStream_t st);
void launch_ssys_reduce(const float* slabs, int nsplit, int K, int L, float* A, hipStream_t st);   // sum the slabs on k <= k', mirror
void launch_ssys_sum_parts(const float* parts, int nparts, size_t n, float* out, hipStream_t st);
// r = b - A S.  bparts != nullptr: b is summed from its nparts per-block parts first (and stored).  cands [n2][4][4]: the chain's first candidates (draws)
// tinv != nullptr: K more blocks make Ti_k = (I + N_k)^-1 [K][32][32] for the chain's rows (needs K, L, the device's tau)
void launch_ssys_residual(const float* A, float* b, const float* bparts, int nparts, const float* S, int n2, float* r, hipStream_t st,
                          float* cands = nullptr, uint32_t it = 0, uint32_t key0 = 0, uint32_t key1 = 0,
                          float* tinv = nullptr, int K = 0, int L = 0, const float* tau = nullptr, float* own8 = nullptr, float* recT = nullptr, float* Tn = nullptr);
struct SSysChainArgs {
  int K, L, update, cond;              // update: 0 draw, else mode (clamped from below by min_x); cond >= 0: evaluate entry cond only
  float min_x;
  const float* A; const float* r0; float* S; const float* lambdaS; const float* tau;
  uint32_t key0, key1, it;
  const float4* cands;                 // [K L][4] {-log u1, z, u2, -} of iteration `it` (SSysResidual); draws only
  const float* Tinv;                   // [K][32][32]: (I + N_k)^-1 of every row's diagonal block (SSysResidual's extra blocks)
  const float4* own8; const float4* recT;   // [K L][2] per-entry and [K L][4] per-candidate constants of the draws (SSysResidual)
  const float* Tn;                     // [K L]: the row's own old values up to the entry put back (SSysResidual)
  double* numer_out; double* tau_out;
};
void launch_ssys_chain(const SSysChainArgs& a, hipStream_t st);


// ---------------------------------------------------------------------------
// variational tri-factorisation (kernel_trivb.hip); K, L <= 32
// ---------------------------------------------------------------------------
struct SmallProductVbArgs {  // effective factor: mean out = X.S (or X.S^T) and its second moment outS2
  const float* X; const float* varX; int rows; const float* S; const float* varS; int K, L, transposeS; float* out; float* outS2;
};
void launch_small_product_vb(const SmallProductVbArgs& a, hipStream_t st);
struct MaskedColsumArgs {    // out[u][c] = sum over the unit's observed inner indices of V[.][c]
  int n; const uint32_t* slot_ptr; const uint32_t* idx; const float* V; const double* colsum2; const double* C64; float* out;
};
void launch_masked_colsum(const MaskedColsumArgs& a, hipStream_t st);
struct SSysChainVbArgs {
  int K, L, n_order, only_params;
  const int* order;                    // entries a = k L + l in update order
  const float* A; const float* r0; const float* lambdaS; const float* tau;
  float* E; float* var; float* mu; float* tauq;     // q(S): expS (in/out), varS, muS, tauS  [K L]
  const float* Aperm;                  // whole passes: A~ in the pass's order (launch_ssys_permute), or null
};
// order_step (recording, many.h): entries between the orders of consecutive iterations -- the list form adds it x order_step to order
void launch_ssys_chain_vb(const SSysChainVbArgs& a, hipStream_t st, int order_step = 0);
void launch_ssys_permute(const float* A, const int* order, int n, float* out, hipStream_t st, int order_step = 0);   // out[s][p] = A[order[s]][order[p]]
bool trivb_ab_switch_set();         // an A/B switch of kernel_trivb.hip that has no list form is set (BNMTF_VB_CHAIN=steps)
struct TriFactorArgs { int which, side, rows, K, L; const float* X; const float* varX; const float* S; const float* varS; double* out; };
void launch_tri_factors(const TriFactorArgs& a, hipStream_t st);
// exp_square_diff's third term (bnmtf_vb_optimised.py:238) from the masked variance sums the G step already holds:
//   sum_jk mv[j][k] ((sum_l S_kl G_jl)^2 - sum_l S_kl^2 G_jl^2),  mv[j][k] = sum_{i in Omega_j} varF_ik;  one partial sum per block
struct TriThirdArgs { int rows, K, L; const float* G; const float* S; const float* mv; double* part; };
__host__ __device__ inline int tri_third_blocks(int rows) { return (rows + 7) / 8; }   // eight rows per block
void launch_tri_third(const TriThirdArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// small models (kernel_small.hip): the WHOLE run(n) of a BNMF Gibbs model in one launch, one 16-wave block per model --
// both factors, the Gram matrices and every per-column exchange in the CU's LDS, q of the missing entries in registers,
// R~ streamed from L2 by the block's own f32 MFMA contraction; grid = number of models (the folds / ranks / restarts of a
// model search: code/cross_validation/line_search_cross_validation.py:54-131 run them one after the other).  Same
// conditionals, same Philox keying and candidate sequence as the large path (bnmf_gibbs_optimised.py:133-155, :167-177).
// ---------------------------------------------------------------------------
constexpr int kSmallThreads = 1024;     // threads of the largest block (16 waves = one CU); row stride of the slot tables.  Smaller models run 256- or 512-thread blocks, several to a CU
constexpr int kSmallStride = 33;        // floats per factor row in LDS (odd: a column gather and a row read are both conflict-free)
constexpr int kSmallKP = 32;            // K <= 32
constexpr int kSmallMaxSlots = 64;      // missing entries per entry thread (slot classes 8 / 16 / 32 / 64)
constexpr uint32_t kSmallNone = 0xFFFFFFFFu;
struct SmallDirDev {
  int n, m;                    // units (rows of this direction's factor), inner extent
  int ldb, ldn;                // leading dimensions: big [round_up(m, 4)][ldb], XT / PT [32][ldn]  (multiples of 64)
  int nthreads, em;            // entry threads in use; slots per entry thread
  const float* big;            // masked R, unit index contiguous (rows: big[j][i], cols: big[i][j])
  const float* lambda;         // [n][32] prior rates, zero padded
  const uint16_t* idx;         // [em][1024] 33 j for the inner index j of slot e of entry thread t (33 m: empty -> the zero row)
  const uint16_t* unit_of;     // [1024] unit of entry thread t
  const uint16_t* seg;         // [n][2] first entry thread and number of entry threads of unit u
  const uint32_t* perm;        // [em][1024] where the OTHER direction keeps this slot's q (e' * 1024 + t'), kSmallNone: empty
  float* X;                    // state [n][32] row major
  float* XT;                   // [32][ldn] the same transposed (column k's old values, coalesced over the units)
  float* q;                    // [em][1024] q of the missing entries as this direction's sweep left them
  uint2* tab;                  // [K nc0][ldn] Philox words of the first nc0 candidates of every (unit, column) of a half sweep (nc0 <= 8, nc0 ldn <= 1024)
  double* C64;                 // [32][32] Gram of X
  double* colsum;              // [32]
};
struct SmallLaunch {
  SmallDirDev rows, cols;
  float* PT;                   // [32][cols.ldn] Pv = R~^T U of the cols contraction (for sum_Omega R.Rp)
  int K;
  double n_obs, sumR, sumR2, alpha, beta;
  double* tau_d; float* tau_f;
  // this call
  int n_iter, update; float min_x;
  uint32_t key0, key1; unsigned long long it0;
  int q_valid;                 // cols.q holds q of the current state (left there by the previous call)
  uint32_t refresh;            // the rows sweep rebuilds q from the factors when iteration % refresh == 0
  const double* gunit;         // [n_iter] Gamma(alpha_s, 1) variates (draws)
  double* rec;                 // [n_iter][5] tau, MSE, R^2, Rp, SSE
  unsigned long long* clock;   // [n_iter + 1] wall_clock64 at the start and after every iteration
  float* U_s; float* V_s;      // samples [n_iter][n][K], or null
  double* expR; double* expC; double* exp_tau; int exp_burn, exp_thin;   // posterior sums (bnmtf_set_expectation), or null / -1
  // tri-factorisation (L > 0; bnmtf_gibbs_optimised.py:138-180): rows = F (I x K), cols = G (J x L), S (K x L) between them.  The F
  // sweep sees G S^T as its other factor, the G sweep F S (formed in place in LDS), the K L entries of S are updated one after the
  // other between the two by the whole block (kernel_small.hip, "S step")
  int L;
  float* S;                    // [K][L] state
  const float* lambdaS;        // [K][L] prior rates
  float* ZT;                   // [32][cols.ldn] Pv = R~^T F (k-major): b = Pv^T G of the S step, and (R~^T F) S is the G sweep's contraction
  uint2* stab;                 // [K L][4] Philox words of the first four candidates of every S draw of an iteration
  float* Wg;                   // [cols.n][56] packed second moments of F's rows over a column's missing entries (the dense S step, K, L <= 10)
  float* S_s;                  // samples [n_iter][K][L], or null
  double* expS;                // posterior sum [K][L], or null
};
// the S step's dense form (the K L x K L system in LDS, the chain on one wave: kernel_small.hip) takes the ranks the reference searches
constexpr int kTriDenseK = 10;
__host__ __device__ inline bool small_tri_dense(int K, int L) { return L > 0 && K <= kTriDenseK && L <= kTriDenseK; }
size_t small_lds_bytes(int I, int J, int nt, int K = 0, int L = 0);  // LDS a block of nt threads needs for an I x J model (K, L: the tri-factorisation's ranks)
void launch_small_gibbs(const SmallLaunch* dev_launches, int n_models, int em, int nt, size_t lds_bytes, hipStream_t st, bool tri = false);

// small helpers
void launch_sum_stats(const double* stats, int nblocks, double* acc, hipStream_t st);   // acc[0..2] += column sums of stats
void launch_sum_cols(const double* stats, int nrows, int ld, int ncols, double* out, hipStream_t st);        // out[c] += column sums, ncols <= 8
void launch_compact_rows(const float* X, int rows, int W, int KP, float* dst, hipStream_t st);               // [rows][KP] -> [rows][W]
void launch_accumulate(const float* X, size_t n, double* sum, const double* tau, double* tausum, hipStream_t st);   // sum += X (fp64), *tausum += *tau
void launch_transpose(const float* X, int rows, int KP, float* XT, int ldT, hipStream_t st);
void launch_tn_sample(const double* mu, const double* tau, size_t n, uint64_t seed, uint32_t it, uint32_t col,
                      uint32_t elem0, double* out, hipStream_t st);
void launch_tn_moments(const double* mu, const double* tau, size_t n, double* e, double* v, hipStream_t st);
void launch_gamma_sample(double alpha, double beta, uint64_t seed, uint32_t it, double* out, hipStream_t st);

// ---------------------------------------------------------------------------
// Non-probabilistic NMF / NMTF (kernel_np.hip): multiplicative updates
// ---------------------------------------------------------------------------
struct NpSweepArgs {
  const float* Rn; int n, m;         // [n][m] the data of the n units (NaN where unobserved)
  float* Xt;                         // [K][n] this direction's factor, column major (updated in columns k0 .. k1-1)
  const float* Yt;                   // [K][m] the other factor, column major
  int K, k0, k1;
  double* stats;                     // null, or [blocks][8]: the eight training-mask sums of the final P (np_entry_stats)
};
struct NpSPassArgs {
  const float* Rn; float* P;         // [I][J] (P only on the observed entries)
  const float* Ft; const float* Gt;  // [K][I], [L][J]
  const float* S_in; float* S_out;   // [K][L]
  const double* part_prev;           // [blocks][2] numerator / denominator partials of entry prev (the previous pass's part_cur)
  double* part_cur;                  // [blocks][2] ... of entry cur
  int I, J, K, L;
  int prev, cur;                     // entries (k L + l) this pass finishes / accumulates; -1: none
};
void launch_np_prepare(const float* R, const uint8_t* M, int I, int J, float* Rn, float* RnT, hipStream_t st);
bool np_sweep_supported(int m, int K);
int np_sweep_blocks(int n, int m);
void launch_np_sweep(const NpSweepArgs& a, hipStream_t st);
void launch_np_stats_finish(const double* part, int nb, double* out, hipStream_t st);   // out[8] = column sums of part[nb][8]
void launch_np_small_product(const float* S, int sc, int sa, const float* in, int A, int C, int n, float* out, hipStream_t st);
void launch_np_build_p(const float* Rn, const float* Ut, const float* Yt, int I, int J, int K, float* P, hipStream_t st);
__host__ __device__ inline int np_s_blocks(int I) { return I < 1024 ? I : 1024; }   // blocks of a pass of the S step
void launch_np_s_pass(const NpSPassArgs& a, hipStream_t st);
void record_np_copy(const float* src, float* dst, int n);   // (many.h: a list-form record only) dst[0 .. n) = src[0 .. n)
void launch_np_metrics(const float* R, const uint8_t* M, const float* Ut, const float* Yt, int I, int J, int K, double* part, hipStream_t st);

// ---------------------------------------------------------------------------
// Held-out metric sums of the current factors, once per iteration (kernel_heldout.hip): the six sums of metrics_from_sums over a
// sparse list of entries, fp64, no pass over R
// ---------------------------------------------------------------------------
constexpr int kHeldoutRowsPerBlock = 4;      // a wave per row of R, four waves per block
struct HeldoutArgs {
  const uint32_t* rowptr;            // [I + 1] the held-out entries of row i are [rowptr[i], rowptr[i + 1])
  const uint32_t* col;               // [n] their columns, ascending within a row
  const float* rval;                 // [n] their values of R
  int I;
  const float* A; int KPa, Wa;       // rows factor [I][KPa] (U, or F), Wa columns in use
  const float* B; int KPb, Wb;       // columns factor [J][KPb] (V, or G)
  const float* S; int K, L;          // tri-factorisation: [K][L] unpadded; null: P = A B^T
  double* part;                      // [heldout_blocks(I)][8] the blocks' partial sums
  double* rec;                       // [8] the iteration's record: n, sum R, sum R^2, sum P, sum P^2, sum R P, 0, 0
};
// the same sums for the column-major fp32 factors of a handle of bnmtf_np_create (ranks up to kHeldoutNpMaxRank)
constexpr int kHeldoutNpMaxRank = 256;
struct HeldoutNpArgs {
  const uint32_t* rowptr; const uint32_t* col; const float* rval;      // as above
  const float* Xr;                   // [K][I] U, or F
  const float* Xc;                   // [K][J] V, or [L][J] G
  const float* S;                    // tri-factorisation: [K][L]; null: P = U V^T
  double* part; double* rec;         // as above
  int I, J, K, L;
};
// the site key of the held-out launch pair in a recorded iteration (many.h): behind every site of TriSite, NpSite and the
// position-aligned records (site -1) of the bnmf_vb family
constexpr int kHeldoutSite = 1 << 20;
__host__ __device__ inline int heldout_blocks(int I) { return (I + kHeldoutRowsPerBlock - 1) / kHeldoutRowsPerBlock; }
// launched on st -- or, while a Recorder is installed, recorded (then `rec` is the run's FIRST record: the list-form fold finds the
// iteration's own) -- the main kernel and the fold
void launch_heldout(const HeldoutArgs& a, hipStream_t st);
void launch_heldout_np(const HeldoutNpArgs& a, hipStream_t st);
// the fold behind a main kernel of `nblocks` blocks: rec[0 .. 8) = the column sums of part [nblocks][8] in a fixed order (launched,
// or recorded behind the main kernel's record); kernel_obs_heldout.hip's launcher ends in it too
void launch_fold(const double* part, int nblocks, double* rec, hipStream_t st);
// rval[e] = R[i][col[e]] for the entries e of every row i (R [I][J])
void launch_heldout_values(const float* R, int I, int J, const uint32_t* rowptr, const uint32_t* col, float* rval, hipStream_t st);

// ---------------------------------------------------------------------------
// Observed-entry layout of the two-factor Gibbs / ICM models (kernel_obs.hip): the residual on the observed
// entries, one wave per unit, no contraction and no Gram matrix
// ---------------------------------------------------------------------------
constexpr int kObsWaves = 4;           // units (waves) per block
constexpr int kObsMaxRank = 256;       // K: nothing ties a rank to a lane; the unit's row and prior rates take 2 KiB of LDS per wave
constexpr int kObsMaxSlots = 8;        // register form: entries per lane (instantiations 1, 2, 4, 8); a unit of more than 512 entries runs the long form
struct ObsSweepArgs {
  const uint32_t* ptr;               // [n + 1] the entries of unit u are [ptr[u], ptr[u + 1])
  const uint32_t* idx;               // their inner indices, ascending within a unit
  const float* val;                  // their values of R
  int n, m, K, KP;                   // units, inner extent, rank, row stride of the row-major factors (K rounded up to 4; padding columns zero)
  int mode;                          // kSweepDraw / kSweepMode
  int cond_k;                        // >= 0: evaluate (numer, tau) of this column only and change nothing
  int force_long;                    // every unit down the long form (BNMTF_OBS_LONG=1)
  float min_x;                       // mode updates: lower clamp of the new value (ICM minimum_TN)
  const float* lambda;               // [n][KP]
  float* X; float* XT; int ldT;      // this direction's factor [n][KP] and transposed [K][ldT]
  const float* Xo; const float* XoT; int ldT_o;   // the other factor [m][KP] and [K][ldT_o], ldT_o > m: XoT[k][m] is zero
  float* escratch;                   // [entries] the long form's residual, at the entry's list position
  const float* tau;                  // device scalar
  uint32_t key0, key1, it, stream;
  double* part;                      // null, or [obs_sweep_blocks(n)][4]: SSE, sum P, sum P^2, sum R P of the final residual
  double* numer_out; double* tau_out;   // cond_k >= 0: [n]
  float* snap;                       // null, or the sample slot [n][K]
};
struct ObsFinishArgs {
  const double* part; int nb;        // the V half sweep's partial sums
  double n_obs, sumR, sumR2, alpha, beta;
  int update;                        // 0 draw (tau = gunit / beta_s), 1 mode (alpha_s / beta_s), 2 ICM ((alpha_s - 1) / beta_s)
  const double* gunit;               // update 0: the iteration's Gamma(alpha_s, 1) variate (stage_gamma_variates)
  double* tau_d; float* tau_f;
  double* rec;                       // [5]: tau, MSE, R^2, Rp, SSE
};
struct ObsMetricArgs {
  const uint32_t* row; const uint32_t* col; const float* val; size_t n;   // the entries, any order
  const double* A; const double* B; int K;                                // [I][K], [J][K]
  double* part;                      // [obs_metric_blocks(n)][8]
};
inline int obs_sweep_blocks(int n) { return (n + kObsWaves - 1) / kObsWaves; }
inline int obs_metric_blocks(size_t n) { const size_t b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }
void launch_obs_sweep(const ObsSweepArgs& a, hipStream_t st);
void launch_obs_finish(const ObsFinishArgs& a, hipStream_t st);
void launch_obs_metric(const ObsMetricArgs& a, double* out8, hipStream_t st);   // out8: n, sum R, sum R^2, sum P, sum P^2, sum R P, 0, 0

// Held-out sums of a two-factor handle's own factors, once per iteration (kernel_obs_heldout.hip; bnmtf_set_heldout_entries): the
// six sums of metrics_from_sums over a row-sorted list of entries, fp64 products of the fp32 rows, fixed summation order
constexpr int kObsHeldoutRows = kHeldoutRowsPerBlock;   // a wave per row, heldout_blocks(I) blocks
constexpr int kObsHeldoutStep = 64;                      // entries of a row per wave step: a lane each
struct ObsHeldoutArgs {
  const uint32_t* rowptr;            // [I + 1] the held-out entries of row i are [rowptr[i], rowptr[i + 1])
  const uint32_t* col;               // [n] their columns, ascending within a row
  const float* rval;                 // [n] their values
  const float* A; const float* B;    // rows.X [I][stride] and cols.X [J][stride]
  int I, K, stride;                  // K <= kObsMaxRank; stride = K rounded up to 4
  double* part;                      // [heldout_blocks(I)][8]
  double* rec;                       // [8] the iteration's record: n, sum R, sum R^2, sum P, sum P^2, sum R P, 0, 0
};
void launch_obs_heldout(const ObsHeldoutArgs& a, hipStream_t st);   // the kernel and launch_fold

// Posterior predictive statistics of stored samples over a row-sorted entry list (kernel_predictive.hip; bnmtf_predictive_samples):
// one launch per chunk of samples, the per-entry accumulators read-modify-written in sample order
constexpr int kPredictiveRows = kHeldoutRowsPerBlock;   // a wave per row, heldout_blocks(I) blocks
constexpr int kPredictiveStep = 64;                      // entries of a row per wave step: a lane each
struct PredictiveArgs {
  const uint32_t* rowptr;            // [I + 1] the entries of row i are [rowptr[i], rowptr[i + 1])
  const uint32_t* col;               // [n] their columns
  const float* A;                    // [C][I][K] the chunk's samples of U, or F; unpadded
  const float* S;                    // [C][K][L], or null (L = 0)
  const float* B;                    // [C][J][K] V, or [C][J][L] G
  int I, J, K, L;                    // K, L <= kObsMaxRank
  int C;                             // samples in the chunk
  int first;                         // the chunk begins with the call's first sample: it sets p_first
  double* p_first; double* sum_d; double* sum_d2;   // [n] in list order; the sums zero before the first chunk
};
void launch_predictive(const PredictiveArgs& a, hipStream_t st);

// Log predictive density of known values under stored samples over a row-sorted entry list (kernel_log_predictive.hip;
// bnmtf_log_predictive_samples): predictive_kernel's gather, and per entry and sample the Gaussian
// log-likelihood l_t = fma(-(h_t d), d, c_t), d = r - p_t, into five accumulators: the shifted moments of l and a running-maximum
// log-sum-exp.  One launch per chunk of samples, the accumulators read-modify-written in sample order
struct LogPredictiveArgs {
  const uint32_t* rowptr;            // [I + 1] the entries of row i are [rowptr[i], rowptr[i + 1])
  const uint32_t* col;               // [n] their columns
  const double* val;                 // [n] their values r, in list order
  const float* A;                    // [C][I][K] the chunk's samples of U, or F; unpadded
  const float* S;                    // [C][K][L], or null (L = 0)
  const float* B;                    // [C][J][K] V, or [C][J][L] G
  const double* c; const double* h;  // [C] the chunk's c_t = (log tau_t - log 2 pi) / 2 and h_t = tau_t / 2, from the host
  int I, J, K, L;                    // K, L <= kObsMaxRank
  int C;                             // samples in the chunk
  int first;                         // the chunk begins with the call's first sample: it sets l_first, l_max and sum_exp = 1
  double* l_first; double* sum_d; double* sum_d2;   // [n] in list order; the sums zero before the first chunk
  double* l_max; double* sum_exp;                   // [n]: max_t l_t so far and sum_t exp(l_t - l_max)
};
void launch_log_predictive(const LogPredictiveArgs& a, hipStream_t st);

// Closed-form predictive mean and variance under a mean-field q over a row-sorted entry list (kernel_predictive_q.hip;
// bnmtf_predictive_moments): the factors' means and variances in fp64, one launch (two for the
// tri-factorisation: the column table H = G S^T first)
constexpr int kPredictiveQRows = kHeldoutRowsPerBlock;  // a wave per row, heldout_blocks(I) blocks
constexpr int kPredictiveQStep = 64;                     // entries of a row per wave step: a lane each
constexpr int kPredictiveQStaged = 4;                    // staged arrays per wave: 4 x 256 doubles, 32 KiB per block
struct PredictiveQArgs {
  const uint32_t* rowptr;            // [I + 1] the entries of row i are [rowptr[i], rowptr[i + 1])
  const uint32_t* col;               // [n] their columns
  const double* EA; const double* VA;   // [I][K] mean and variance of U, or F; unpadded.  VA null: a = 0
  const double* ES; const double* VS;   // [K][L], or null (L = 0).  VS null: b = 0
  const double* EB; const double* VB;   // [J][W], W = L ? L : K: V, or G.  VB null: c = 0
  double* H;                         // [J][hstride] (G S^T)_jk, the pad column zero; written by the table pass (L > 0), else null
  int I, J, K, L;                    // K, L <= kObsMaxRank
  int hstride;                       // K rounded up to 2 doubles: a row of H begins on a 16-byte boundary
  double* mean; double* var;         // [n] in list order
};
void launch_predictive_q(const PredictiveQArgs& a, hipStream_t st);   // predictive_q_table_kernel (L > 0), then the entry pass

// The n best columns of every selected row under a total order (kernel_top.hip; bnmtf_top_entries): a wave
// per (row, column segment) pair, its sorted list in LDS, and a merge of a row's segment lists
constexpr int kTopRows = kHeldoutRowsPerBlock;           // waves per block: a (row, segment) pair each
constexpr int kTopStep = 64;                             // columns per wave step: a lane each
constexpr int kTopMaxN = 128;                            // n (BNMTF_TOP_MAX_N): two list slots per lane
constexpr int kTopMaxSplit = 1024;                       // column segments per row
struct TopArgs {
  const double* A;                   // [r][K] the selected rows of the rows factor (U, or F), unpadded
  const double* S;                   // [K][L], or null (L = 0)
  double* FS;                        // [r][L] (F S) of the selected rows (top_fs_kernel writes it), or null
  const double* B;                   // [J][stride] the columns factor (V, or G)
  int r, J, K, L;                    // K, L <= kObsMaxRank
  int stride;                        // W = L ? L : K rounded up to 2 doubles: a row of B begins on a 16-byte boundary
  const uint32_t* exptr;             // [r + 1] the excluded columns of selected row q are [exptr[q], exptr[q + 1])
  const uint32_t* excol;             // ascending and distinct within a row
  int n, largest;                    // 1 <= n <= kTopMaxN; the order: higher score first (largest), or lower first
  int split, seg_steps;              // segments per row and whole kTopStep-column steps per segment
  double* part_key; int32_t* part_col; int32_t* part_cnt;   // [r][split][n], [r][split]: the segments' lists, best first; key = +-score
  int32_t* cols; double* scores; int32_t* counts;           // [r][n], [r]: the answer; -1 / nan behind counts[q] slots
};
void launch_top(const TopArgs& a, hipStream_t st);        // top_fs_kernel (L > 0), top_kernel, top_merge_kernel

// Fold new units into a fitted model (kernel_foldin.hip; bnmtf_fold_in): the other factor fixed, the whole
// chain of a unit in one wave of one launch, the statistics of its factor row kept in fp64 in that wave's LDS
constexpr int kFoldInWaves = 4;            // units (waves) per block
constexpr int kFoldInMaxRank = 256;        // W (BNMTF_FOLDIN_MAX_RANK): a unit's x, rates, a and statistics take 9 KiB of LDS per wave
constexpr int kFoldInMaxSlots = 8;         // register form: entries per lane (1, 2, 4, 8); a unit of more than 512 entries runs the long form
struct FoldInArgs {
  const uint32_t* ptr;               // [n + 1] the entries of unit u are [ptr[u], ptr[u + 1]), at least one each
  const uint32_t* idx;               // their indices into the fixed factor, ascending within a unit, all < m
  const float* val;                  // their values
  int n, m, W, KP;                   // units, rows of the fixed factor, rank, its row stride (W rounded up to 4; padding columns zero)
  const float* Xo; const float* XoT; int ldT;   // the fixed factor [m][KP] and [W][ldT], ldT > m: XoT[k][m] is zero
  const float* lambda; const float* init;       // [n][W]
  const uint32_t* ids;               // [n] the element word of each unit's Philox counter
  float tau, min_x;
  uint32_t key0, key1, it0;          // the seed's halves and the iteration word of the first sweep
  int T, discard, keep_every;        // sweeps; the kept ones are discard, discard + keep_every, ... < T
  int mode;                          // kSweepDraw / kSweepMode
  int force_long;                    // every unit down the long form
  float* escratch;                   // [entries] the long form's residual, at the entry's list position
  double* stats;                     // [3][n][W]: the first kept x, sum (x_t - first), sum (x_t - first)^2 over the kept sweeps
  float* samples;                    // null, or [T][n][W]
};
inline int foldin_blocks(int n) { return (n + kFoldInWaves - 1) / kFoldInWaves; }
void launch_foldin(const FoldInArgs& a, hipStream_t st);

// The variational two-factor model on the same lists (kernel_obs_vb.hip): q = (mu, tau, var) beside the expectation X, and
// S2 = var + X^2 transposed beside XT for the other direction's second gather
struct ObsVbSweepArgs {
  const uint32_t* ptr; const uint32_t* idx; const float* val;     // as ObsSweepArgs
  int n, m, K, KP;
  int only_k;                        // >= 0: update_U(k) / update_V(k) -- mu and tau of this column only
  int moments;                       // only_k >= 0: also the column's expectation and variance (0: they stay)
  int force_long;
  const float* lambda;               // [n][KP]
  float* X; float* XT; float* S2T; int ldT;       // this direction's expectation [n][KP], and with S2 transposed [K][ldT]
  float* mu; float* tauq; float* var;             // [n][KP]
  const float* Xo; const float* XoT; const float* S2oT; int ldT_o;   // the other factor [m][KP], [K][ldT_o] twice; ldT_o > m: word m of every column is zero
  float* escratch;                   // [entries]
  const float* tau;                  // device scalar: exptau
  double* stat;                      // null (the hooks), or the blocks' sums of quad, log erfc, log tau, lambda E [blocks][4] -- with part: and of q2, q3 [blocks][6]
  double* part;                      // null, or [blocks][4]: SSE, sum P, sum P^2, sum R P of the final residual (the V half sweep)
  // launch_obs_trivb_sweep only (the tri-factorisation's F / G half sweeps against an effective factor; all of it unread otherwise):
  const int* order;                  // device: the column order of a whole half sweep (null: 0 .. K - 1)
  const float* cov_S;                // E[S]; element (column c of this factor, inner t) at cov_S[c * cov_sc + t * cov_st]
  const float* cov_mv;               // [n][32] masked variance sums of the other factor over the unit's entries (mvG / mvF)
  int cov_sc, cov_st, cov_n;         // strides and inner extent (L for the F half sweep, K for the G half sweep; <= 32)
};
struct ObsVbFinishArgs {
  const double* stat_r; int nb_r;    // the U half sweep's [nb_r][4]
  const double* stat_c; const double* part; int nb_c;   // the V half sweep's [nb_c][6] and [nb_c][4]
  double n_obs, sumR, sumR2, alpha, beta;
  double* tau_d; float* tau_f;
  double* rec;                       // [14]: exptau, MSE, R^2, Rp, exp_square_diff, beta_s, the four sums of U, the four of V
};
struct ObsVbEsdArgs {
  const uint32_t* ptr; const uint32_t* idx; const float* val; int n;     // the row list
  int K, KP;
  const float* X; const float* var; const float* Xo; const float* varo;  // rows' and columns' expectation and variance [.][KP]
  double* part;                      // [obs_vb_esd_blocks(n)]
};
inline int obs_vb_esd_blocks(int n) { return n < 1 ? 1 : (n > 1024 ? 1024 : n); }
void launch_obs_vb_sweep(const ObsVbSweepArgs& a, hipStream_t st);
void launch_obs_vb_finish(const ObsVbFinishArgs& a, hipStream_t st);
void launch_obs_vb_esd(const ObsVbEsdArgs& a, double* out, hipStream_t st);
// the same sweep with the tri-factorisation's covariance term and column order (kernel_obs_vb.hip: obs_trivb_sweep_kernel, a second
// instantiation of the body; XT / S2T are not written -- nothing gathers F or G themselves)
void launch_obs_trivb_sweep(const ObsVbSweepArgs& a, hipStream_t st);


// ---------------------------------------------------------------------------
// The tri-factorisation on the observed-entry layout (kernel_obs_tri.hip): the effective factors the two
// half sweeps of obs_sweep_kernel run against, and the S system's per-column inputs from the column list; K, L <= 32, every
// row-major factor [.][32]
// ---------------------------------------------------------------------------
constexpr int kObsTriStride = 32;      // row stride of F, G, both effective factors and Pv: what kernel_ssys.hip's launchers read
struct ObsTriEffArgs {      // out = X . S (transposeS = 0: inner K, width L) or X . S^T (transposeS = 1: inner L, width K), row by row
  const float* X; int n;             // [n][32], padding columns zero
  const float* S; int K, L;          // [K][L] unpadded
  int transposeS;
  float* out;                        // [n][32], padding columns zero
  float* outT; int ldT;              // [width][ldT], ldT > n: the words behind column n are never written (they stay zero)
};
struct ObsTriGramArgs {     // per column j of the column list: W_j = sum_{i in Omega_j} F_i F_i^T (packed), Pv_j = sum_{i in Omega_j} R_ij F_i
  const uint32_t* ptr; const uint32_t* idx; const float* val;   // the column list: [n + 1], rows ascending within a column, values
  int n, K;
  const float* F;                    // [I][32]
  float* Wc;                         // [n + 2][tri_padded(K)], tri_pos order (pads and the two extra rows are never written)
  float* Pv;                         // [n][32]: the layout launch_ssys_b reads with split = 1, n_pad = n
};
struct ObsTriGramVbArgs {   // launch_obs_tri_gram_vb: W~_j = W_j + diag(mv_j), mv_jk = sum_{i in Omega_j} varF_ik (the second moments' column Gram)
  const float* varF;                 // [I][32]
  float* mv;                         // [n][32]
};
constexpr int kObsTriGramWaves = 4;    // columns (waves) per block of the column-Gram kernel
constexpr int kObsTriEffRows = 64;     // rows per block of the effective-factor kernel
inline int obs_tri_gram_blocks(int n) { return (n + kObsTriGramWaves - 1) / kObsTriGramWaves; }
inline int obs_tri_eff_blocks(int n) { return (n + kObsTriEffRows - 1) / kObsTriEffRows; }
void launch_obs_tri_eff(const ObsTriEffArgs& a, hipStream_t st);
void launch_obs_tri_gram(const ObsTriGramArgs& a, hipStream_t st);

// The variational tri-factorisation on the same handle (kernel_obs_trivb.hip)
struct ObsTriVbEffArgs {    // the effective factor's mean m = X . S (or X . S^T) and second moment S2e = S2X . S2S - X^2 . S^2 + m^2, S2 = var + E^2
  const float* X; const float* varX; int n;       // [n][32] twice, padding columns zero
  const float* S; const float* varS; int K, L;    // [K][L] unpadded
  int transposeS;
  float* out; float* out2;           // mean and S2e [n][32], padding columns zero
  float* outT; float* out2T; int ldT;   // transposed [width][ldT], ldT > n: the words behind column n are never written (they stay zero)
};
struct ObsMvArgs {          // out[u][c] = sum over the unit's entries e of V[idx[e]][c], in list order per half wave
  const uint32_t* ptr; const uint32_t* idx; int n;
  const float* V;                    // [m][32]
  float* out;                        // [n][32]
};
struct ObsTriVbFinishArgs {
  ObsVbFinishArgs f;                 // as obs_vb_finish_kernel's; rec[4] = SSE + sum (q2 - q3) + third
  const double* third; int n_third;  // launch_tri_third's partial sums
};
struct ObsTriVbEsdArgs {
  const uint32_t* ptr; const uint32_t* idx; const float* val; int n;     // the row list
  int K, L;
  const float* F; const float* varF; const float* G; const float* varG;  // [.][32]
  const float* S; const float* varS;                                    // [K][L]
  double* part;                      // [obs_vb_esd_blocks(n)]
};
constexpr int kObsMvWaves = 4;
inline int obs_mv_blocks(int n) { return (n + kObsMvWaves - 1) / kObsMvWaves; }
void launch_obs_tri_gram_vb(const ObsTriGramArgs& a, const ObsTriGramVbArgs& vb, hipStream_t st);      // obs_tri_gram_kernel's loop, Wc with the variance sums on its diagonal
void launch_obs_trivb_eff(const ObsTriVbEffArgs& a, hipStream_t st);
void launch_obs_mv(const ObsMvArgs& a, hipStream_t st);
void launch_obs_trivb_finish(const ObsTriVbFinishArgs& a, hipStream_t st);
void launch_obs_trivb_esd(const ObsTriVbEsdArgs& a, double* out, hipStream_t st);

// ---------------------------------------------------------------------------
// The non-probabilistic NMF / NMTF on the observed-entry layout (kernel_obs_np.hip): the multiplicative
// updates of kernel_np.hip with P = U V^T (or F S G^T) on the observed entries only, one wave per unit; ranks up to kObsMaxRank
// ---------------------------------------------------------------------------
struct OnpSweepArgs {
  const uint32_t* ptr; const uint32_t* idx; const float* val;     // as ObsSweepArgs
  int n, m, K, KP;                   // units, inner extent, rank, row stride of this factor and of Xo (K rounded up to 4; padding columns zero)
  int k0, k1;                        // the columns [k0, k1) in order: all of them, or one (the single-column form)
  int force_long;                    // every unit down the long form (BNMTF_OBS_LONG=1)
  int resume, keep;                  // P of every entry from escratch instead of phase 1 / into escratch behind the last column
  float* X; float* XT; int ldT;      // this direction's factor [n][KP] and transposed [K][ldT]
  const float* Xo; const float* XoT; int ldT_o;   // the other (or effective) factor [m][KP] and [K][ldT_o], ldT_o > m: XoT[k][m] is zero
  float* escratch;                   // [entries] P at the entry's list position (the long form; resume / keep)
  double* part;                      // null, or [obs_sweep_blocks(n)][8]: n, R, R^2, P, P^2, R P, I-divergence, SSE of the final P
};
struct OnpEffArgs {         // out = X . S (transposeS = 0: inner K, width L) or X . S^T (transposeS = 1: inner L, width K), fp32, inner index in order
  const float* X; int n, ldX;        // [n][ldX]
  const float* S; int K, L, transposeS;
  float* out; int ldo;               // [n][ldo], the padding columns zero
  float* outT; int ldT;              // [width][ldT]
};
struct OnpSPassArgs {       // one pass of NMTF's S step over the row list (NpSPass's scheme)
  const uint32_t* ptr; const uint32_t* idx; const float* val; int I;
  const float* F; int ldF;           // [I][ldF]
  const float* GT; int ldGT;         // [L][ldGT]
  const float* Xo;                   // build: G S^T [J][ldF]
  float* P;                          // [entries] in row-list order
  const float* S_in; float* S_out;   // the step's starting values (read only); every entry as it is finished
  int K, L;
  int prev, cur;                     // entries of S (k L + l) or -1: finish prev and move P by its change; sum cur's numerator and denominator
  int build;                         // P from F and G S^T first (the step's first pass)
  int apply;                         // cur < 0: still move P by prev's change (the single update leaves P current)
  int nb;                            // blocks of every summing pass: the partials of prev
  const double* part_prev; double* part_cur;   // [nb][2]
};
struct OnpMetricArgs {      // the eight sums of metrics_from_np_sums over an entry list; P in fp64 from the fp32 factors
  const uint32_t* row;               // the entries' rows, or null: the entries are a row list and ptr [I + 1] finds the row
  const uint32_t* ptr; int I;
  const uint32_t* col; const float* val; size_t n;
  const float* A; int ldA;           // [I][ldA]
  const float* S; int K, L;          // L > 0: P = (A_i S) . B_j with A_i S in fp64
  const float* B; int ldB;           // [J][ldB]
  double* part;                      // [obs_metric_blocks(n)][8]
};
inline int onp_s_blocks(int I) { const int b = obs_sweep_blocks(I); return b > 1024 ? 1024 : b; }
void launch_onp_sweep(const OnpSweepArgs& a, hipStream_t st);
void launch_onp_fold(const double* part, int nb, double* out8, hipStream_t st);       // thread t the blocks t, t + 256, ..., then a tree
void launch_onp_eff(const OnpEffArgs& a, hipStream_t st);
void launch_onp_s_pass(const OnpSPassArgs& a, hipStream_t st);
void launch_onp_metric(const OnpMetricArgs& a, double* out8, hipStream_t st);

}  // namespace bnmtf
