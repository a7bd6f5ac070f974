// Many models in one launch (round 6): the model-selection jobs of the reference (a cross-validation's folds x ranks: dozens of
// models of GDSC's size, 622 x 138) run a model per process slot, and a kernel of ONE such model occupies 18-78 blocks of a
// 256-CU chip.  Every kernel of the multi-launch path that a variational iteration uses has a LIST form: blockIdx.z = model, the
// arguments of model z read from a device array through the scalar cache (constant address space: as uniform as kernel
// arguments, no vector registers).  Host side: the launchers, called while a Recorder is installed (thread-local), append
// (list-form kernel, grid, block, LDS, argument bytes) instead of launching; api_many.inc runs the models' host code in lock-step
// and turns the records of a launch site into one launch.
//
// A kernel with both forms is written ONCE, as a struct K (below: one_form, list_form, launch_forms):
//   K::Args      the arguments, whole dwords.  Whoever fills one zeroes its padding first (memset): a recorded list compares bytes.
//                What moves from one iteration to the next (an order, a record) is in Args as the run's FIRST and a step; the body
//                applies `it`.
//   K::kThreads  the launch bounds of both forms.
//   K::blocks    static __host__ __device__ int blocks(const Args&): the model's own block count.  The single launch's grid, the
//                recorded grid and the list form's exit all come from this one function: a model run among others keeps the bits
//                of its own run only while the three agree.
//   K::body      template <int FORM> static __device__ void body(const Args&, int nb, int it): block blockIdx.x of nb.  FORM = 0 in
//                the single form (nb = gridDim.x, it = 0), 1 in the list form -- each form its own instantiation: a body shared by
//                two kernels is inlined differently into each, and the single-model kernel keeps the code it had.
// Written by hand instead, with a shared body and their own pair of wrappers: gemm_bf16x3 (kernel_gemm.hip), sweep_vb
// (kernel_sweep_vb.hip), post and gram_reduce (kernel_post.hip).  They are the benchmark's hot path: their register budgets and
// launch lines are pinned by name (tests/test_kernel_resources_cpu.py, tests/test_tail_resources_cpu.py), and post and gram_reduce
// record from one launcher with a two-dimensional grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace bnmtf {

template <class P>
__device__ __forceinline__ P load_pack(const P* list, int idx) {
  static_assert(sizeof(P) % 4 == 0, "argument packs are whole dwords");
  typedef __attribute__((address_space(4))) const uint32_t cu32;
  cu32* src = (cu32*)(uintptr_t)(list + idx);
  P out;
  uint32_t* dst = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(P) / 4); ++i) dst[i] = src[i];
  return out;
}

struct LaunchRec {
  const void* fn = nullptr;            // the list form: (const Pack* list, int it)
  dim3 grid, block;
  size_t lds = 0;
  bool flex = false;                   // grid.x may differ between the models of one launch (the list form leaves with blockIdx.x >= its own count)
  uint32_t off = 0, size = 0;          // the argument pack's bytes in the recorder's arena
};
struct Recorder {                      // (cleared per iteration: the vectors keep their capacity, a record costs a memcpy)
  std::vector<LaunchRec> recs;
  // keys[q]: the site key (site, index within the site) of recs[q].  The records of the models of a batch meet in a launch by key,
  // not by position, and the sites are launched in key order; a family that names no site gets (-1, position).
  std::vector<std::pair<int, int>> keys;
  int site = -1, sub = 0;
  std::vector<unsigned char> arena;
  const char* missing = nullptr;       // a launcher without a list form was called while recording (record_missing): its kernel
  void clear() { recs.clear(); keys.clear(); arena.clear(); missing = nullptr; site = -1; sub = 0; }
  const unsigned char* args(const LaunchRec& r) const { return arena.data() + r.off; }
};
extern thread_local Recorder* g_recorder;

// While a Recorder is installed: the records from here on belong to `site`, as (site, first), (site, first + 1), ...
inline void site_at(int site, int first = 0) {
  if (Recorder* rc = g_recorder) { rc->site = site; rc->sub = first; }
}

template <class P>
inline bool record_launch(const void* many_fn, dim3 grid, dim3 block, size_t lds, const P& p, bool flex = false) {
  Recorder* rc = g_recorder;
  if (!rc) return false;
  LaunchRec r;
  r.fn = many_fn; r.grid = grid; r.block = block; r.lds = lds; r.flex = flex;
  r.off = (uint32_t)rc->arena.size(); r.size = (uint32_t)sizeof(P);
  rc->arena.resize(rc->arena.size() + sizeof(P));
  memcpy(rc->arena.data() + r.off, &p, sizeof(P));
  rc->recs.push_back(r);
  rc->keys.push_back({rc->site, rc->sub++});
  return true;
}

// The two forms of a kernel K (the contract: this file's head).
template <class K>
__global__ __launch_bounds__(K::kThreads) void one_form(typename K::Args a) { K::template body<0>(a, (int)gridDim.x, 0); }
// blockIdx.z = model; grid.x is the largest block count of the launch, a model's surplus blocks leave
template <class K>
__global__ __launch_bounds__(K::kThreads) void list_form(const typename K::Args* list, int it) {
  const typename K::Args a = load_pack(list, blockIdx.z);
  const int nb = K::blocks(a);
  if ((int)blockIdx.x >= nb) return;
  K::template body<1>(a, nb, it);
}
// Records the list form while a Recorder is installed, launches the single form otherwise; either over K::blocks(a) (x grid_y:
// a second grid dimension is every model's own).  Every list form leaves by its own count, so grid.x may differ between the
// models of a launch (flex).
template <class K>
inline void launch_forms(const typename K::Args& a, hipStream_t st, dim3 block = dim3(K::kThreads), size_t lds = 0, unsigned grid_y = 1) {
  const dim3 grid((unsigned)K::blocks(a), grid_y);
  if (record_launch((const void*)list_form<K>, grid, block, lds, a, true)) return;
  one_form<K><<<grid, block, lds, st>>>(a);
}

// A launcher that has no list form, called while a Recorder is installed: it launches nothing and says so here -- the caller
// turns the iteration into an error (a kernel launched on the side, out of the batch's order, or left out, would be wrong bits).
inline bool record_missing(const char* what) {
  Recorder* rc = g_recorder;
  if (!rc) return false;
  if (!rc->missing) rc->missing = what;
  return true;
}

}  // namespace bnmtf
