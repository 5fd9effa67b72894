// tests/simt/emu_fr.cpp -- the Fr transform kernels of bls12_381_amd/csrc/fr.hip.h compiled for the HOST (test infrastructure only).
// emu_fr_ntt_many builds the tables with the device kernels (k_fr_twiddles, k_fr_tw_levels, k_fr_ninv, k_fr_coset_table) and then WALKS
// THE PLAN of csrc/fr_plan.h -- the function api_aux.hip::blsgpu_fr_ntt_many_device launches from -- step by step, so the CPU suite
// runs the launch sequence the GPU runs, with its grids, blocks and arguments (tests/test_simt_fr.py).
//
// The transform kernels stride their loops by blockDim.x and use no cross-lane operation but the workgroup barrier, so they compute
// the same at any block size: `threads` == 0 runs the LDS kernels with ONE lane per workgroup in this thread (cheap: the breadth of
// the cases), `threads` != 0 runs them with the plan's block size on one host thread per lane, which is what exercises the barriers.
//
// Built with -fsanitize=bounds,shift -fsanitize-trap=all, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_child.py), as for tests/simt/emu_msm.cpp.
#define EMU_LANES 512
#define EMU_DYN_LDS_WORDS (9 * 4096)               // the largest column tile (FR_COLS_LOG)
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <functional>
#include <thread>
#include <vector>

thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
EmuState g_emu;

static inline unsigned long long __brevll(unsigned long long x) { return __builtin_bitreverse64(x); }
static inline int __clzll(unsigned long long x) { return __builtin_clzll(x); }

#include "fr.hip.h"

using namespace bls;

namespace {

// the lane pool of tests/simt/emu_msm.cpp: EMU_LANES lane threads started once, a workgroup is one job for the lanes below its block size
struct LanePool {
  std::vector<std::thread> th;
  EmuMeet<1> start, done;
  std::function<void()> job;
  unsigned block = 0, grid = 0, blk = 0;
  LanePool() {
    for (unsigned l = 0; l < EMU_LANES; l++)
      th.emplace_back([this, l] {
        for (;;) {
          start.barrier(EMU_LANES + 1);
          if (l < block) {
            threadIdx.x = l; blockDim.x = block; blockIdx.x = blk; gridDim.x = grid;
            job();
          }
          done.barrier(EMU_LANES + 1);
        }
      });
  }
  void workgroup(unsigned g, unsigned b, unsigned i, const std::function<void()>& fn) {
    job = fn; grid = g; block = b; blk = i;
    start.barrier(EMU_LANES + 1);
    done.barrier(EMU_LANES + 1);
  }
};
LanePool* pool() { static LanePool* p = new LanePool(); return p; }

unsigned nblk(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }
template <class Fn> void launch_threads(unsigned grid, unsigned block, Fn fn) {
  for (unsigned i = 0; i < grid; i++) pool()->workgroup(grid, block, i, fn);
}
template <class Fn> void launch_loop(unsigned grid, unsigned block, Fn fn) {
  blockDim.x = block; gridDim.x = grid;
  for (unsigned i = 0; i < grid; i++)
    for (unsigned l = 0; l < block; l++) { blockIdx.x = i; threadIdx.x = l; fn(); }
}
// a kernel that keeps a tile in LDS between barriers: its real block on lane threads, or one lane per workgroup
template <class Fn> void launch_lds(bool threads, unsigned grid, unsigned block, Fn fn) {
  if (threads) launch_threads(grid, block, fn);
  else launch_loop(grid, 1, fn);
}

}  // namespace

extern "C" {

// as tests/simt/emu_msm.cpp: `bytes` bytes whose end is the start of an inaccessible page; never freed
void* emu_guarded(size_t bytes) {
  const size_t page = (size_t)sysconf(_SC_PAGESIZE);
  const size_t body = (bytes + page - 1) / page * page;
  const size_t guard = (size_t)1 << 20;
  char* m = (char*)mmap(nullptr, body + guard, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == (char*)MAP_FAILED) return nullptr;
  if (mprotect(m + body, guard, PROT_NONE) != 0) return nullptr;
  return m + body - bytes;
}

// data: k 2^log_n scalars (8 u32 each), transformed in place.  tmp: as many (used when the plan says so, may be NULL otherwise);
// tw: 2^log_n - 1 scalars; cs: 2^log_n scalars (coset != NULL); ninv: one scalar.  coset: 8 u32 Montgomery words or NULL.
// cols: 0 = stage passes, 1 = the column-tile plan with the shape (tlog, dmax, block).  kernels_out: the FrKernel of every step, -1 ends it
// (at least 33 ints).  Returns the number of steps, or -1 for arguments the plan does not take.
int emu_fr_ntt_many(u32* data, u32* tmp, u32* tw, u32* cs, u32* ninv, int log_n, size_t k, int inverse, const u32* coset, int cols, int tlog, int dmax, int block,
                    int threads, int* kernels_out) {
  if (log_n < 0 || log_n > 28 || k > (((size_t)1 << 28) >> log_n) || (cols && (block > EMU_LANES || tlog > FR_COLS_LOG))) return -1;
  if (!fr_plan_many(log_n, k, inverse != 0, coset != nullptr, cols != 0).n_steps) { kernels_out[0] = -1; return 0; }      // no launch, no table
  const int dir = inverse ? 1 : 0;
  const size_t n = (size_t)1 << log_n, half = n >> 1;
  // api_aux.hip fr_twiddles_ready / fr_ninv_ready / the coset table of blsgpu_fr_ntt_many_device
  launch_loop(nblk((half + FR_TW_RUN - 1) / FR_TW_RUN, 256), 256, [=] { k_fr_twiddles(tw, log_n, dir); });
  if (log_n > 1) launch_loop(nblk(half, 256), 256, [=] { k_fr_tw_levels(tw, log_n); });
  if (coset) {
    FrArg g;
    for (int i = 0; i < 8; i++) g.w[i] = coset[i];
    launch_loop(nblk((n + FR_TW_RUN - 1) / FR_TW_RUN, 256), 256, [=] { k_fr_coset_table(cs, g, log_n, dir); });
  }
  const u32* scale = nullptr;
  if (inverse && !coset) { launch_loop(1, 64, [=] { k_fr_ninv(ninv, log_n); }); scale = ninv; }
  FrColsShape shape;
  if (cols) { shape.tlog = tlog; shape.dmax = dmax; shape.block = block; }
  const FrPlan plan = fr_plan_many(log_n, k, inverse != 0, coset != nullptr, cols != 0, shape);
  if (plan.needs_tmp && !tmp) return -1;
  u32* buf[2] = {data, tmp};
  const size_t total = plan.total;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrStep s = plan.step[i];
    const u32* src = buf[s.src];
    u32* dst = buf[s.dst];
    const u32* cin = s.coset_in ? cs : nullptr;
    const u32* cout = s.coset_out ? cs : nullptr;
    kernels_out[i] = s.kernel;
    if ((size_t)s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    switch (s.kernel) {
      case FR_K_COLS:
        if (s.coset_in) launch_lds(threads != 0, s.grid, s.block, [=] { k_fr_cols<true>(src, dst, tw, s.lh, s.d, s.lk, cin, log_n); });
        else launch_lds(threads != 0, s.grid, s.block, [=] { k_fr_cols<false>(src, dst, tw, s.lh, s.d, s.lk, nullptr, log_n); });
        break;
      case FR_K_STAGE2:
        if (s.coset_in) launch_loop(s.grid, s.block, [=] { k_fr_stage2<true>(src, dst, tw, log_n, s.lh, total / 4, cin); });
        else launch_loop(s.grid, s.block, [=] { k_fr_stage2<false>(src, dst, tw, log_n, s.lh, total / 4, nullptr); });
        break;
      case FR_K_STAGE1:
        if (s.coset_in) launch_loop(s.grid, s.block, [=] { k_fr_stage1<true>(src, dst, tw, log_n, s.lh, total / 2, cin); });
        else launch_loop(s.grid, s.block, [=] { k_fr_stage1<false>(src, dst, tw, log_n, s.lh, total / 2, nullptr); });
        break;
      default:
        launch_lds(threads != 0, s.grid, s.block, [=] { k_fr_tile<true>(src, dst, tw, log_n, s.d, scale, total, cin, cout); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}

// the single transform's own tile kernel (k_fr_tile<false>, one vector of 2^log_n <= 2^FR_TILE_LOG scalars, x -> y): what
// blsgpu_fr_ntt_device launches at log_n <= 10, kept under the emulation so that the batched kernel's twin stays checked
int emu_fr_tile_single(const u32* x, u32* y, u32* tw, u32* ninv, int log_n, int inverse, int threads) {
  if (log_n < 1 || log_n > FR_TILE_LOG) return -1;
  const int dir = inverse ? 1 : 0;
  const size_t n = (size_t)1 << log_n, half = n >> 1;
  launch_loop(nblk((half + FR_TW_RUN - 1) / FR_TW_RUN, 256), 256, [=] { k_fr_twiddles(tw, log_n, dir); });
  if (log_n > 1) launch_loop(nblk(half, 256), 256, [=] { k_fr_tw_levels(tw, log_n); });
  const u32* scale = nullptr;
  if (inverse) { launch_loop(1, 64, [=] { k_fr_ninv(ninv, log_n); }); scale = ninv; }
  launch_lds(threads != 0, 1, 256, [=] { k_fr_tile<false>(x, y, tw, log_n, log_n, scale, n, nullptr, nullptr); });
  return 1;
}
}
