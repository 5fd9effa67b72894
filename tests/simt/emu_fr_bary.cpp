// tests/simt/emu_fr_bary.cpp -- the evaluation-form opening kernels of bls12_381_amd/csrc/fr_bary.hip.h compiled for the HOST (test
// infrastructure only).  emu_fr_bary builds the forward twiddle table with the transform's own kernels (k_fr_twiddles, k_fr_tw_levels:
// what fr_twiddles_ready launches) and then WALKS THE PLAN of csrc/fr_bary_plan.h -- the function api_aux.hip launches from -- step by
// step, with its grids, blocks, LDS sizes and buffer roles, at whatever (block, chunk) the test asks for: a tile of 64 x 2 elements
// reaches the row-over-tiles shape at 256 elements.
//
// The kernels add across lanes with __shfl_down and meet at the workgroup barrier, so every launch runs its block on one host thread per
// lane (the lane pool of tests/simt/emu_fr_scan.cpp); there is no one-lane shortcut here.
//
// Built with -fsanitize=bounds,shift -fsanitize-trap=all, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_bary_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (8 * 8 + 4) + 256 * 8 + 4 * 20)            // frb_lds_bytes of the shipped shape
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <functional>
#include <thread>
#include <vector>

thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
EmuState g_emu;

static inline unsigned long long __brevll(unsigned long long x) { return __builtin_bitreverse64(x); }
static inline int __clzll(unsigned long long x) { return __builtin_clzll(x); }

#include "fr_bary.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frb_lds_bytes(bls::FrBaryShape()), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");

using namespace bls;

namespace {

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
template <class Fn> void launch(unsigned grid, unsigned block, Fn fn) {
  for (unsigned i = 0; i < grid; i++) pool()->workgroup(grid, block, i, fn);
}

template <bool OPEN>
int run_bary(const FrBaryPlan& plan, const u32* evals, int log_n, size_t k, const u32* points, int order, u32* y, u32* q, unsigned chunk, const u32* tw, u32* const* buf,
             int* kernels_out) {
  for (int i = 0; i < plan.n_steps; i++) {
    const FrBaryStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    kernels_out[i] = s.kernel;
    switch (s.kernel) {
      case FRB_K_ROWS: case FRB_K_TILE:
        launch(s.grid, s.block, [=] { k_frb_tile<OPEN>(s.kernel, evals, points, tw, log_n, k, order, chunk, y, q, dst); });
        break;
      case FRB_K_ROW:
        launch(s.grid, s.block, [=] { k_frb_row<OPEN>(src, ((size_t)1 << log_n) / plan.tile, (unsigned)plan.tile, points, log_n, k, y, q, dst); });
        break;
      default:
        launch(s.grid, s.block, [=] { k_frb_quot(evals, src, log_n, k, chunk, q); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
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

// the records each scratch buffer of the plan must hold (FrBaryBuf order: rec, rowrec); returns the number of steps, -1 for a refusal
int emu_fr_bary_recs(int log_n, size_t k, int open, int block, int chunk, size_t* recs) {
  FrBaryShape sh; sh.block = block; sh.chunk = chunk;
  const FrBaryPlan plan = fr_bary_plan(log_n, k, open != 0, sh);
  for (int i = 0; i < 2; i++) recs[i] = plan.recs[i];
  return plan.n_steps;
}
// evals: k * 2^log_n scalars (8 u32 each); points, y: k scalars; q: as evals (open) or NULL; tw: 2^log_n scalars, what the entry point
// reserves for the forward twiddle table (NULL at log_n = 0); rec / rowrec: recs[0] records of FRB_REC_WORDS / recs[1] of
// FRB_ROWREC_WORDS u32.  kernels_out: the FrBaryKernel of every step, -1 ends it (at least 4 ints).  Returns the number of steps.
int emu_fr_bary(int open, const u32* evals, int log_n, size_t k, const u32* points, int order, u32* y, u32* q, int block, int chunk, u32* tw, u32* rec, u32* rowrec,
                int* kernels_out) {
  if (block > EMU_LANES || order < 0 || order > 1) return -1;
  FrBaryShape sh; sh.block = block; sh.chunk = chunk;
  const FrBaryPlan plan = fr_bary_plan(log_n, k, open != 0, sh);
  if (plan.n_steps < 0) return -1;
  if (plan.n_steps && log_n > 0) {                      // fr_twiddles_ready(c, log_n, 0)
    const size_t half = ((size_t)1 << log_n) >> 1;
    launch((unsigned)(((half + FR_TW_RUN - 1) / FR_TW_RUN + 255) / 256), 256, [=] { k_fr_twiddles(tw, log_n, 0); });
    if (log_n > 1) launch((unsigned)((half + 255) / 256), 256, [=] { k_fr_tw_levels(tw, log_n); });
  }
  u32* buf[2] = {rec, rowrec};
  if (open) return run_bary<true>(plan, evals, log_n, k, points, order, y, q, (unsigned)chunk, tw, buf, kernels_out);
  return run_bary<false>(plan, evals, log_n, k, points, order, y, q, (unsigned)chunk, tw, buf, kernels_out);
}
}
