// tests/simt/emu_fr_bary.cpp -- the evaluation-form opening kernels of bls12_381_amd/csrc/fr_bary.hip.h compiled for the HOST (test
// infrastructure only).  emu_fr_bary builds the forward twiddle table with the transform's own kernels (k_fr_twiddles, k_fr_tw_levels:
// what fr_twiddles_ready launches) and then WALKS THE PLAN of csrc/fr_bary_plan.h -- the function api_fr.hip launches from -- step by
// step, with its grids, blocks, LDS sizes and buffer roles, at whatever (block, chunk) the test asks for: a tile of 64 x 2 elements
// reaches the row-over-tiles shape at 256 elements.
//
// The kernels add across lanes with __shfl_down and meet at the workgroup barrier, so every launch runs its block on one host thread per
// lane (the lane pool of tests/simt/emu_harness.h); there is no one-lane shortcut here.
//
// Built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_bary_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (8 * 8 + 4) + 256 * 8 + 4 * 20)            // frb_lds_bytes of the shipped shape
#include "emu_harness.h"

#include "fr_bary.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frb_lds_bytes(bls::FrBaryShape()), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");

using namespace bls;

namespace {

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
        launch_threads(s.grid, s.block, [=] { k_frb_tile<OPEN>(s.kernel, evals, points, tw, log_n, k, order, chunk, y, q, dst); });
        break;
      case FRB_K_ROW:
        launch_threads(s.grid, s.block, [=] { k_frb_row<OPEN>(src, ((size_t)1 << log_n) / plan.tile, (unsigned)plan.tile, points, log_n, k, y, q, dst); });
        break;
      default:
        launch_threads(s.grid, s.block, [=] { k_frb_quot(evals, src, log_n, k, chunk, q); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}

}  // namespace

extern "C" {

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
    launch_threads((unsigned)(((half + FR_TW_RUN - 1) / FR_TW_RUN + 255) / 256), 256, [=] { k_fr_twiddles(tw, log_n, 0); });
    if (log_n > 1) launch_threads((unsigned)((half + 255) / 256), 256, [=] { k_fr_tw_levels(tw, log_n); });
  }
  u32* buf[2] = {rec, rowrec};
  if (open) return run_bary<true>(plan, evals, log_n, k, points, order, y, q, (unsigned)chunk, tw, buf, kernels_out);
  return run_bary<false>(plan, evals, log_n, k, points, order, y, q, (unsigned)chunk, tw, buf, kernels_out);
}
}
