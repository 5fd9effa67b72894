// tests/simt/emu_fr.cpp -- the Fr transform kernels of bls12_381_amd/csrc/fr.hip.h compiled for the HOST (test infrastructure only).
// emu_fr_ntt_many builds the tables with the device kernels (k_fr_twiddles, k_fr_tw_levels, k_fr_ninv, k_fr_coset_table) and then WALKS
// THE PLAN of csrc/fr_plan.h -- the function api_fr.hip::blsgpu_fr_ntt_many_device launches from -- step by step, so the CPU suite
// runs the launch sequence the GPU runs, with its grids, blocks and arguments (tests/test_simt_fr.py).
//
// The transform kernels stride their loops by blockDim.x and use no cross-lane operation but the workgroup barrier, so they compute
// the same at any block size: `threads` == 0 runs the LDS kernels with ONE lane per workgroup in this thread (cheap: the breadth of
// the cases), `threads` != 0 runs them with the plan's block size on one host thread per lane, which is what exercises the barriers.
//
// The lane pool, the launchers, the trapping checks and emu_guarded() are those of tests/simt/emu_harness.h; the tests call this
// library from a child process (tests/simt_fr_child.py).
#define EMU_LANES 512
#define EMU_DYN_LDS_WORDS (9 * 4096)               // the largest column tile (FR_COLS_LOG)
#include "emu_harness.h"

#include "fr.hip.h"

using namespace bls;

namespace {

// a kernel that keeps a tile in LDS between barriers: its real block on lane threads, or one lane per workgroup
template <class Fn> void launch_lds(bool threads, unsigned grid, unsigned block, Fn fn) {
  if (threads) launch_threads(grid, block, fn);
  else launch_loop(grid, 1, fn);
}

}  // namespace

extern "C" {

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
  // api_fr.hip fr_twiddles_ready / fr_ninv_ready / the coset table of blsgpu_fr_ntt_many_device
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
