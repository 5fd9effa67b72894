// tests/simt/emu_fr_scan.cpp -- the Fr scan / batch inversion kernels of bls12_381_amd/csrc/fr_scan.hip.h compiled for the HOST (test
// infrastructure only).  emu_fr_scan and emu_fr_invert WALK THE PLAN of csrc/fr_scan_plan.h -- the function api_fr.hip launches from --
// step by step, with its grids, blocks, LDS sizes and buffer roles, at whatever (block, chunk) the test asks for: a tile of 64 x 2
// elements reaches the multi-tile path at 129 elements and the second aggregate level at 128 * 128 + 1.
//
// The kernels scan across lanes with __shfl_up / __shfl_down and meet at the workgroup barrier, so every launch runs its block on one host
// thread per lane (the lane pool of tests/simt/emu_harness.h); there is no one-lane shortcut here.
//
// Built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_scan_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (8 * 8 + 4) + 4 * 20)            // frs_lds_bytes of the shipped shape
#include "emu_harness.h"

#include "fr_scan.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frs_lds_bytes(bls::FrScanShape()), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");

using namespace bls;

namespace {

template <int OP>
int run_scan(const FrScanPlan& plan, int exclusive, const u32* in, u32* out, const u32* points, size_t len, size_t k, unsigned chunk, u32* const* buf, int* kernels_out) {
  for (int i = 0; i < plan.n_steps; i++) {
    const FrScanStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    u32* carry = s.carry >= 0 ? buf[s.carry] : nullptr;
    kernels_out[i] = s.kernel;
    switch (s.kernel) {
      case FRS_K_SINGLE: case FRS_K_REDUCE: case FRS_K_SCAN:
        launch_threads(s.grid, s.block, [=] { k_frs_tile<OP>(s.kernel, exclusive, in, out, points, len, k, chunk, dst, carry, buf[FRS_BUF_LANE]); });
        break;
      default:
        launch_threads(s.grid, s.block, [=] { k_frs_agg<OP>(s.kernel, src, s.items, chunk, s.kernel == FRS_K_AGG_REDUCE ? dst : nullptr, carry, s.kernel == FRS_K_AGG_SCAN ? dst : nullptr); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}

}  // namespace

extern "C" {

// the records each scratch buffer of the plan must hold (FrScanBuf order: agg0, agg1, carry0, carry1, lane); returns the number of steps
int emu_fr_scan_recs(size_t len, size_t k, int block, int chunk, size_t* recs) {
  if (!shape_ok(block, chunk)) return -1;
  FrScanShape sh; sh.block = block; sh.chunk = chunk;
  const FrScanPlan plan = fr_scan_plan(len, k, sh);
  for (int i = 0; i < 5; i++) recs[i] = plan.recs[i];
  return plan.n_steps;
}
// in / out: k * len scalars (8 u32 each; may be the same buffer); points: k scalars (HORNER) or NULL; agg0 / agg1 / lane: recs[0] / recs[1] /
// recs[4] records of frs_rec_words(op) u32; carry0 / carry1: recs[2] / recs[3] scalars.  kernels_out: the FrScanKernel of every step, -1 ends it
// (at least 6 ints).  Returns the number of steps, or -1 for a shape the plan does not take.
int emu_fr_scan(int op, int exclusive, const u32* in, u32* out, const u32* points, size_t len, size_t k, int block, int chunk, u32* agg0, u32* agg1, u32* carry0, u32* carry1,
                u32* lane, int* kernels_out) {
  if (!shape_ok(block, chunk) || op < 0 || op > 2 || (op == FRS_HORNER && exclusive)) return -1;
  FrScanShape sh; sh.block = block; sh.chunk = chunk;
  const FrScanPlan plan = fr_scan_plan(len, k, sh);
  if (plan.n_steps < 0) return -1;
  u32* buf[5] = {agg0, agg1, carry0, carry1, lane};
  if (op == FRS_SUM) return run_scan<FRS_SUM>(plan, exclusive, in, out, points, len, k, (unsigned)chunk, buf, kernels_out);
  if (op == FRS_PRODUCT) return run_scan<FRS_PRODUCT>(plan, exclusive, in, out, points, len, k, (unsigned)chunk, buf, kernels_out);
  return run_scan<FRS_HORNER>(plan, 0, in, out, points, len, k, (unsigned)chunk, buf, kernels_out);
}
// in / out: n scalars (may be the same buffer); flags: n bytes or NULL
int emu_fr_invert(const u32* in, u32* out, uint8_t* flags, size_t n, int block, int chunk, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  FrScanShape sh; sh.block = block; sh.chunk = chunk;
  const FrScanPlan plan = fr_invert_plan(n, sh);
  if (plan.n_steps < 0) return -1;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrScanStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    kernels_out[i] = s.kernel;
    launch_threads(s.grid, s.block, [=] { k_frs_invert(in, out, flags, n, (unsigned)chunk); });
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}
}
