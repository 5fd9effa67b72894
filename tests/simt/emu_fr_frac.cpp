// tests/simt/emu_fr_frac.cpp -- the fused front of the Fr fraction scans (bls12_381_amd/csrc/fr_frac.hip.h) and the scan kernels behind
// it compiled for the HOST (test infrastructure only).  emu_fr_frac WALKS THE PLAN of csrc/fr_frac_plan.h -- the function api_fr.hip
// launches from -- step by step, with its grids, blocks, LDS sizes and buffer roles, at whatever (block, chunk) the test asks for: a tile
// of 64 x 2 elements reaches the multi-tile path at 129 elements and the second aggregate level at 128 * 128 + 1.
//
// Over tests/simt/emu_harness.h, as tests/simt/emu_fr_scan.cpp: every launch runs its block on one host thread per lane, the library
// is built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_frac_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (4 * 8 + 4) + 4 * 20)            // frs_lds_bytes of the largest shipped shape
#include "emu_harness.h"

#include "fr_frac.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frs_lds_bytes(bls::FrScanShape{bls::FRS_BLOCK, bls::FRF_CHUNK_MAX}), "EMU_DYN_LDS_WORDS is smaller than the shipped shapes' LDS");

using namespace bls;

namespace {

struct Args { const u32 *xa, *xb, *da, *db, *chal; size_t pitch, len, k; int c, exclusive; u32* out; uint8_t* flags; };

template <int OP>
int run(const FrFracPlan& plan, const Args& a, u32* const* buf, int* kernels_out) {
  constexpr int SOP = frf_scan_op(OP);
  const unsigned chunk = (unsigned)plan.shape.chunk;
  for (int i = 0; i < plan.n_steps; i++) {
    const FrScanStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    u32* carry = s.carry >= 0 ? buf[s.carry] : nullptr;
    kernels_out[i] = s.kernel;
    switch (s.kernel) {
      case FRF_K_FRONT:
        launch_threads(s.grid, s.block, [=] { k_frf_front<OP>(s.src, a.exclusive, a.c, a.xa, a.xb, a.da, a.db, a.pitch, a.chal, a.len, a.k, chunk, a.out, a.flags, dst, buf[FRS_BUF_LANE]); });
        break;
      case FRS_K_SCAN:
        launch_threads(s.grid, s.block, [=] { k_frs_tile<SOP>(s.kernel, a.exclusive, a.out, a.out, nullptr, a.len, a.k, chunk, dst, carry, buf[FRS_BUF_LANE]); });
        break;
      default:
        launch_threads(s.grid, s.block, [=] { k_frs_agg<SOP>(s.kernel, src, s.items, chunk, s.kernel == FRS_K_AGG_REDUCE ? dst : nullptr, carry, s.kernel == FRS_K_AGG_SCAN ? dst : nullptr); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}

FrFracPlan plan_of(int op, int c, size_t len, size_t k, size_t pitch, int block, int chunk) {
  if (block == 0) return fr_frac_plan(op, c, len, k, pitch);
  if (block > EMU_LANES) { FrFracPlan p; p.n_steps = -1; return p; }
  return fr_frac_plan(op, c, len, k, pitch, FrScanShape{block, chunk});
}

}  // namespace

extern "C" {

// the plan of a call (block == 0: the shipped shape of (op, c)).  info: recs[5] (FrScanBuf order), then block, chunk, lds of step 0,
// table_reach; kinds / grids: one entry per step.  Returns the number of steps, -1 for a refusal.
int emu_fr_frac_plan(int op, int c, size_t len, size_t k, size_t pitch, int block, int chunk, size_t* info, int* kinds, unsigned* grids) {
  const FrFracPlan plan = plan_of(op, c, len, k, pitch, block, chunk);
  for (int i = 0; i < 5; i++) info[i] = plan.recs[i];
  info[5] = (size_t)plan.shape.block; info[6] = (size_t)plan.shape.chunk; info[7] = plan.n_steps > 0 ? plan.step[0].lds : 0; info[8] = plan.table_reach;
  for (int i = 0; i < plan.n_steps; i++) { kinds[i] = plan.step[i].kernel == FRF_K_FRONT ? 100 + plan.step[i].src : plan.step[i].kernel; grids[i] = plan.step[i].grid; }
  return plan.n_steps;
}
// xa / xb / da / db: column sets of table_reach scalars (8 u32 each) or NULL; chal: beta, gamma; out: k * len scalars; flags: k * len bytes
// or NULL; agg0 / agg1 / lane: recs[0] / recs[1] / recs[4] records of 12 u32; carry0 / carry1: recs[2] / recs[3] scalars.  kernels_out:
// the kind of every step, -1 ends it (at least 6 ints).  Returns the number of steps, or -1 for what the plan refuses.
int emu_fr_frac(int op, int exclusive, int c, const u32* xa, const u32* xb, const u32* da, const u32* db, size_t pitch, const u32* chal, size_t len, size_t k,
                u32* out, uint8_t* flags, int block, int chunk, u32* agg0, u32* agg1, u32* carry0, u32* carry1, u32* lane, int* kernels_out) {
  const FrFracPlan plan = plan_of(op, c, len, k, pitch, block, chunk);
  if (plan.n_steps < 0) return -1;
  u32* buf[5] = {agg0, agg1, carry0, carry1, lane};
  const Args a{xa, xb, da, db, chal, pitch, len, k, c, exclusive, out, flags};
  if (op == FRF_GRAND_PRODUCT) return run<FRF_GRAND_PRODUCT>(plan, a, buf, kernels_out);
  return run<FRF_FRAC_SUM>(plan, a, buf, kernels_out);
}
}
