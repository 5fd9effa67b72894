// tests/simt/emu_fr_lagrange.cpp -- the Lagrange-coefficient kernel of bls12_381_amd/csrc/fr_lagrange.hip.h compiled for the HOST (test
// infrastructure only).  emu_flg WALKS THE PLAN of csrc/fr_lagrange_plan.h -- the function api_fr.hip launches from -- with its grid,
// block, team, tile and LDS size, at whatever shape the test asks for: 4 lanes with a tile of 4 nodes and 2 nodes per lane and pass make
// a pass of 8 nodes, so a few dozen nodes reach every path (several passes, several tiles, a repeat across tiles, the trees); 8 lanes in
// two teams of 4 are the WAVE shape with two segments per workgroup.  block == 0 takes the shipped shape, `which` choosing between the
// plan's pick, BLOCK and WAVE.
//
// Over tests/simt/emu_harness.h: every launch runs its block on one host thread per lane, the library is built with the trapping
// bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page (a segment that breaks the offsets contract
// and WAS used as an address ends the process), and the tests call this library from a child process
// (tests/simt_fr_lagrange_child.py).  -DFLG_FAULT=n builds the kernel with one of its seeded faults (tests/test_simt_fr_lagrange.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (512 * 8 + 2 * 256 * 8 + 2 * 256)           // the BLOCK shape: a tile of 512 nodes, the two trees of 256 lanes
#include "emu_harness.h"

#include "fr_lagrange.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= (FLG_BLOCK / 8) * bls::flg_team_lds_words(8, 8) * 4 &&
              sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::flg_team_lds_words(FLG_BLOCK, FLG_TILE) * 4, "EMU_DYN_LDS_WORDS is smaller than the shipped shapes' LDS");

using namespace bls;

namespace {

FlgPlan plan_of(size_t nseg, size_t total, bool want_lambda, int which, int block, int team, int tile, int r) {
  if (block == 0) return flg_plan(nseg, total, want_lambda, which);
  if (block > EMU_LANES) return FlgPlan();
  return flg_plan(nseg, total, want_lambda, FlgShape{block, team, tile, r, team});
}

template <int R, bool WG>
void run(const FlgPlan& p, const u32* nodes, const u32* offsets, size_t nseg, size_t total, const u32* points, const u32* values, u32* lambda, u32* y, uint8_t* flags, u32* work,
         u32* pre, u32* status) {
  const unsigned team = p.team, tile = p.tile;
  launch_threads(p.grid, p.block, [=] { k_flg_segments<R, WG>(nodes, offsets, (u32)nseg, (u32)total, points, values, lambda, y, flags, work, pre, team, tile, status); });
}

}  // namespace

extern "C" {

// info: shape, block, team, tile, r, teams, grid, lds, pre_bytes, work_bytes.  Returns 1, or 0 for a refusal.
int emu_flg_plan(size_t nseg, size_t total, int want_lambda, int which, int block, int team, int tile, int r, size_t* info) {
  const FlgPlan p = plan_of(nseg, total, want_lambda != 0, which, block, team, tile, r);
  if (!p.ok) return 0;
  info[0] = (size_t)p.shape; info[1] = p.block; info[2] = p.team; info[3] = p.tile; info[4] = p.r; info[5] = p.teams; info[6] = p.grid; info[7] = p.lds;
  info[8] = p.pre_bytes; info[9] = p.work_bytes;
  return 1;
}
// the device form of blsgpu_fr_lagrange_segments_device, argument check included: 0, or -1 for what the check or the plan refuses.
// work / pre: exactly work_bytes / pre_bytes of the plan; status: one word.
int emu_flg(const u32* nodes, const u32* offsets, size_t nseg, size_t total, const u32* points, const u32* values, u32* lambda, u32* y, uint8_t* flags, int which, int block,
            int team, int tile, int r, u32* work, u32* pre, u32* status) {
  FlgArgs a;
  a.nodes = nodes; a.offsets = offsets; a.nseg = nseg; a.total = total; a.points = points; a.values = values; a.lambda = lambda; a.y = y; a.flags = flags; a.device = true;
  if (flg_check(a)) return -1;
  if (!nseg) return 0;
  const FlgPlan p = plan_of(nseg, total, lambda != nullptr, which, block, team, tile, r);
  if (!p.ok || p.lds > sizeof(u32) * EMU_DYN_LDS_WORDS || (p.r != 2 && p.r != FLG_R)) return -1;
  const bool wg = p.shape == FLG_SHAPE_BLOCK;
  if (p.r == 2) {
    if (wg) run<2, true>(p, nodes, offsets, nseg, total, points, values, lambda, y, flags, work, pre, status);
    else run<2, false>(p, nodes, offsets, nseg, total, points, values, lambda, y, flags, work, pre, status);
  } else {
    if (wg) run<FLG_R, true>(p, nodes, offsets, nseg, total, points, values, lambda, y, flags, work, pre, status);
    else run<FLG_R, false>(p, nodes, offsets, nseg, total, points, values, lambda, y, flags, work, pre, status);
  }
  return 0;
}
}
