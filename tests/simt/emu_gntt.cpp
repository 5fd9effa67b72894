// tests/simt/emu_gntt.cpp -- the group transform kernels of bls12_381_amd/csrc/gntt.hip.h compiled for the HOST (test infrastructure
// only).  emu_gntt_many builds the Fr tables with the device kernels of fr.hip.h (k_fr_twiddles, k_fr_tw_levels, k_fr_ninv), as
// api_aux.hip does, and then WALKS THE PLAN of csrc/gntt_plan.h -- the function api_msm.hip launches from -- step by step, with its
// grids, blocks and stage indices (tests/test_simt_gntt.py).  The crossover between the two shapes is read from BLSGPU_GNTT_TEAM_MAX
// through gntt_team_max_from, the function the library's diag.h reads it through.
//
// The permutation and the G1 lane shape use no cross-lane operation: their lanes run one after the other in this thread.  The G2 lane
// shape exchanges values inside lane pairs and the team shapes meet at the mailbox barriers: they run with the plan's block size on one
// host thread per lane (tests/simt/hip/hip_runtime.h).
//
// The lane pool, the launchers, the trapping checks and emu_guarded() are those of tests/simt/emu_harness.h; the tests call this
// library from a child process (tests/simt_gntt_child.py).
#define EMU_LANES 256
#include "emu_harness.h"
#include <cstdlib>

#include "fr.hip.h"
#include "gntt.hip.h"

using namespace bls;

namespace {

// api_msm.hip g_ntt_many_device: the loop over the plan
template <class LaneS, class TeamS>
void run_plan(const GnPlan& plan, u32* x, const u32* tw, const u32* ninv, int log_n) {
  for (int i = 0; i < plan.n_steps; i++) {
    const GnStep s = plan.step[i];
    const u32* nv = s.stage ? nullptr : ninv;
    const size_t total = plan.total, B = plan.butterflies;
    if (s.kernel == GN_K_PERMUTE) launch_loop(s.grid, s.block, [=] { k_gntt_permute<LaneS::IO::WW>(x, log_n, total); });
    else if (s.shape == GN_TEAM) launch_threads(s.grid, s.block, [=] { k_gntt_stage<TeamS>(x, tw, nv, s.stage, B); });
    else if (LaneS::LANES == 1) launch_loop(s.grid, s.block, [=] { k_gntt_stage<LaneS>(x, tw, nv, s.stage, B); });
    else launch_threads(s.grid, s.block, [=] { k_gntt_stage<LaneS>(x, tw, nv, s.stage, B); });
  }
}

}  // namespace

extern "C" {

// the plan alone: six ints per step (kernel, shape, grid, block, LDS bytes, stage) into out (at least 6 * 25 ints); returns the number
// of steps, -1 for arguments the entry points refuse.  team_max < 0: BLSGPU_GNTT_TEAM_MAX or the built-in constant, as the library.
int emu_gntt_plan(int group, int log_n, size_t k, long long team_max, int* out) {
  if (log_n < 0 || log_n > GNTT_MAX_LOG || k > (((size_t)1 << GNTT_MAX_LOG) >> log_n)) return -1;
  const GnPlan plan = gntt_plan_many(group, log_n, k, team_max < 0 ? gntt_team_max_from(getenv("BLSGPU_GNTT_TEAM_MAX")) : (size_t)team_max);
  for (int i = 0; i < plan.n_steps; i++) {
    const GnStep& s = plan.step[i];
    int* o = out + 6 * i;
    o[0] = s.kernel; o[1] = s.shape; o[2] = (int)s.grid; o[3] = (int)s.block; o[4] = (int)s.lds; o[5] = s.stage;
  }
  return plan.n_steps;
}

// xyz: k 2^log_n projective wire points (36 / 72 u32 each), transformed in place.  tw: 2^log_n - 1 scalars; ninv: one scalar.
// Returns the number of steps and the shape the plan chose in *shape_out, or -1 for arguments the entry points refuse.
int emu_gntt_many(int group, u32* xyz, u32* tw, u32* ninv, int log_n, size_t k, int inverse, int* shape_out) {
  if (log_n < 0 || log_n > GNTT_MAX_LOG || k > (((size_t)1 << GNTT_MAX_LOG) >> log_n)) return -1;
  const GnPlan plan = gntt_plan_many(group, log_n, k, gntt_team_max_from(getenv("BLSGPU_GNTT_TEAM_MAX")));
  *shape_out = plan.shape;
  if (!plan.n_steps) return 0;                       // no launch, no table
  if ((size_t)plan.step[1].lds > sizeof(u32) * EMU_DYN_LDS_WORDS || plan.step[1].block > EMU_LANES) return -1;
  const int dir = inverse ? 1 : 0;
  const size_t half = ((size_t)1 << log_n) >> 1;
  // api_aux.hip fr_twiddles_ready / fr_ninv_ready
  launch_loop(nblk((half + FR_TW_RUN - 1) / FR_TW_RUN, 256), 256, [=] { k_fr_twiddles(tw, log_n, dir); });
  if (log_n > 1) launch_loop(nblk(half, 256), 256, [=] { k_fr_tw_levels(tw, log_n); });
  const u32* nv = nullptr;
  if (inverse) { launch_loop(1, 64, [=] { k_fr_ninv(ninv, log_n); }); nv = ninv; }
  if (group == 1) run_plan<GnG1Lane, GnG1Team>(plan, xyz, tw, nv, log_n);
  else run_plan<GnG2Lane, GnG2Team>(plan, xyz, tw, nv, log_n);
  return plan.n_steps;
}
}
