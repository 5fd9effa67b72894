// tests/simt/emu_gsum.cpp -- the segmented point sums of bls12_381_amd/csrc/gsum.hip.h compiled for the HOST (test infrastructure
// only).  emu_gsum WALKS THE PLAN of csrc/gsum_plan.h -- the function api_msm.hip launches from -- with its grids, block and LDS size,
// at whatever (block, terms) the test asks for: 4 lanes of 2 terms make a chunk of 8 terms, so a few dozen terms reach every path
// (a head that meets the lane before it, a segment over several chunks, the combine pass's tree).  block == 0 takes the shipped shape.
//
// Over tests/simt/emu_harness.h: every launch runs its block on one host thread per lane, the library is built with the trapping
// bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page (an index >= npoints that WAS dereferenced
// ends the process), and the tests call this library from a child process (tests/simt_gsum_child.py).  -DGSUM_FAULT=n builds the
// kernels with one of their seeded faults (tests/test_simt_gsum.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (44 + 2))                         // gsum_lds_bytes of the larger shipped shape (G1: 256 lanes)
#include "emu_harness.h"

#include "convert.hip.h"
#include "gsum.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::gsum_lds_bytes(1, GSUM_BLOCK_G1) && sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::gsum_lds_bytes(2, GSUM_BLOCK_G2),
              "EMU_DYN_LDS_WORDS is smaller than the shipped shapes' LDS");

using namespace bls;

namespace {

GsumPlan plan_of(int group, size_t nseg, size_t total, int block, int terms) {
  if (block == 0) return gsum_plan(group, nseg, total);
  if (block > EMU_LANES) return GsumPlan();
  return gsum_plan(group, nseg, total, GsumShape{block, terms});
}

template <class F>
void run(const GsumPlan& plan, const u32* xy, const uint8_t* inf, size_t npoints, const u32* idx, const unsigned long long* offsets, size_t nseg, size_t total, u32* out, u32* part,
         u32* meta, u32* status) {
  const unsigned terms = plan.terms;
  const u32 chunk = plan.chunk;
  const size_t nchunks = plan.nchunks;
  if (plan.chunks_grid)
    launch_threads(plan.chunks_grid, plan.block, [=] { k_gsum_chunks<F>(xy, inf, (u32)npoints, idx, offsets, (u32)nseg, (u32)total, terms, out, part, meta, status); });
  launch_threads(plan.combine_grid, plan.block, [=] { k_gsum_combine<F>(offsets, (u32)nseg, (u32)total, chunk, nchunks, part, meta, out); });
}

}  // namespace

extern "C" {

// info: part_bytes, meta_bytes, chunk, nchunks, chunks_grid, combine_grid, lds, block, terms.  Returns 1, or 0 for a refusal.
int emu_gsum_plan(int group, size_t nseg, size_t total, int block, int terms, size_t* info) {
  const GsumPlan p = plan_of(group, nseg, total, block, terms);
  if (!p.ok) return 0;
  info[0] = p.part_bytes; info[1] = p.meta_bytes; info[2] = p.chunk; info[3] = p.nchunks; info[4] = p.chunks_grid; info[5] = p.combine_grid; info[6] = p.lds;
  info[7] = p.block; info[8] = p.terms;
  return 1;
}
// the device form of blsgpu_g{1,2}_sum_segments_device, argument check included: 0, or -1 for what the check or the plan refuses.
// part / meta: exactly part_bytes / meta_bytes of the plan; status: one word.
int emu_gsum(int group, const u32* xy, const uint8_t* inf, size_t npoints, const u32* idx, const unsigned long long* offsets, size_t nseg, size_t total, int block, int terms,
             u32* out, u32* part, u32* meta, u32* status) {
  GsumArgs a;
  a.group = group; a.xy = xy; a.inf = inf; a.npoints = npoints; a.idx = idx; a.offsets = offsets; a.nseg = nseg; a.total = total; a.out = out; a.device = true;
  if (gsum_check(a)) return -1;
  if (!nseg) return 0;
  const GsumPlan plan = plan_of(group, nseg, total, block, terms);
  if (!plan.ok || plan.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
  if (group == 1) run<FpPolicy>(plan, xy, inf, npoints, idx, offsets, nseg, total, out, part, meta, status);
  else run<Fp2Policy>(plan, xy, inf, npoints, idx, offsets, nseg, total, out, part, meta, status);
  return 0;
}
}
