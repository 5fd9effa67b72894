// tests/simt/emu_fr_edwards.cpp -- the twisted Edwards kernels of bls12_381_amd/csrc/fr_edwards.hip.h compiled for the HOST (test
// infrastructure only).  Every entry point runs the argument check of csrc/fr_edwards_plan.h and then WALKS ITS PLAN -- the functions
// api_fr.hip launches from -- with its grids, blocks and LDS sizes, at the shipped shape (block == 0) or at whatever shape the test asks
// for: 4 lanes of 2 terms make an MSM chunk of 8 terms, so a few dozen terms reach every path of the two passes.
//
// Over tests/simt/emu_harness.h: the kernels that meet at barriers or shuffle (normalize, the two MSM passes) run one host thread per
// lane; check, mul_batch, the table build and the MSM's PREP have no cross-lane operation and run their lanes one after the other.  The
// library is built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call it from a child process (tests/simt_fr_edwards_child.py).  -DFR_EDWARDS_FAULT=n builds the kernels with one of their
// seeded wrong-result variants (tests/test_simt_fr_edwards.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (64 * 4 * 32)                            // fred_mul_lds_bytes of the shipped shape, the largest of the family
#include "emu_harness.h"

#include "fr_edwards.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::fred_mul_lds_bytes(FRED_MUL_BLOCK) && sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::fred_msm_lds_bytes(FRED_MSM_BLOCK),
              "EMU_DYN_LDS_WORDS is smaller than the shipped shapes' LDS");

using namespace bls;

namespace {

EdArgs curve_args(const u32* a, const u32* d) {
  EdArgs k;
  for (int i = 0; i < 8; i++) { k.a.w[i] = a[i]; k.d.w[i] = d[i]; }
  return k;
}
bool lds_fits(size_t bytes) { return bytes <= sizeof(u32) * EMU_DYN_LDS_WORDS; }

}  // namespace

extern "C" {

int emu_fred_check(const u32* a, const u32* d, const u32* xy, size_t n, uint8_t* ok) {
  if (fred_check_args(xy, n, ok, true)) return -1;
  if (!n) return 0;
  const FredLaunch l = fred_points_launch(n);
  const EdArgs c = curve_args(a, d);
  launch_loop(l.grid, l.block, [=] { k_fred_check(c, xy, n, ok); });
  return 0;
}

// block: lanes per workgroup (a multiple of 64), 0 = the shipped one
int emu_fred_normalize(const u32* a, const u32* d, const u32* xyz, size_t n, u32* xy, uint8_t* ok, int block) {
  if (fred_normalize_args(xyz, n, xy, ok, true)) return -1;
  if (!n) return 0;
  if (block && (block % 64 || block > EMU_LANES)) return -1;
  const FredLaunch l = block ? fred_points_launch(n, block) : fred_points_launch(n);
  const EdArgs c = curve_args(a, d);
  launch_threads(l.grid, l.block, [=] { k_fred_normalize<false>(c, xyz, n, xy, ok); });
  return 0;
}

// info: W, doublings, grid, block, lds
int emu_fred_mul_plan(size_t n, int bits, int block, size_t* info) {
  const FredMulPlan p = block ? fred_mul_plan(n, bits, block) : fred_mul_plan(n, bits);
  if (!p.ok) return 0;
  info[0] = p.W; info[1] = p.doublings; info[2] = p.mul.grid; info[3] = p.mul.block; info[4] = p.mul.lds;
  return 1;
}
int emu_fred_mul(const u32* a, const u32* d, const u32* xy, const u32* scalars, int bits, size_t n, u32* out, u32* status, int block) {
  if (fred_mul_args(xy, scalars, bits, n, out, true)) return -1;
  if (!n) return 0;
  const FredMulPlan p = block ? fred_mul_plan(n, bits, block) : fred_mul_plan(n, bits);
  if (!p.ok || !lds_fits(p.mul.lds)) return -1;
  const EdArgs c = curve_args(a, d);
  launch_loop(p.mul.grid, p.mul.block, [=] { k_fred_mul(c, xy, scalars, bits, n, out, status); });
  return 0;
}

// info: W, H, entries, bytes.  Returns 1, or 0 for a refusal.
int emu_fred_table_plan(size_t n, int bits, int window, size_t* info) {
  const FredTablePlan p = fred_table_plan(n, bits, window);
  if (!p.ok) return 0;
  info[0] = p.W; info[1] = p.H; info[2] = p.entries; info[3] = p.bytes;
  return 1;
}
// table: exactly `bytes` of the plan; flag: one word, set when a base is not on the curve
int emu_fred_table(const u32* a, const u32* d, const u32* xy, size_t n, int bits, int window, u32* table, u32* flag) {
  const FredTablePlan p = fred_table_plan(n, bits, window);
  if (!p.ok || !xy || fred_misaligned(xy)) return -1;
  const EdArgs c = curve_args(a, d);
  launch_loop(p.build.grid, p.build.block, [=] { k_fred_table_build(c, xy, p.n, p.window, p.W, p.H, table, flag); });
  launch_threads(p.norm.grid, p.norm.block, [=] { k_fred_normalize<true>(c, table, p.entries, table, nullptr); });
  return 0;
}

// info: off_bytes, part_bytes, meta_bytes, chunk, nchunks, chunks_grid, combine_grid, lds, block, terms.  Returns 1, or 0 for a refusal.
int emu_fred_msm_plan(size_t k, size_t total, int block, int terms, size_t* info) {
  const FredMsmPlan p = block ? fred_msm_plan(k, total, FredMsmShape{block, terms}) : fred_msm_plan(k, total);
  if (!p.ok || p.cut.block > EMU_LANES) return 0;
  info[0] = p.off_bytes; info[1] = p.part_bytes; info[2] = p.meta_bytes; info[3] = p.cut.chunk; info[4] = p.cut.nchunks; info[5] = p.chunks.grid; info[6] = p.combine.grid;
  info[7] = p.chunks.lds; info[8] = p.cut.block; info[9] = p.cut.terms;
  return 1;
}
// the device form of blsgpu_fr_edwards_msm_segments_device, argument check included: 0, or -1 for what the check or the plan refuses.
// off64 / part / meta: exactly off_bytes / part_bytes / meta_bytes of the plan; status: one word.
int emu_fred_msm(const u32* a, const u32* d, const u32* table, size_t nbases, int bits, int window, const u32* base_first, const u32* offsets, const u32* scalars, size_t k,
                 size_t total, int block, int terms, u32* out, unsigned long long* off64, u32* part, u32* meta, u32* status) {
  FredMsmArgs ar;
  ar.nbases = nbases; ar.base_first = base_first; ar.offsets = offsets; ar.scalars = scalars; ar.k = k; ar.total = total; ar.out = out; ar.device = true;
  if (fred_msm_args(ar)) return -1;
  if (!k) return 0;
  const FredMsmPlan p = block ? fred_msm_plan(k, total, FredMsmShape{block, terms}) : fred_msm_plan(k, total);
  if (!p.ok || p.cut.block > EMU_LANES || !lds_fits(p.chunks.lds)) return -1;
  EdMsmArgs m;
  m.c = curve_args(a, d); m.table = table; m.nbases = (u32)nbases; m.bits = bits; m.window = window; m.W = fred_windows(bits, window); m.H = fred_table_half(window);
  const unsigned t = p.cut.terms;
  const u32 chunk = p.cut.chunk;
  const size_t nchunks = p.cut.nchunks;
  launch_loop(p.prep.grid, p.prep.block, [=] { k_fred_msm_prep(offsets, base_first, k, (u32)total, nbases, off64, status); });
  if (p.chunks.grid)
    launch_threads(p.chunks.grid, p.chunks.block, [=] { k_fred_msm_chunks(m, base_first, scalars, off64, (u32)k, (u32)total, t, out, part, meta, status); });
  launch_threads(p.combine.grid, p.combine.block, [=] { k_fred_msm_combine(m.c, off64, (u32)k, (u32)total, chunk, nchunks, part, meta, out); });
  return 0;
}
}
