// tests/simt/emu_kzg_recover.cpp -- the kernels of bls12_381_amd/csrc/kzg_recover.hip.h compiled for the HOST (test infrastructure only).
// Every entry point below is ONE stage of blsgpu_kzg_recover_device, launched with the grids of csrc/kzg_recover_plan.h -- the function
// api_fr.hip launches from -- at whatever scatter tile (4, or 0 for the shipped KZGR_TILE) and root tile (0 for the shipped
// KZGR_ROOT_TILE) the test asks for.  The transforms and the batch inversion between the stages are the test's (tests/kzg_recover_ref.py,
// in Python integers).
//
// Over tests/simt/emu_harness.h: every launch runs its block on one host thread per lane, the library is built with the trapping
// bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the tests call this library from a
// child process (tests/simt_kzg_recover_child.py).  -DKZG_REC_FAULT=n builds the kernels with one of their seeded faults.
#define EMU_LANES 256
#include "emu_harness.h"

// the LDS compare-and-swap of k_kzg_rec_slots
static inline int atomicCAS(int* p, int expected, int desired) {
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  return expected;
}

#include "kzg_recover.hip.h"

using namespace bls;

extern "C" {

// info: ok, bytes, eff, mis, slot, status, upper, rootd, rootc, zd, zc, work, coef, scalars, tables, offsets_grid, slots_grid, roots_grid, vanish_per_poly, vanish_grid,
//       scatter_block, scatter_grid, scale_grid, finish_per_poly, finish_grid
void emu_kzgr_plan(int log_n, int log_l, size_t count, size_t m, int coef_scratch, int tile, size_t* info) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, coef_scratch != 0, (unsigned)tile);
  const size_t v[25] = {(size_t)p.ok, p.bytes, p.eff, p.mis, p.slot, p.status, p.upper, p.rootd, p.rootc, p.zd, p.zc, p.work, p.coef, (size_t)p.scalars, (size_t)p.tables,
                        p.offsets_grid, p.slots_grid, p.roots_grid, p.vanish_per_poly, p.vanish_grid, p.scatter_block, p.scatter_grid, p.scale_grid, p.finish_per_poly, p.finish_grid};
  for (int i = 0; i < 25; i++) info[i] = v[i];
}
int emu_kzgr_offsets(const u32* offsets, size_t count, size_t m, int log_n, int log_l, u32* eff, uint8_t* mis) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, false);
  if (!p.ok || !count) return -1;
  launch_threads(p.offsets_grid, KZGR_BLOCK, [=] { k_kzg_rec_offsets(offsets, (u32)count, (u32)m, eff, mis); });
  return 0;
}
int emu_kzgr_slots(const u32* eff, const uint8_t* mis, const u32* col, size_t count, size_t m, int log_n, int log_l, int* slot, u32* status, u32* upper, u32* sticky) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, false);
  if (!p.ok || !count) return -1;
  launch_threads(p.slots_grid, KZGR_BLOCK, [=] { k_kzg_rec_slots(eff, mis, col, p.log_c, slot, status, upper, sticky); });
  return 0;
}
int emu_kzgr_roots(u32* rootd, u32* rootc, int log_n, int log_l) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, 1, 0, false);
  if (!p.ok) return -1;
  FrArg g;
  for (int i = 0; i < 8; i++) g.w[i] = (u32)(KZGR_GEN_MONT[i >> 1] >> (32 * (i & 1)));
  launch_loop(p.roots_grid, KZGR_BLOCK, [=] { k_kzg_rec_roots(rootd, rootc, g, p.log_c, log_l); });
  return 0;
}
int emu_kzgr_vanish(const int* slot, const u32* status, const u32* rootd, const u32* rootc, size_t count, int log_n, int log_l, int order, int root_tile, u32* zd, u32* zc) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, 0, false);
  if (!p.ok || !count || root_tile < 0 || (unsigned)root_tile > KZGR_ROOT_TILE) return -1;
  const u32 tile = root_tile ? (u32)root_tile : KZGR_ROOT_TILE;
  launch_threads(p.vanish_grid, KZGR_BLOCK, [=] { k_kzg_rec_vanish(slot, status, rootd, rootc, p.log_c, order, p.vanish_per_poly, tile, zd, zc); });
  return 0;
}
int emu_kzgr_scatter(const int* slot, const void* cells, const u32* zd, size_t count, size_t m, int log_n, int log_l, int order, int tile, void* ez) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, false, (unsigned)tile);
  if (!p.ok || !count) return -1;
  if (p.tile == 4) launch_threads(p.scatter_grid, p.scatter_block, [=] { k_kzg_rec_scatter<4>(slot, (const uint4*)cells, zd, count, p.log_c, log_l, order, (uint4*)ez); });
  else if (p.tile == KZGR_TILE) launch_threads(p.scatter_grid, p.scatter_block, [=] { k_kzg_rec_scatter<KZGR_TILE>(slot, (const uint4*)cells, zd, count, p.log_c, log_l, order, (uint4*)ez); });
  else return -1;
  return 0;
}
int emu_kzgr_scale(u32* x, const u32* zcinv, size_t count, int log_n, int log_l) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, 0, false);
  if (!p.ok || !count) return -1;
  launch_loop(p.scale_grid, KZGR_BLOCK, [=] { k_kzg_rec_scale(x, zcinv, (size_t)p.scalars, log_n, p.log_c); });
  return 0;
}
int emu_kzgr_check(const u32* q, size_t count, int log_n, int log_l, u32* upper) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, 0, false);
  if (!p.ok || !count) return -1;
  launch_threads(p.finish_grid, KZGR_BLOCK, [=] { k_kzg_rec_check(q, log_n, p.finish_per_poly, upper); });
  return 0;
}
int emu_kzgr_finish(const void* q, const u32* status, const u32* upper, size_t count, int log_n, int log_l, void* out, uint8_t* ok) {
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, 0, false);
  if (!p.ok || !count) return -1;
  launch_loop(p.finish_grid, KZGR_BLOCK, [=] { k_kzg_rec_finish((const uint4*)q, status, upper, log_n, p.finish_per_poly, (uint4*)out, ok); });
  return 0;
}
}
