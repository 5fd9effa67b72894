// tests/simt/emu_fr_lookup.cpp -- the Fr lookup kernels (bls12_381_amd/csrc/fr_lookup.hip.h) compiled for the HOST (test
// infrastructure only).  emu_fr_lookup_run builds a table and counts against it with k_frl_build, k_frl_count and k_frl_finish launched
// FROM THE PLAN of csrc/fr_lookup_plan.h -- the function api_fr.hip launches from -- at whatever block and path threshold the test asks
// for: at block 64 a table of 1000 rows is built by sixteen workgroups, and with the threshold lowered to 64 a table of 65 rows takes the
// cache path.
//
// Over tests/simt/emu_harness.h.  The kernels use atomics and barriers, so the lanes of a workgroup are host threads
// (launch_threads); workgroups run one after the other, in ascending or -- `reverse` -- descending order (a GPU promises neither; with
// the later rows first, only the atomicMin makes the FIRST row of a repeated key its representative).  The library is built with the
// trapping bounds / shift checks, every buffer (the handle's keys, slots and counters included) ends flush against an inaccessible page,
// and the tests call this library from a child process (tests/simt_fr_lookup_child.py).  -DFRL_HASH_BITS=2 keeps two bits of the hash
// and sets all others, so every probe chain starts in the last four slots and wraps; -DFRL_FAULT=n builds the kernels with one of their
// five seeded faults (tests/test_simt_fr_lookup.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS 4096                                     // FRL_LDS_ROWS counters = 2 * FRL_CACHE words
#include "emu_harness.h"

// tests/simt/hip/hip_runtime.h has no compare-and-swap and no minimum on `unsigned`
static inline unsigned atomicCAS(unsigned* p, unsigned cmp, unsigned v) {
  __atomic_compare_exchange_n(p, &cmp, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return cmp;
}
static inline unsigned atomicMin(unsigned* p, unsigned v) {
  unsigned old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_RELAXED)) {}
  return old;
}

#include "fr_lookup.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::FRL_LDS_ROWS * 4 && sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::FRL_CACHE * 8, "EMU_DYN_LDS_WORDS is smaller than the shipped LDS");

using namespace bls;

namespace {

FrLookupPlan plan_of(size_t rows, size_t n, int block, size_t lds_rows) {
  if (block > EMU_LANES) return FrLookupPlan();
  return fr_lookup_plan(rows, n, block ? block : FRL_BLOCK, lds_rows ? lds_rows : FRL_LDS_ROWS);
}
template <class Fn> void launch_ordered(unsigned grid, unsigned block, bool reverse, Fn fn) {
  for (unsigned i = 0; i < grid; i++) pool()->workgroup(grid, block, reverse ? grid - 1 - i : i, fn);
}

}  // namespace

extern "C" {

// info: slots, block, build_grid, lds_path, count_lds, count_grid, iters, finish_grid.  Returns 1, or 0 for a refusal.
int emu_fr_lookup_plan(size_t rows, size_t n, int block, size_t lds_rows, size_t* info) {
  const FrLookupPlan p = plan_of(rows, n, block, lds_rows);
  info[0] = p.slots; info[1] = p.block; info[2] = p.build_grid; info[3] = (size_t)p.lds_path; info[4] = p.count_lds; info[5] = p.count_grid; info[6] = p.iters; info[7] = p.finish_grid;
  return p.ok;
}
uint32_t emu_fr_lookup_hash(const uint32_t* key, int c) { return frl_hash(key, c); }
// t: c columns of `rows` scalars at t_pitch; f: c columns of n scalars at f_pitch; mult (rows scalars), index (n words), missing (one
// 64-bit word): each may be NULL.  info: distinct, slots, lds_path, count_grid.  Returns 0, or -1 for what the plan refuses.
int emu_fr_lookup_run(int c, const u32* t, size_t t_pitch, size_t rows, const u32* f, size_t f_pitch, size_t n, int negate, int block, size_t lds_rows, int reverse,
                      u32* mult, u32* index, unsigned long long* missing, size_t* info) {
  const FrLookupPlan p = plan_of(rows, n, block, lds_rows);
  if (!p.ok || p.count_lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
  u32* keys = (u32*)emu_guarded(rows * (size_t)c * 32);
  u32* slot = (u32*)emu_guarded(p.slots * 4);
  u32* counters = (u32*)emu_guarded(rows * 4);
  if (!keys || !slot || !counters) return -1;
  for (size_t i = 0; i < p.slots; i++) slot[i] = 0;
  for (size_t i = 0; i < rows; i++) counters[i] = 0xdeadbeefu;      // stale scratch: the count call must zero what it uses
  counters[0] = 0;
  const u32 mask = (u32)(p.slots - 1);
  launch_ordered(p.build_grid, p.block, reverse != 0, [=] { k_frl_build(t, t_pitch, (u32)rows, c, keys, slot, mask, counters); });
  info[0] = counters[0]; info[1] = p.slots; info[2] = (size_t)p.lds_path; info[3] = p.count_grid;
  if (missing) *missing = 0;
  if (mult) for (size_t i = 0; i < rows; i++) counters[i] = 0;
  u32* cnt = mult ? counters : nullptr;
  const unsigned iters = p.iters;
  if (p.count_grid && (mult || index || missing)) {
    if (p.lds_path) launch_threads(p.count_grid, p.block, [=] { k_frl_count<true>(f, f_pitch, n, c, keys, slot, mask, (u32)rows, iters, cnt, index, missing); });
    else launch_threads(p.count_grid, p.block, [=] { k_frl_count<false>(f, f_pitch, n, c, keys, slot, mask, (u32)rows, iters, cnt, index, missing); });
  }
  if (mult) launch_threads(p.finish_grid, p.block, [=] { k_frl_finish(counters, (u32)rows, negate, mult); });
  return 0;
}
}
