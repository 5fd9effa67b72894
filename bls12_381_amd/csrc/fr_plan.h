// fr_plan.h -- the launch plan of the batched Fr transform (blsgpu_fr_ntt_many*) as plain host code: which kernels of fr.hip.h run, in
// which order, with which grid / block / dynamic LDS and arguments, for k vectors of 2^log_n scalars laid end to end.  No HIP calls
// here: api_fr.hip walks the plan and launches, tests/simt/emu_fr.cpp walks the same plan on the host.
//
//   log_n <= FR_TILE_LOG   one launch of k_fr_tile<true>, IN PLACE: a workgroup takes a tile of 2^tile_log consecutive elements of the
//                          concatenated array, i.e. whole vectors, and has read all of them into LDS before its first store.
//   log_n >  FR_TILE_LOG   the top log_n - FR_TILE_LOG stages over global memory (k_fr_cols / k_fr_stage2 / k_fr_stage1 address
//                          butterfly blocks of 2^(lh+1) elements, so the concatenation of k vectors is k times as many blocks), the first
//                          of them data -> scratch, the others in the scratch buffer, then k_fr_tile<true> scratch -> data.
// A forward coset shift is applied by whichever step reads the data first (`coset_in`); the inverse one replaces the n^-1 scale on the
// store of the tile kernel (`coset_out`).
#pragma once
#include <stddef.h>

namespace bls {

constexpr int FR_PLAN_TILE_LOG = 10;              // = FR_TILE_LOG (fr.hip.h static_asserts it)
enum FrKernel { FR_K_COLS = 0, FR_K_STAGE2 = 1, FR_K_STAGE1 = 2, FR_K_TILE = 3 };
enum FrBuf { FR_BUF_DATA = 0, FR_BUF_TMP = 1 };

struct FrStep {
  int kernel;                  // FrKernel
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS
  int src, dst;                // FrBuf
  int lh;                      // cols: lh_top; stage1 / stage2: log_h; tile: unused
  int d, lk;                   // cols: stages of the pass, log2 of the adjacent columns; tile: d = tile_log
  bool coset_in;               // multiply by the forward coset table on the load
  bool coset_out;              // tile: scale by the inverse coset table (n^-1 g^-j) on the store instead of n^-1
};
struct FrPlan {
  int n_steps = 0;
  FrStep step[32];
  size_t total = 0;            // k * 2^log_n
  bool needs_tmp = false;      // a scratch buffer of total * 32 bytes
};
// the shape of the column-tile passes: tile log2, stages per pass, lanes (api_fr.hip: 11, 7, 512 measured; BLSGPU_NTT_COLS overrides)
struct FrColsShape { int tlog = 11, dmax = 7, block = 512; };

// log_n in [0, 28], k * 2^log_n <= 2^28.  use_cols: the column-tile passes are usable AND wanted for this log_n.
inline FrPlan fr_plan_many(int log_n, size_t k, bool inverse, bool coset, bool use_cols, FrColsShape cs = FrColsShape()) {
  FrPlan p;
  const size_t total = k << log_n;
  p.total = total;
  if (log_n == 0 || k == 0) return p;              // no step: a vector of one element is its own transform, on any coset (g^0 = 1)
  bool first = coset && !inverse;                  // the forward shift belongs to the first step that reads the data
  auto push = [&](FrStep s) { s.coset_in = first; s.coset_out = false; first = false; p.step[p.n_steps++] = s; };
  if (log_n <= FR_PLAN_TILE_LOG) {
    // tiles of whole vectors; a call smaller than one tile takes the smallest power of two that holds it
    int tile_log = FR_PLAN_TILE_LOG;
    while (tile_log > log_n && ((size_t)1 << (tile_log - 1)) >= total) tile_log--;
    FrStep s{FR_K_TILE, (unsigned)((total + ((size_t)1 << tile_log) - 1) >> tile_log), 256, ((size_t)9 << tile_log) * 4, FR_BUF_DATA, FR_BUF_DATA, 0, tile_log, 0, false, false};
    push(s);
    p.step[p.n_steps - 1].coset_out = coset && inverse;
    return p;
  }
  p.needs_tmp = true;
  const int tl = FR_PLAN_TILE_LOG;
  int lh = log_n - 1;
  int src = FR_BUF_DATA;
  if (use_cols) {
    const int m = lh + 1 - tl, passes = (m + cs.dmax - 1) / cs.dmax;
    for (int ps = 0; ps < passes; ps++) {
      const int d = (lh + 1 - tl + (passes - ps) - 1) / (passes - ps);      // the remaining stages split evenly over the remaining passes
      const int ls = lh - d + 1;
      const int lk = cs.tlog - d < ls ? cs.tlog - d : ls;
      push(FrStep{FR_K_COLS, (unsigned)(total >> (d + lk)), (unsigned)cs.block, ((size_t)9 << (d + lk)) * 4, src, FR_BUF_TMP, lh, d, lk, false, false});
      src = FR_BUF_TMP; lh -= d;
    }
  }
  while (lh - 1 >= tl) {                           // two stages per pass over the data
    push(FrStep{FR_K_STAGE2, (unsigned)((total / 4 + 255) / 256), 256, 0, src, FR_BUF_TMP, lh, 0, 0, false, false});
    src = FR_BUF_TMP; lh -= 2;
  }
  if (lh >= tl) { push(FrStep{FR_K_STAGE1, (unsigned)((total / 2 + 255) / 256), 256, 0, src, FR_BUF_TMP, lh, 0, 0, false, false}); src = FR_BUF_TMP; lh--; }
  push(FrStep{FR_K_TILE, (unsigned)(total >> tl), 256, ((size_t)9 << tl) * 4, FR_BUF_TMP, FR_BUF_DATA, 0, tl, 0, false, false});
  p.step[p.n_steps - 1].coset_out = coset && inverse;
  return p;
}

}  // namespace bls
