// fr_spmv_plan.h -- the launch plan of the sparse matrix-vector product over Fr (blsgpu_fr_spmv*) as plain host code: which kernels of
// fr_spmv.hip.h run, in which order, with which grid / block / dynamic LDS, and how large the scratch records are.  No HIP calls here:
// api_fr.hip walks the plan and launches, tests/simt/emu_fr_spmv.cpp walks the same plan on the host -- with a small tile, so that rows
// crossing several tiles are reached at a few hundred non-zeros.
//
// The NON-ZEROS of the CSR matrix, not its rows, are cut into tiles of `block` lanes x `chunk` consecutive entries, so the work of a
// workgroup is the same whatever the row lengths are.  Every step is a launch of its own on the stream (no workgroup waits for another):
//
//   FILL    out = 0 for all k * n_rows outputs    only when the matrix has an empty row (nobody else writes those), or no entry at all
//   TILE    one workgroup per tile, all k right-hand sides inside it: products, segmented sum, rows that begin and end in the tile are
//           written; what is left are two records per (tile, vector)
//             HEAD[t]  the sum of the tile's entries up to the first row end (the whole tile if no row ends in it): the continuation of
//                      a row that began in an earlier tile -- read only when tile t begins in the middle of a row
//             TAIL[t]  the sum of the entries behind the last row end, when that row began in tile t and goes on beyond it
//           and META[t] = 1 + that row's index (0: the tile leaves no open row that began in it)
//   FIXUP   one wavefront per tile with META[t] != 0: out[row] = TAIL[t] + HEAD[t+1] + ... + HEAD[t_end], t_end = the tile of the row's
//           last entry (known from row_ptr: nothing is searched).  Absent when there is one tile.
// A row is written exactly once: by TILE when it lies inside one tile, by FIXUP for the tile it begins in otherwise.
#pragma once
#include <stddef.h>

namespace bls {

constexpr int FRSP_BLOCK = 256;                   // lanes per workgroup (a multiple of 64: the block scan and FIXUP use whole wavefronts)
constexpr int FRSP_CHUNK = 8;                     // consecutive non-zeros a lane owns
constexpr size_t FRSP_MAX = (size_t)1 << 28;      // nnz, n_rows, n_cols, k * max(n_rows, n_cols)

enum FrSpmvKernel { FRSP_K_FILL = 0, FRSP_K_TILE = 1, FRSP_K_FIXUP = 2 };

struct FrSpmvShape { int block = FRSP_BLOCK, chunk = FRSP_CHUNK; };

// dynamic LDS of the tile kernel: the values staged as in fr_scan.hip.h (frs_lds_addr: eight words per entry, four words of padding per
// lane chunk), one column index per entry, one SUM record of the block scan per wavefront.  Shipped shape: 78 144 bytes, two workgroups
// in a CU's 160 KB.
constexpr size_t frsp_lds_words(FrSpmvShape s) { return (size_t)s.block * (s.chunk * 8 + 4) + (size_t)s.block * s.chunk + (size_t)(s.block / 64) * 20; }
constexpr size_t frsp_lds_bytes(FrSpmvShape s) { return frsp_lds_words(s) * 4; }
static_assert(2 * frsp_lds_bytes(FrSpmvShape()) <= 160 * 1024, "two workgroups of the shipped shape must fit a CU's LDS");

struct FrSpmvStep {
  int kernel;                  // FrSpmvKernel
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS
  size_t items;                // FILL: scalars to zero; TILE: non-zeros; FIXUP: tiles
};
struct FrSpmvPlan {
  int n_steps = 0;
  FrSpmvStep step[3];
  size_t tile = 0, tiles = 0;
  size_t rec_scalars = 0;      // scalars (eight u32) each of HEAD and TAIL must hold: tiles * k
  size_t meta_words = 0;       // u32 of META: tiles
};

inline size_t frsp_tiles(size_t nnz, FrSpmvShape s = FrSpmvShape()) {
  const size_t tile = (size_t)s.block * s.chunk;
  return (nnz + tile - 1) / tile;
}

// has_empty: the matrix has a row without entries (decided once, at upload)
inline FrSpmvPlan fr_spmv_plan(size_t n_rows, size_t nnz, size_t k, bool has_empty, FrSpmvShape s = FrSpmvShape()) {
  FrSpmvPlan p;
  p.tile = (size_t)s.block * s.chunk;
  if (!n_rows || !k) return p;
  p.tiles = frsp_tiles(nnz, s);
  const unsigned b = (unsigned)s.block;
  if (has_empty || !nnz) p.step[p.n_steps++] = FrSpmvStep{FRSP_K_FILL, 0, 0, 0, k * n_rows};
  if (!nnz) return p;
  p.rec_scalars = p.tiles * k;
  p.meta_words = p.tiles;
  p.step[p.n_steps++] = FrSpmvStep{FRSP_K_TILE, (unsigned)p.tiles, b, frsp_lds_bytes(s), nnz};
  const size_t per = (size_t)s.block / 64;           // tiles a FIXUP workgroup takes: one per wavefront
  if (p.tiles > 1) p.step[p.n_steps++] = FrSpmvStep{FRSP_K_FIXUP, (unsigned)((p.tiles + per - 1) / per), b, 0, p.tiles};
  return p;
}

}  // namespace bls
