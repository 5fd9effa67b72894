// fr_bary_plan.h -- the launch plan of the evaluation-form openings (blsgpu_fr_bary_eval_many* / blsgpu_fr_bary_open_many*) as plain host
// code: which kernels of fr_bary.hip.h run, in which order, with which grid / block / dynamic LDS, on which buffers.  No HIP calls here:
// api_fr.hip walks the plan and launches, tests/simt/emu_fr_bary.cpp walks the same plan on the host -- with a small tile, so that both
// shapes are reached at a few hundred elements.
//
// k rows of n = 2^log_n evaluations lie end to end; a tile is `block` lanes x `chunk` consecutive elements.  Rows and tiles are powers of
// two, so a tile holds whole rows or a row holds whole tiles:
//
//   n <= tile      ROWS                    one launch: a workgroup owns tile / n whole rows (the last tile of the call may be partial)
//   n >  tile      TILE  ROW               eval: one record per tile, then one workgroup per row sums its records and writes y
//                  TILE  ROW  QUOT         open: TILE also parks 1 / (z - D[i]) in q, ROW also writes q[j] of a row whose z = D[j],
//                                          QUOT rewrites every other q[i] in place as (y - f[i]) / (z - D[i])
// Every step is a launch of its own on the stream (no workgroup ever waits for another), and the sequence depends on the shape alone:
// whether a row's point lies in the domain is found and resolved on the device.
//
// Buffers: evals / points / y / q are the caller's.  REC holds one record per tile (TILE writes, ROW reads): the tile's sums
// A = sum f[i] / (z - D[i]) -- without the element where z = D[i] --, F = sum f[i], that element's f, and its index in the row + 1
// (0: none).  ROWREC holds one record per row (ROW writes, QUOT reads): y and the same index.
#pragma once
#include <stddef.h>

namespace bls {

constexpr int FRB_BLOCK = 256;                    // lanes per workgroup (a multiple of 64: the cross-lane sums use whole wavefronts)
constexpr int FRB_CHUNK = 8;                      // consecutive elements a lane owns: a power of two, at most FRS_CHUNK_MAX (the chunk's inverses stay in registers)
constexpr int FRB_REC_WORDS = 28;                 // A (8), F (8), f[j] (8), j + 1 (1), padding to 16 bytes (3)
constexpr int FRB_ROWREC_WORDS = 12;              // y (8), j + 1 (1), padding (3)
constexpr int FRB_WREC_WORDS = 20;                // LDS, one per wavefront: A, F, j + 1, padding
constexpr size_t FRB_MAX_TOTAL = (size_t)1 << 28;

enum FrBaryKernel { FRB_K_ROWS = 0, FRB_K_TILE = 1, FRB_K_ROW = 2, FRB_K_QUOT = 3 };
enum FrBaryBuf { FRB_BUF_NONE = -1, FRB_BUF_REC = 0, FRB_BUF_ROWREC = 1 };
enum FrBaryOrder { FRB_NATURAL = 0, FRB_BITREV = 1 };

struct FrBaryShape { int block = FRB_BLOCK, chunk = FRB_CHUNK; };

// dynamic LDS of ROWS / TILE: a lane's chunk is chunk * 8 words + 4 words of padding (fr_scan.hip.h: frs_lds_addr), one y per lane,
// one record per wavefront; of ROW: the wavefront records alone; QUOT uses none
constexpr size_t frb_lds_bytes(FrBaryShape s) { return ((size_t)s.block * (s.chunk * 8 + 4) + (size_t)s.block * 8 + (size_t)(s.block / 64) * FRB_WREC_WORDS) * 4; }
constexpr size_t frb_row_lds_bytes(FrBaryShape s) { return (size_t)(s.block / 64) * FRB_WREC_WORDS * 4; }

struct FrBaryStep {
  int kernel;                  // FrBaryKernel
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS
  int src, dst;                // FrBaryBuf: records read / written (NONE: the caller's arrays alone)
};
struct FrBaryPlan {
  int n_steps = 0;             // -1: the shape cannot hold this call
  FrBaryStep step[3];
  size_t total = 0, tile = 0;
  size_t recs[2] = {0, 0};     // records each FrBaryBuf must hold
};

inline FrBaryPlan fr_bary_plan(int log_n, size_t k, bool open, FrBaryShape s = FrBaryShape()) {
  FrBaryPlan p;
  const size_t tile = (size_t)s.block * s.chunk, n = (size_t)1 << log_n;
  p.tile = tile;
  if (s.block < 64 || s.block % 64 || s.chunk < 1 || s.chunk > 8 || (s.chunk & (s.chunk - 1)) || (s.block & (s.block - 1)) || log_n < 0 || log_n > 28 ||
      k > (FRB_MAX_TOTAL >> log_n)) { p.n_steps = -1; return p; }
  if (!k) return p;
  const size_t total = k << log_n;
  p.total = total;
  const unsigned b = (unsigned)s.block;
  if (n <= tile) {
    p.step[p.n_steps++] = FrBaryStep{FRB_K_ROWS, (unsigned)((total + tile - 1) / tile), b, frb_lds_bytes(s), FRB_BUF_NONE, FRB_BUF_NONE};
    return p;
  }
  const size_t t0 = total / tile;
  p.recs[FRB_BUF_REC] = t0;
  p.recs[FRB_BUF_ROWREC] = k;
  p.step[p.n_steps++] = FrBaryStep{FRB_K_TILE, (unsigned)t0, b, frb_lds_bytes(s), FRB_BUF_NONE, FRB_BUF_REC};
  p.step[p.n_steps++] = FrBaryStep{FRB_K_ROW, (unsigned)k, b, frb_row_lds_bytes(s), FRB_BUF_REC, FRB_BUF_ROWREC};
  if (open) p.step[p.n_steps++] = FrBaryStep{FRB_K_QUOT, (unsigned)t0, b, 0, FRB_BUF_ROWREC, FRB_BUF_NONE};
  return p;
}

}  // namespace bls
