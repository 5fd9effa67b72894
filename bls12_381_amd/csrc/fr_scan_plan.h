// fr_scan_plan.h -- the launch plan of the Fr scans (blsgpu_fr_scan_many*) and of the batch inversion (blsgpu_fr_batch_invert*) as plain
// host code: which kernels of fr_scan.hip.h run, in which order, with which grid / block / dynamic LDS, on which buffers.  No HIP calls
// here: api_fr.hip walks the plan and launches, tests/simt/emu_fr_scan.cpp walks the same plan on the host -- with a small tile and
// chunk, so that the multi-tile and aggregate-level paths are reached at a few hundred elements.
//
// The k x len array is ONE flat sequence of `total` = k len elements with segment heads at the multiples of len.  A tile is `block` lanes
// x `chunk` consecutive elements.  Reduce-then-scan, every step a launch of its own on the stream (no workgroup ever waits for another):
//
//   total <= tile                       SINGLE                                     one launch, carry-in = the identity
//   tiles <= tile                       REDUCE   AGG_SCAN            SCAN          aggregates of the tiles, scanned by ONE workgroup
//   otherwise                           REDUCE   AGG_REDUCE  AGG_SCAN(top)  AGG_SCAN(carry)  SCAN
//                                                                                  a second level: aggregates of tile-many aggregates
// Two levels cover tile^3 elements; with the shipped tile of 2048 that is 2^33, far beyond the 2^28 the entry points admit, and the plan
// refuses (n_steps = -1) a shape whose parameters do not reach (only a test can ask for one).
//
// Buffers: DATA_IN / DATA_OUT are the caller's; AGG0 holds one aggregate record per tile, AGG1 one per group of `tile` tiles (REDUCE /
// AGG_REDUCE write them); CARRY0 / CARRY1 hold the exclusive scan of AGG0 / AGG1 (AGG_SCAN writes them), i.e. what precedes each tile
// (group) in its row; LANE holds, for every lane of every tile, the aggregate of what precedes the lane's chunk inside its tile (REDUCE
// writes it, SCAN reads it: the scan pass then costs one product per element).  A record is frs_rec_words(op) u32, a carry eight.
//
// The batch inversion is one launch of k_frs_invert per call: tiles are independent (each inverts its own total).
#pragma once
#include <stddef.h>

namespace bls {

constexpr int FRS_BLOCK = 256;                    // lanes per workgroup (a multiple of 64: the wavefront scan uses whole wavefronts)
constexpr int FRS_CHUNK = 8;                      // consecutive elements a lane owns
constexpr int FRS_CHUNK_MAX = 8;                  // k_frs_invert keeps a chunk's prefix products in registers
constexpr int FRS_REC_WORDS = 20;                 // the widest aggregate record (HORNER): value (8), multiplier (8), crossed-a-head flag (1), padding to 16 bytes (3)
enum FrScanOp { FRS_SUM = 0, FRS_PRODUCT = 1, FRS_HORNER = 2 };
// words of a record in global memory: SUM and PRODUCT carry no multiplier -- value (8), flag (1), padding (3)
constexpr int frs_rec_words(int op) { return op == FRS_HORNER ? FRS_REC_WORDS : 12; }
constexpr size_t FRS_MAX_TOTAL = (size_t)1 << 28;

enum FrScanKernel { FRS_K_SINGLE = 0, FRS_K_REDUCE = 1, FRS_K_AGG_REDUCE = 2, FRS_K_AGG_SCAN = 3, FRS_K_SCAN = 4, FRS_K_INVERT = 5 };
enum FrScanBuf { FRS_BUF_NONE = -1, FRS_BUF_AGG0 = 0, FRS_BUF_AGG1 = 1, FRS_BUF_CARRY0 = 2, FRS_BUF_CARRY1 = 3, FRS_BUF_LANE = 4 };

struct FrScanShape { int block = FRS_BLOCK, chunk = FRS_CHUNK; };

// dynamic LDS of the element kernels: a lane's chunk is chunk * 8 words + 4 words of padding (fr_scan.hip.h: frs_lds_addr), then one
// aggregate record per wavefront
constexpr size_t frs_lds_bytes(FrScanShape s) { return ((size_t)s.block * (s.chunk * 8 + 4) + (size_t)(s.block / 64) * FRS_REC_WORDS) * 4; }
constexpr size_t frs_agg_lds_bytes(FrScanShape s) { return (size_t)(s.block / 64) * FRS_REC_WORDS * 4; }

struct FrScanStep {
  int kernel;                  // FrScanKernel
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS
  size_t items;                // elements (SINGLE / REDUCE / SCAN / INVERT) or aggregate records (AGG_*) the launch covers
  int src, dst, carry;         // FrScanBuf: aggregates read / records written / carries read (NONE: the identity); element kernels read and write the data
};
struct FrScanPlan {
  int n_steps = 0;             // -1: the shape cannot hold this total
  FrScanStep step[5];
  size_t total = 0, tile = 0;
  size_t recs[5] = {0, 0, 0, 0, 0};       // records each FrScanBuf must hold
};

inline FrScanPlan fr_scan_plan(size_t len, size_t k, FrScanShape s = FrScanShape()) {
  FrScanPlan p;
  const size_t tile = (size_t)s.block * s.chunk;
  p.tile = tile;
  if (!len || !k) return p;
  const size_t total = len * k;
  p.total = total;
  const size_t t0 = (total + tile - 1) / tile;      // tiles
  const size_t lds = frs_lds_bytes(s), alds = frs_agg_lds_bytes(s);
  const unsigned b = (unsigned)s.block;
  if (t0 == 1) { p.step[p.n_steps++] = FrScanStep{FRS_K_SINGLE, 1, b, lds, total, FRS_BUF_NONE, FRS_BUF_NONE, FRS_BUF_NONE}; return p; }
  p.recs[FRS_BUF_AGG0] = p.recs[FRS_BUF_CARRY0] = t0;
  p.recs[FRS_BUF_LANE] = t0 * s.block;              // REDUCE writes one record per lane, SCAN reads it back
  p.step[p.n_steps++] = FrScanStep{FRS_K_REDUCE, (unsigned)t0, b, lds, total, FRS_BUF_NONE, FRS_BUF_AGG0, FRS_BUF_NONE};
  if (t0 <= tile) {
    p.step[p.n_steps++] = FrScanStep{FRS_K_AGG_SCAN, 1, b, alds, t0, FRS_BUF_AGG0, FRS_BUF_CARRY0, FRS_BUF_NONE};
  } else {
    const size_t t1 = (t0 + tile - 1) / tile;
    if (t1 > tile) { p.n_steps = -1; return p; }
    p.recs[FRS_BUF_AGG1] = p.recs[FRS_BUF_CARRY1] = t1;
    p.step[p.n_steps++] = FrScanStep{FRS_K_AGG_REDUCE, (unsigned)t1, b, alds, t0, FRS_BUF_AGG0, FRS_BUF_AGG1, FRS_BUF_NONE};
    p.step[p.n_steps++] = FrScanStep{FRS_K_AGG_SCAN, 1, b, alds, t1, FRS_BUF_AGG1, FRS_BUF_CARRY1, FRS_BUF_NONE};
    p.step[p.n_steps++] = FrScanStep{FRS_K_AGG_SCAN, (unsigned)t1, b, alds, t0, FRS_BUF_AGG0, FRS_BUF_CARRY0, FRS_BUF_CARRY1};
  }
  p.step[p.n_steps++] = FrScanStep{FRS_K_SCAN, (unsigned)t0, b, lds, total, FRS_BUF_NONE, FRS_BUF_NONE, FRS_BUF_CARRY0};
  return p;
}

// the batch inversion: one launch, a tile per workgroup (chunk <= FRS_CHUNK_MAX)
inline FrScanPlan fr_invert_plan(size_t n, FrScanShape s = FrScanShape()) {
  FrScanPlan p;
  const size_t tile = (size_t)s.block * s.chunk;
  p.tile = tile; p.total = n;
  if (!n) return p;
  if (s.chunk > FRS_CHUNK_MAX) { p.n_steps = -1; return p; }
  p.step[p.n_steps++] = FrScanStep{FRS_K_INVERT, (unsigned)((n + tile - 1) / tile), (unsigned)s.block, frs_lds_bytes(s), n, FRS_BUF_NONE, FRS_BUF_NONE, FRS_BUF_NONE};
  return p;
}

}  // namespace bls
