// fr_frac_plan.h -- the launch plan of the Fr fraction scans (blsgpu_fr_grand_product*, blsgpu_fr_frac_sum*) as plain host code: which
// kernels run, in which order, with which grid / block / dynamic LDS, on which buffers.  No HIP calls here: api_fr.hip walks the plan
// and launches, tests/simt/emu_fr_frac.cpp walks the same plan on the host, tests/cpp/fr_frac_plan_main.cpp sweeps it under sanitizers.
//
// A call is fr_scan_plan.h's reduce-then-scan with ONE change: the first pass over the elements is k_frf_front (fr_frac.hip.h), which
// builds f[i] from the column sets, writes it to `out` and leaves the records k_frs_tile's REDUCE mode leaves.  Everything behind it is
// the scan's own: k_frs_agg on the aggregates, k_frs_tile<PRODUCT | SUM> in SCAN mode on `out` in place.
//
//   total <= tile                       FRONT(single)                                     one launch
//   tiles <= tile                       FRONT(reduce)   AGG_SCAN                SCAN
//   otherwise                           FRONT(reduce)   AGG_REDUCE  AGG_SCAN(top)  AGG_SCAN(carry)  SCAN
//
// The tile.  A lane keeps, for each of its `chunk` elements, the running numerator, the running denominator product and one factor in
// registers (24 VGPRs per element) and the column tables pass one at a time through ONE tile-sized LDS buffer, so neither grows with c:
// frac_sum carries sum_j m_j / d_j as the pair (S, P) with S <- S d_j + m_j P, P <- P d_j, the same shape as the grand product's (N, D).
// What grows with c is the work a tile does before and after its one inversion -- 3 c + 3 products per element -- so frf_shape() takes
// fewer elements per lane as c grows only where that keeps the lanes' share close to the inversion's cost; four elements per lane
// (96 VGPRs of state, 36 KB of LDS, two workgroups per CU with room to spare) up to c = 4, two above.
#pragma once
#include "fr_scan_plan.h"

namespace bls {

enum FrFracOp { FRF_GRAND_PRODUCT = 0, FRF_FRAC_SUM = 1 };
constexpr int FRF_MAX_COLS = 8;                   // c lies in [1, FRF_MAX_COLS]
constexpr int FRF_CHUNK_MAX = 4;                  // k_frf_front keeps a chunk's state in registers
constexpr size_t FRF_LDS_LIMIT = 80 * 1024;       // two workgroups per CU of 160 KB
constexpr int FRF_K_FRONT = 6;                    // the step kind next to FrScanKernel's: FrScanStep::src holds the front's mode (FRS_K_SINGLE / FRS_K_REDUCE)

// the scan operation behind a fraction operation
constexpr int frf_scan_op(int op) { return op == FRF_GRAND_PRODUCT ? FRS_PRODUCT : FRS_SUM; }

// the tile of (op, c): the shape of the front kernel AND of the scan passes behind it (they share the lane records)
inline FrScanShape frf_shape(int op, int c) {
  FrScanShape s;
  s.block = FRS_BLOCK;
  s.chunk = (op == FRF_FRAC_SUM && c > 4) ? 2 : 4;
  return s;
}

struct FrFracPlan {
  int n_steps = 0;             // -1: refused (c or the operation out of range, a size out of range, a shape that cannot hold the total)
  FrScanStep step[5];          // step[0] is the front (kernel = FRF_K_FRONT, src = its mode), the rest are fr_scan_plan's
  FrScanShape shape;
  size_t total = 0, tile = 0;
  size_t recs[5] = {0, 0, 0, 0, 0};       // records each FrScanBuf must hold (frs_rec_words(frf_scan_op(op)) u32 each; carries eight)
  size_t table_reach = 0;      // scalars the call reads behind each column set's base pointer: (c - 1) * pitch + total
};

// pitch: scalars between consecutive tables of a set (>= k * len).  Sizes: k * len and (c - 1) * pitch + k * len at most 2^28.
inline FrFracPlan fr_frac_plan(int op, int c, size_t len, size_t k, size_t pitch, FrScanShape s) {
  FrFracPlan p;
  p.shape = s;
  p.tile = (size_t)s.block * s.chunk;
  const auto refuse = [&p] { p.n_steps = -1; return p; };
  if ((op != FRF_GRAND_PRODUCT && op != FRF_FRAC_SUM) || c < 1 || c > FRF_MAX_COLS) return refuse();
  if (s.block < 64 || s.block % 64 || s.chunk < 1 || s.chunk > FRF_CHUNK_MAX || frs_lds_bytes(s) > FRF_LDS_LIMIT) return refuse();
  if (!len || !k) return p;
  if (k > FRS_MAX_TOTAL / len) return refuse();                   // also the 64-bit overflow of k * len
  const size_t total = len * k;
  if (pitch < total || pitch > FRS_MAX_TOTAL || (size_t)(c - 1) * pitch + total > FRS_MAX_TOTAL) return refuse();
  const FrScanPlan sp = fr_scan_plan(len, k, s);
  if (sp.n_steps < 0) return refuse();
  p.total = total;
  p.table_reach = (size_t)(c - 1) * pitch + total;
  p.n_steps = sp.n_steps;
  for (int i = 0; i < sp.n_steps; i++) p.step[i] = sp.step[i];
  for (int i = 0; i < 5; i++) p.recs[i] = sp.recs[i];
  p.step[0].src = p.step[0].kernel;                               // FRS_K_SINGLE or FRS_K_REDUCE
  p.step[0].kernel = FRF_K_FRONT;
  return p;
}
inline FrFracPlan fr_frac_plan(int op, int c, size_t len, size_t k, size_t pitch) {
  if (c < 1 || c > FRF_MAX_COLS) { FrFracPlan p; p.n_steps = -1; return p; }
  return fr_frac_plan(op, c, len, k, pitch, frf_shape(op, c));
}

}  // namespace bls
