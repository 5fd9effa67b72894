// fr_spmv.hip.h -- sparse matrix-vector products over Fr (blsgpu_fr_spmv*): out[v][i] = sum_{p in [row_ptr[i], row_ptr[i+1])} val[p] x[v][col[p]]
// for a resident CSR matrix (blsgpu_fr_matrix) and k right-hand sides.  fr_spmv_plan.h decides the launches and names the records.
//
// The schedule.  The non-zeros are one flat sequence with a row end wherever row_ptr says so, cut into tiles of blockDim.x lanes x
// `chunk` consecutive entries -- the scans' tiling (fr_scan.hip.h), with the rows as segments of unequal length.  k_frsp_tile stages the
// tile's values (16-byte words, consecutive lanes on consecutive words, frs_tile_load) and column indices in LDS ONCE and then, for
// every right-hand side in turn, lets each lane walk its chunk: gather x[col], one product per entry, a running sum that is closed at
// every row end.  A row that begins and ends inside the lane's chunk is written at once.  What a lane cannot finish alone -- the sum
// up to its first row end (`lead`) and the sum behind its last one -- goes through the SUM monoid of the scans: the lane's aggregate is
// (sum behind the last row end, "a row ended here"), frs_block_scan<FRS_SUM> gives every lane the open sum in front of its chunk, and
// the lane that holds a row's LAST entry writes the row -- unless the row began in an earlier tile, then the sum is the tile's HEAD
// record; the last lane leaves the TAIL record of a row that goes on.  k_frsp_fixup adds TAIL + HEAD + ... + HEAD per crossing row.
// No atomics, no workgroup waiting for another: every output is the same sum in the same order from run to run.
//
// Which row a lane starts in is a binary search of row_ptr between the first rows of this tile and the next one (tile_row, found once
// at upload: k_frsp_prepare); at a row end the next row is row + 1, or a second search when that one is empty, so a run of empty rows
// costs a logarithm and not its length.  Empty rows are written by nobody here: the plan zeroes `out` first when the matrix has one.
//
// Arithmetic: the lazy 9 x 29-bit limbs of fr.hip.h, bounds in that file's notation ("A": limbs < A 2^29, "V": value < V r).
//   resident val'  = 2^5 val mod r, canonical (folded once at upload, as the transform folds it into its twiddles)       A1 V1
//   x[col]           canonical (precondition of every Fr entry point)                                                    A1 V1
//   product          frl_mul(x, val') = x val 2^5 / 2^261 = x val / 2^256: the reference's Montgomery product            A1 V2
//   running sum      starts at 0 or at a reduced sum (A1 V2) and takes at most FRSP_LAZY = 3 products                 <= A4 V8
//                    -> frl_reduce (needs A <= 4, V <= 8)                                                                A1 V2
//   row end / chunk end: frl_reduce (the sum holds at most A1 V2 + 2 products = A3 V6), frl_canon                        canonical
// Sums ACROSS lanes and tiles are canonical fr_add (scalar.hip.h): a handful per lane against `chunk` products.
#pragma once
#include "fr.hip.h"
#include "fr_scan.hip.h"
#include "fr_spmv_plan.h"

namespace bls {

constexpr int FRSP_LAZY = 3;                         // products added to a reduced sum before the next frl_reduce
static_assert(1 + FRSP_LAZY <= 4 && 2 + 2 * FRSP_LAZY <= 8, "A1 V2 + FRSP_LAZY x A1 V2 must stay within frl_reduce's A <= 4, V <= 8");
static_assert(FRSP_BLOCK % 64 == 0, "the block scan and the fix-up work on whole wavefronts");

// the product (ONE call site, inside the entry loop: inlined, so no limb goes through the stack) and the closing reduction
DEV FrL frsp_mul(const FrL& x, const FrL& v) { return frl_mul(x, v); }
DEV Fr frsp_close(const FrL& acc) { return frl_canon(frl_reduce(acc)); }      // acc <= A4 V8 -> canonical
DEV FrL frl_zero() { FrL r; for (int i = 0; i < 9; i++) r.l[i] = 0; return r; }

// the largest i in [lo, hi] with row_ptr[i] <= p (row_ptr[lo] <= p is given): the row that holds entry p when row_ptr[hi + 1] > p --
// empty rows share their start with the next non-empty one and are skipped
DEV u32 frsp_row_of(const u32* __restrict__ row_ptr, u32 lo, u32 hi, u32 p) {
  while (lo < hi) {
    const u32 mid = lo + (hi - lo + 1) / 2;
    if (row_ptr[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- upload: validation and the resident form ---------------------------------------------------------------------------------------
// flag[0] |= 1: row_ptr decreases somewhere, 2: a column index >= n_cols, 4: a value's limbs are not below r, 8: row_ptr[0] != 0.
// nnz = row_ptr[n_rows] as the host read it (and bounded it) before the launch: col and val are read below nnz only.
__global__ void __launch_bounds__(256) k_frsp_validate(const u32* __restrict__ row_ptr, const u32* __restrict__ col, const u32* __restrict__ val, size_t n_rows, size_t n_cols,
                                                       size_t nnz, u32* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u32 f = 0;
  if (i == 0 && row_ptr[0] != 0) f |= 8u;
  if (i < n_rows && row_ptr[i] > row_ptr[i + 1]) f |= 1u;
  if (i < nnz) {
    if (col[i] >= n_cols) f |= 2u;
    if (!fr_words_below_r(val + i * 8)) f |= 4u;
  }
  if (f) atomicOr(flag, f);
}
// val_out[p] = 2^5 val_in[p] (val_in == val_out allowed: a lane reads its own element before it writes it); tile_row[t] = the row of
// entry t * tile for t < tiles, tile_row[tiles] = n_rows - 1; flag[1] |= 1 when a row is empty.  For a VALIDATED matrix.
__global__ void __launch_bounds__(256) k_frsp_prepare(const u32* __restrict__ row_ptr, const u32* val_in, u32* val_out, u32* __restrict__ tile_row, u32* flag, size_t n_rows,
                                                      size_t nnz, size_t tiles, unsigned tile) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz) {
    Fr v = fr_load(val_in + i * 8);
    for (int s = 0; s < 5; s++) v = fr_add(v, v);
    fr_store(val_out + i * 8, v);
  }
  if (i < n_rows && row_ptr[i] == row_ptr[i + 1]) atomicOr(flag + 1, 1u);
  if (i < tiles) tile_row[i] = frsp_row_of(row_ptr, 0, (u32)(n_rows - 1), (u32)(i * tile));
  if (i == tiles) tile_row[i] = (u32)(n_rows - 1);
}

// ---- a tile of non-zeros, all right-hand sides -------------------------------------------------------------------------------------
// val: the resident values (2^5 val), col, row_ptr, tile_row: the resident matrix; x: k x n_cols, out: k x n_rows; head / tail: one
// scalar per (tile, vector) at (tile * k + v) * 8; meta: one word per tile (fr_spmv_plan.h).  x and out do not overlap (the entry point
// refuses that), so the gather never reads what another workgroup writes.
__global__ void __launch_bounds__(FRSP_BLOCK, 2) k_frsp_tile(const u32* __restrict__ row_ptr, const u32* __restrict__ col, const u32* __restrict__ val,
                                                              const u32* __restrict__ tile_row, size_t n_rows, size_t n_cols, size_t nnz, const u32* __restrict__ x,
                                                              u32* __restrict__ out, size_t k, unsigned chunk, u32* __restrict__ head, u32* __restrict__ tail,
                                                              u32* __restrict__ meta) {
  BLS_DYN_LDS(lds);
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= nnz) return;
  const unsigned cnt = nnz - base < (size_t)tile ? (unsigned)(nnz - base) : tile;
  u32* lcol = lds + blockDim.x * (chunk * 8 + 4);
  u32* wrec = lcol + tile;
  frs_tile_load<false>(val, base, cnt, nnz, chunk, lds);
  for (unsigned i = threadIdx.x; i < cnt; i += blockDim.x) lcol[i] = col[base + i];
  __syncthreads();
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;
  const u32 p0 = (u32)base + s0;                                  // nnz <= 2^28: positions fit a word
  const u32 row_hi = tile_row[blockIdx.x + 1];                    // no entry of this tile lies in a later row
  u32 row0 = 0, start0 = 0, end0 = 0;
  if (mine) {
    row0 = frsp_row_of(row_ptr, tile_row[blockIdx.x], row_hi, p0);
    start0 = row_ptr[row0];
    end0 = row_ptr[row0 + 1];
  }
  const bool last_lane = threadIdx.x == (cnt - 1) / chunk;        // holds the tile's last entry
#pragma unroll 1
  for (size_t v = 0; v < k; v++) {
    const u32* xv = x + v * n_cols * 8;
    u32* ov = out + v * n_rows * 8;
    FrL acc = frl_zero();
    int lazy = 0;
    Fr lead = fr_zero();                                          // the sum up to the chunk's first row end: row0's, and it needs what precedes the chunk
    bool lead_closed = false, open = false;                       // open: the chunk's last entry does not end its row
    u32 row = row0, end = end0;
    FrsAgg a = frs_identity<FRS_SUM>();                           // (the sum behind the chunk's last row end, a row ended in the chunk)
#pragma unroll 1
    for (unsigned j = 0; j < mine; j++) {
      const FrL prod = frsp_mul(frl_load(xv + (size_t)lcol[s0 + j] * 8), frl_load(lds + frs_lds_addr(s0 + j, chunk)));      // A1 V2
      acc = frl_add(acc, prod);
      if (++lazy == FRSP_LAZY) { acc = frl_reduce(acc); lazy = 0; }      // <= A4 V8 -> A1 V2
      open = p0 + j + 1 != end;
      if (!open) {                                                // entry p0 + j is the last one of `row`
        const Fr s = frsp_close(acc);
        if (!a.f) { lead = s; lead_closed = true; }
        else fr_store(ov + (size_t)row * 8, s);                   // the row began behind an earlier row end of this chunk: it is complete
        a.f = 1;
        acc = frl_zero(); lazy = 0;
        if (j + 1 < mine) {                                       // the row of entry p0 + j + 1 (it exists and lies in this tile)
          row++;
          if (row_ptr[row + 1] == end) row = frsp_row_of(row_ptr, row, row_hi, end);
          end = row_ptr[row + 1];
        }
      }
    }
    a.v = frsp_close(acc);
    const FrsAgg before = frs_block_scan<FRS_SUM>(a, wrec);       // before.v: the open sum in front of the chunk (since the tile's last row end, or its start)
    const size_t rec = ((size_t)blockIdx.x * k + v) * 8;
    if (lead_closed) {
      const Fr t = fr_add(before.v, lead);
      if (start0 >= base) fr_store(ov + (size_t)row0 * 8, t);     // row0 began in this tile: complete
      else fr_store(head + rec, t);                               // ... in an earlier one: this is the tile's first row end
    }
    if (last_lane) {
      u32 m = 0;
      if (open) {
        const Fr t = a.f ? a.v : fr_add(before.v, a.v);
        if (row_ptr[row] >= base) { fr_store(tail + rec, t); m = row + 1; }
        else fr_store(head + rec, t);                             // no row end in the whole tile: it lies inside one row
      }
      if (v == 0) meta[blockIdx.x] = m;
    }
  }
}

// ---- rows that cross tiles ------------------------------------------------------------------------------------------------------------
// One wavefront per tile t with meta[t] = row + 1: the row began in t and ends in tile t_end > t (where its last entry lies), every tile
// between them lies inside the row, so  out[row] = TAIL[t] + HEAD[t + 1] + ... + HEAD[t_end].  The lanes take the HEAD records in
// turn and add up across the wavefront; tile: entries per tile.
__global__ void __launch_bounds__(FRSP_BLOCK) k_frsp_fixup(const u32* __restrict__ row_ptr, const u32* __restrict__ head, const u32* __restrict__ tail,
                                                           const u32* __restrict__ meta, size_t tiles, size_t n_rows, size_t k, unsigned tile, u32* __restrict__ out) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t t = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (t >= tiles) return;
  const u32 m = meta[t];
  if (!m) return;
  const u32 row = m - 1;
  const size_t t_end = (row_ptr[row + 1] - 1) / tile;
#pragma unroll 1
  for (size_t v = 0; v < k; v++) {
    Fr s = fr_zero();
#pragma unroll 1
    for (size_t u = t + 1 + lane; u <= t_end && u < tiles; u += 64) s = fr_add(s, fr_load(head + (u * k + v) * 8));
#pragma unroll 1
    for (unsigned d = 32; d; d >>= 1) s = fr_add(s, frs_shfl(s, d, true));      // lane 0 ends with the sum of all 64 (the others' values are unused)
    if (lane == 0) fr_store(out + (v * n_rows + row) * 8, fr_add(s, fr_load(tail + (t * k + v) * 8)));
  }
}

}  // namespace bls
