// tests/simt/emu_fr_spmv.cpp -- the sparse matrix-vector product kernels of bls12_381_amd/csrc/fr_spmv.hip.h compiled for the HOST (test
// infrastructure only).  emu_fr_spmv WALKS THE PLAN of csrc/fr_spmv_plan.h -- the function api_fr.hip launches from -- step by step,
// with its grids, blocks, LDS sizes and record sizes, at whatever (block, chunk) the test asks for: with a tile of 64 x 2 entries a row
// of 300 non-zeros already spans three tiles.  emu_fr_spmv_prepare / emu_fr_spmv_validate run the two upload kernels.
//
// The tile kernel scans across lanes with __shfl_up and meets at the workgroup barrier, the fix-up adds across a wavefront with
// __shfl_down, so every launch runs its block on one host thread per lane (the lane pool of tests/simt/emu_harness.h).
//
// Built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_spmv_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * (8 * 8 + 4) + 256 * 8 + 4 * 20)      // frsp_lds_words of the shipped shape
#include "emu_harness.h"
#include <string.h>

#include "fr_spmv.hip.h"
static_assert(EMU_DYN_LDS_WORDS >= bls::frsp_lds_words(bls::FrSpmvShape()), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");

using namespace bls;

namespace {

FrSpmvShape shape_of(int block, int chunk) { FrSpmvShape s; s.block = block; s.chunk = chunk; return s; }

}  // namespace

extern "C" {

// sizes[0] = tiles, [1] = scalars each of HEAD and TAIL must hold, [2] = words of META; returns the number of steps of the plan
int emu_fr_spmv_sizes(size_t n_rows, size_t nnz, size_t k, int has_empty, int block, int chunk, size_t* sizes) {
  if (!shape_ok(block, chunk)) return -1;
  const FrSpmvPlan plan = fr_spmv_plan(n_rows, nnz, k, has_empty != 0, shape_of(block, chunk));
  sizes[0] = frsp_tiles(nnz, shape_of(block, chunk)); sizes[1] = plan.rec_scalars; sizes[2] = plan.meta_words;
  return plan.n_steps;
}
// flag: one word, zero on entry
void emu_fr_spmv_validate(const u32* row_ptr, const u32* col, const u32* val, size_t n_rows, size_t n_cols, size_t nnz, u32* flag) {
  const size_t span = nnz > n_rows ? nnz : n_rows;
  launch_threads((unsigned)((span + 255) / 256), 256, [=] { k_frsp_validate(row_ptr, col, val, n_rows, n_cols, nnz, flag); });
}
// val_out: nnz scalars; tile_row: tiles + 1 words; flag: two words, zero on entry (flag[1]: a row is empty)
int emu_fr_spmv_prepare(const u32* row_ptr, const u32* val_in, u32* val_out, u32* tile_row, u32* flag, size_t n_rows, size_t nnz, int block, int chunk) {
  if (!shape_ok(block, chunk) || !n_rows) return -1;
  const size_t tiles = frsp_tiles(nnz, shape_of(block, chunk));
  size_t span = nnz > n_rows ? nnz : n_rows;
  if (tiles + 1 > span) span = tiles + 1;
  launch_threads((unsigned)((span + 255) / 256), 256, [=] { k_frsp_prepare(row_ptr, val_in, val_out, tile_row, flag, n_rows, nnz, tiles, (unsigned)(block * chunk)); });
  return 0;
}
// the prepared matrix (val = what emu_fr_spmv_prepare wrote) times x (k x n_cols scalars) -> out (k x n_rows scalars); head / tail:
// sizes[1] scalars each, meta: sizes[2] words.  kernels_out: the FrSpmvKernel of every step, -1 ends it (at least 4 ints).  Returns the
// number of steps, or -1.
int emu_fr_spmv(const u32* row_ptr, const u32* col, const u32* val, const u32* tile_row, size_t n_rows, size_t n_cols, size_t nnz, int has_empty, const u32* x, u32* out, size_t k,
                int block, int chunk, u32* head, u32* tail, u32* meta, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  const FrSpmvPlan plan = fr_spmv_plan(n_rows, nnz, k, has_empty != 0, shape_of(block, chunk));
  for (int i = 0; i < plan.n_steps; i++) {
    const FrSpmvStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    kernels_out[i] = s.kernel;
    switch (s.kernel) {
      case FRSP_K_FILL:
        memset(out, 0, s.items * 32);
        break;
      case FRSP_K_TILE:
        launch_threads(s.grid, s.block, [=] { k_frsp_tile(row_ptr, col, val, tile_row, n_rows, n_cols, nnz, x, out, k, (unsigned)chunk, head, tail, meta); });
        break;
      default:
        launch_threads(s.grid, s.block, [=] { k_frsp_fixup(row_ptr, head, tail, meta, s.items, n_rows, k, (unsigned)plan.tile, out); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}
}
