// tests/simt/emu_kzg.cpp -- the data-movement kernels of bls12_381_amd/csrc/kzg.hip.h compiled for the HOST (test infrastructure only).
// Every entry point below is ONE stage of blsgpu_kzg_multiproof_create / _proofs_device / blsgpu_kzg_cells_device, launched with the
// grids of csrc/kzg_plan.h -- the functions api_msm.hip launches from -- at whatever transposition tile the test asks for (4, or 0 for
// the shipped KZG_TILE).  The transforms and the MSM between the stages are the test's (tests/kzg_ref.py, in Python integers).
//
// Over tests/simt/emu_harness.h: every launch runs its block on one host thread per lane, the library is built with the trapping
// bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the tests call this library from a
// child process (tests/simt_kzg_child.py).  -DKZG_FAULT=n builds the kernels with one of their seeded faults (tests/test_simt_kzg.py).
#define EMU_LANES 256
#include "emu_harness.h"

#include "kzg.hip.h"

using namespace bls;

namespace {

template <int T> void transpose(const KzgTranspose& tp, const uint4* in, uint4* out, size_t vecs, int log_r, int log_cc, int brev) {
  launch_threads(tp.grid, tp.block, [=] { k_kzg_transpose<T>(in, out, vecs, log_r, log_cc, brev); });
}
int run_transpose(const KzgTranspose& tp, const uint4* in, uint4* out, size_t vecs, int log_r, int log_cc, int brev) {
  if (tp.tile == 4) transpose<4>(tp, in, out, vecs, log_r, log_cc, brev);
  else if (tp.tile == KZG_TILE) transpose<KZG_TILE>(tp, in, out, vecs, log_r, log_cc, brev);
  else return -1;
  return 0;
}
unsigned tile_of(int tile) { return tile ? (unsigned)tile : (unsigned)KZG_TILE; }

}  // namespace

extern "C" {

// info: ok, msm, scalars, points, vectors, coeff_bytes, rows_bytes, seg_bytes, point_bytes, offset_bytes, base_first_bytes, transpose grid, transpose block
void emu_kzg_plan(int log_n, int log_l, size_t count, int form, int tile, size_t* info) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, form, tile_of(tile));
  const size_t v[13] = {(size_t)p.ok, (size_t)p.msm, (size_t)p.scalars, (size_t)p.points, (size_t)p.vectors, p.coeff_bytes, p.rows_bytes, p.seg_bytes, p.point_bytes, p.offset_bytes,
                        p.base_first_bytes, p.transpose.grid, p.transpose.block};
  for (int i = 0; i < 13; i++) info[i] = v[i];
}
// create: the SRS prefix (n affine wire points + flags) -> S^ [t][j] (2n projective wire points)
int emu_kzg_srs_rows(const void* xy, const uint8_t* inf, void* out, int log_n, int log_l) {
  const KzgCreatePlan p = kzg_plan_create(log_n, log_l);
  if (!p.ok || !p.msm) return -1;
  launch_loop(p.gather_grid, KZG_BLOCK, [=] { k_kzg_srs_rows((const uint4*)xy, inf, (uint4*)out, p.log_c, log_l); });
  return 0;
}
// create: [t][m] -> [m][t] over 2n points
int emu_kzg_srs_transpose(const void* in, void* out, int log_n, int log_l) {
  const KzgCreatePlan p = kzg_plan_create(log_n, log_l);
  if (!p.ok || !p.msm) return -1;
  launch_loop(p.permute_grid, KZG_BLOCK, [=] { k_kzg_point_permute((const uint4*)in, (uint4*)out, (size_t)1, log_n + 1, 2, p.log_c, log_l); });
  return 0;
}
// the copy of an evaluation-form input (log_out = log_n) or the zero extension of the cells (log_out = log_n + 1)
int emu_kzg_copy(const void* in, void* out, size_t count, int log_n, int log_out, int brev) {
  launch_loop(kzg_grid((uint64_t)count << log_out), KZG_BLOCK, [=] { k_kzg_scalar_copy((const uint4*)in, (uint4*)out, count, log_n, log_out, brev); });
  return 0;
}
int emu_kzg_coeff_rows(const void* coeffs, void* rows, size_t count, int log_n, int log_l, int form) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, form);
  if (!p.ok || !p.msm) return -1;
  launch_loop(p.rows_grid, KZG_BLOCK, [=] { k_kzg_coeff_rows((const uint4*)coeffs, (uint4*)rows, count, p.log_c, log_l); });
  return 0;
}
// proofs: [v][t][m] -> [v][m][t]
int emu_kzg_transpose(const void* rows, void* seg, size_t count, int log_n, int log_l, int tile) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, 0, tile_of(tile));
  if (!p.ok || !p.msm) return -1;
  return run_transpose(p.transpose, (const uint4*)rows, (uint4*)seg, count, log_l, p.log_c + 1, 0);
}
int emu_kzg_segments(u32* off, u32* bf, size_t count, int log_n, int log_l) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, 0);
  if (!p.ok || !p.msm) return -1;
  launch_loop(p.seg_grid, KZG_BLOCK, [=] { k_kzg_segments(off, bf, (size_t)p.points, p.log_c, log_l); });
  return 0;
}
// the identities over the upper c of every vector (c = 1: over both points of every polynomial, the whole result)
int emu_kzg_fill(void* pts, size_t count, int log_n, int log_l) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, 0);
  if (!p.ok) return -1;
  const int log_v = p.log_c + 1;
  if (p.msm) launch_loop(p.fill_grid, KZG_BLOCK, [=] { k_kzg_identity_fill((uint4*)pts, count, log_v, (size_t)p.c, p.log_c); });
  else launch_loop(p.fill_grid, KZG_BLOCK, [=] { k_kzg_identity_fill((uint4*)pts, count, log_v, (size_t)0, log_v); });
  return 0;
}
int emu_kzg_permute(const void* pts, void* out, size_t count, int log_n, int log_l, int order) {
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, 0);
  if (!p.ok || !p.msm) return -1;
  launch_loop(p.permute_grid, KZG_BLOCK, [=] { k_kzg_point_permute((const uint4*)pts, (uint4*)out, count, p.log_c + 1, order == KZG_ORDER_BITREV ? 1 : 0, p.log_c, log_l); });
  return 0;
}
// cells: the tiled map E -> cells
int emu_kzg_cells_map(const void* ext, void* cells, size_t count, int log_n, int log_l, int order, int tile) {
  const KzgCellsPlan p = kzg_plan_cells(log_n, log_l, count, 0, tile_of(tile));
  if (!p.ok || !count) return -1;
  return run_transpose(p.map, (const uint4*)ext, (uint4*)cells, count, log_l, p.log_c + 1, order == KZG_ORDER_BITREV ? 1 : 0);
}
}
