// tests/simt/emu_kzg_verify.cpp -- the kernels of bls12_381_amd/csrc/kzg_verify.hip.h compiled for the HOST (test infrastructure only).
// Every entry point below is ONE stage of blsgpu_kzg_verify_cells_device (or of blsgpu_kzg_cell_verifier_create), launched with the grids
// and the fold's cut of csrc/kzg_verify_plan.h -- the function api_msm.hip launches from -- at whatever chunk the test asks for (0 for
// the automatic cut).  The inverse transforms, the point products, their sums, the MSM and the pairing between the stages are the
// test's (tests/kzg_verify_ref.py, in Python integers).
//
// Over tests/simt/emu_harness.h: the workgroup that scans the offsets runs on one host thread per lane, the one-item-per-lane kernels
// lane after lane; the library is built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an
// inaccessible page, and the tests call this library from a child process (tests/simt_kzg_verify_child.py).  -DKZGV_FAULT=n builds the
// kernels with one of their seeded faults (tests/test_simt_kzg_verify.py).
#define EMU_LANES 256
#include "emu_harness.h"

#include "convert.hip.h"
#include "kzg.hip.h"
#include "kzg_verify.hip.h"

using namespace bls;

extern "C" {

// info: ok, chunk, nchunks, bytes, then the sizes in bytes the plan leaves for eff, mis, badidx, off64, msm_off, base_first, scal, pxy, pinf, cellc, part, agg, ab, qidx, poff, bad
void emu_kzgv_plan(int log_n, int log_l, size_t m, size_t nseg, unsigned chunk, size_t* info) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, nseg, chunk);
  const size_t v[20] = {(size_t)p.ok, p.chunk, (size_t)p.nchunks, p.bytes, p.mis - p.eff, p.badidx - p.mis, p.bad - p.badidx, p.msm_off - p.off64, p.base_first - p.msm_off,
                        p.scal - p.base_first, p.pxy - p.scal, p.pinf - p.pxy, p.prod - p.pinf, p.part - p.cellc, p.agg - p.part, p.msm - p.agg, p.abxy - p.ab, p.poff - p.qidx,
                        p.gt - p.poff, p.isone - p.bad};
  for (int i = 0; i < 20; i++) info[i] = v[i];
}
void emu_kzgv_roots(u32* tab, int log_n) { launch_loop(1, 64, [=] { k_kzgv_roots(tab, log_n); }); }
int emu_kzgv_offsets(const u32* offsets, size_t nseg, size_t m, int log_n, int log_l, u32* eff, uint8_t* mis, unsigned long long* off64, u32* msm_off, u32* base_first, u32* status) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, nseg);
  if (!p.ok || !nseg) return -1;
  launch_threads(p.scan_grid, KZGV_BLOCK, [=] { k_kzgv_offsets(offsets, (u32)nseg, (u32)m, log_l, eff, mis, off64, msm_off, base_first, status); });
  return 0;
}
int emu_kzgv_weights(const u32* eff, size_t nseg, size_t m, const u32* row, const u32* col, size_t ncommit, const u32* r, const u32* tab, const void* commit_xy,
                     const uint8_t* commit_inf, const void* proof_xy, const uint8_t* proof_inf, int log_n, int log_l, int order, u32* scal, void* pxy, uint8_t* pinf, uint8_t* badidx,
                     u32* status) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, nseg);
  if (!p.ok || !m) return -1;
  launch_loop(p.weights_grid, KZGV_BLOCK, [=] {
    k_kzgv_weights(eff, (u32)nseg, (u32)m, row, col, (u32)ncommit, r, tab, (const uint2*)commit_xy, commit_inf, (const uint2*)proof_xy, proof_inf, log_n, log_l, order, scal, (uint2*)pxy,
                   pinf, badidx, status);
  });
  return 0;
}
// the cells in natural coset order (kzg.hip.h's copy, as the chain launches it)
int emu_kzgv_cell_copy(const void* cells, void* cellc, size_t m, int log_n, int log_l, int order) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, m ? 1 : 0);
  if (!p.ok || !m) return -1;
  launch_loop(p.copy_grid, KZG_BLOCK, [=] { k_kzg_scalar_copy((const uint4*)cells, (uint4*)cellc, m, log_l, log_l, order == KZGV_ORDER_BITREV ? 1 : 0); });
  return 0;
}
// both passes of the fold; part: exactly the bytes the plan leaves for it
int emu_kzgv_fold(const u32* eff, size_t nseg, size_t m, const u32* col, const u32* rho, const u32* cellc, const u32* tab, int log_n, int log_l, int order, unsigned chunk, u32* agg,
                  u32* part) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, nseg, chunk);
  if (!p.ok || !nseg) return -1;
  if (m)
    launch_loop(p.fold_grid, KZGV_BLOCK, [=] { k_kzgv_fold_chunks(eff, (u32)nseg, (u32)m, col, rho, cellc, tab, log_n, log_l, order, p.chunk, (u32)p.nchunks, agg, part); });
  launch_loop(p.combine_grid, KZGV_BLOCK, [=] { k_kzgv_fold_combine(eff, (u32)nseg, log_l, p.chunk, part, agg); });
  return 0;
}
int emu_kzgv_finish(const u32* sum, const u32* msm, const uint8_t* mis, const uint8_t* badidx, size_t nseg, int log_n, int log_l, u32* ab, u32* out_ab, u32* qidx,
                    unsigned long long* poff, uint8_t* bad, const uint8_t* isone, uint8_t* verdict) {
  const KzgvPlan p = kzgv_plan(log_n, log_l, 0, nseg);
  if (!p.ok || !nseg) return -1;
  launch_loop(p.finish_grid, KZGV_BLOCK, [=] { k_kzgv_finish(sum, msm, mis, badidx, (u32)nseg, ab, out_ab, qidx, poff, bad); });
  launch_loop(p.finish_grid, KZGV_BLOCK, [=] { k_kzgv_verdict(isone, bad, (u32)nseg, verdict); });
  return 0;
}
}
