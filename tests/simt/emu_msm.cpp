// tests/simt/emu_msm.cpp -- the MSM kernels of bls12_381_amd/csrc compiled for the HOST (test infrastructure only): the segmented MSM
// (msm_seg.hip.h), the scalar decompositions, the endomorphism images, the subgroup check and the G1 bucket accumulation of msm.hip.h.
// The entry points launch the __global__ functions themselves with the grid and block shapes of api_msm.hip (restated below, each with
// the lines it restates), every lane a host thread where lanes cooperate (tests/simt/hip/hip_runtime.h), so that the CPU suite can
// compare the very code the GPU runs with the oracle (tests/test_simt_msm.py).
//
// The lane pool, the launchers, the trapping checks and emu_guarded() are those of tests/simt/emu_harness.h; the tests call this
// library from a child process (tests/simt_msm_child.py).
#define EMU_LANES 256
#include "emu_harness.h"

#include "msm_seg.hip.h"
#include "abi_kernels.hip.h"

using namespace bls;

namespace {

// api_msm.hip msm_segments_launch (:644-661): the batch loop, accumulate -> combine -> export per batch of `batch` segments
template <class F, int MODE, class FK>
void segments(const u32* rec, const u32* endo, size_t nbases, const u32* bf, const u32* off, const u32* s, size_t k, size_t batch, size_t total, int form,
              u32* status, u32* wsums, u32* seg_rec, u32* out) {
  typedef SegCfg<FK, MODE> C;
  constexpr int WW = Wire<F>::WORDS;
  for (size_t s0 = 0; s0 < k; s0 += batch) {
    const u32 nb = (u32)(k - s0 < batch ? k - s0 : batch);
    launch_threads(nb * C::NGRP, SEG_THREADS, [=] { k_msm_seg_accumulate<FK, MODE>(rec, endo, nbases, bf, off, s, (u32)s0, (u32)total, form, status, wsums); });
    auto combine = [=] { k_msm_seg_combine<FK, C::NWIN>(wsums, seg_rec, nb); };
    if (C::LPA == 1) launch_loop(nblk((size_t)nb * C::LPA, 256), 256, combine);
    else launch_threads(nblk((size_t)nb * C::LPA, 256), 256, combine);
    launch_loop(nblk(nb, 256), 256, [=] { k_proj_export<F>(seg_rec, out + s0 * 3 * WW, (size_t)nb); });
  }
}

}  // namespace

extern "C" {

// api_msm.hip bases_import (:62), bases_make_endo (:32-33, :43-44); group 1 = G1, 2 = G2
void emu_bases_import(int group, const u32* xy, const uint8_t* inf, u32* rec, size_t n) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_bases_import<FpPolicy>(xy, inf, rec, n); });
  else launch_loop(nblk(n, 256), 256, [=] { k_bases_import<Fp2Policy>(xy, inf, rec, n); });
}
void emu_bases_endo(int group, const u32* rec, u32* endo, size_t n) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_bases_endo(rec, endo, n); });
  else launch_loop(nblk(n, 256), 256, [=] { k_bases_endo_g2(rec, endo, n); });
}
void emu_bases_subgroup_check(int group, const u32* rec, size_t n, u32* bad) {
  if (group == 1) launch_loop(nblk(n, 128), 128, [=] { k_bases_subgroup_check<FpPolicy>(rec, n, bad); });
  else launch_loop(nblk(n, 128), 128, [=] { k_bases_subgroup_check<Fp2Policy>(rec, n, bad); });
}

// split != 0: GLV (G1) / psi split (G2) over the images in `endo`; 0: plain 256-bit windows.  wsums: batch * NWIN PROJ records (the
// window sums of the LAST batch remain), seg_rec: batch PROJ records, out: k x 3 wire elements (projective)
void emu_msm_segments(int group, int split, const u32* rec, const u32* endo, size_t nbases, const u32* base_first, const u32* offsets, const u32* scalars,
                      size_t k, size_t batch, size_t total, int form, u32* status, u32* wsums, u32* seg_rec, u32* out) {
  // api_msm.hip msm_segments_device (:676-679)
  if (group == 1) {
    if (split) segments<FpPolicy, SEG_GLV, FpPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
    else segments<FpPolicy, SEG_PLAIN, FpPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
  } else {
    if (split) segments<Fp2Policy, SEG_GLS, Fp2PairPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
    else segments<Fp2Policy, SEG_PLAIN, Fp2PairPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
  }
}

// api_msm.hip :342, :346
void emu_decompose(int group, const u32* scalars, u32* out, int n, u32* status, int form) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_glv_decompose(scalars, out, n, status, form); });
  else launch_loop(nblk(n, 256), 256, [=] { k_gls_decompose(scalars, out, n, status, form); });
}

// api_msm.hip :426 (G1); ctrl[2] = number of items
void emu_msm_accumulate_g1(const u32* bases, const u32* bases2, u32 nsplit, const u32* sorted, const u32* items, const u32* ctrl, u32* records, u32 max_items) {
  launch_loop(nblk(max_items, BLS_ACC_BLOCK), BLS_ACC_BLOCK,
              [=] { k_msm_accumulate<FpPolicy>(bases, bases2, nsplit, sorted, reinterpret_cast<const ItemDesc*>(items), ctrl, records); });
}
void emu_proj_export(int group, const u32* rec, u32* xyz, size_t n) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_proj_export<FpPolicy>(rec, xyz, n); });
  else launch_loop(nblk(n, 256), 256, [=] { k_proj_export<Fp2Policy>(rec, xyz, n); });
}
}
