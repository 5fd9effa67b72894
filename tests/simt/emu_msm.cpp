// tests/simt/emu_msm.cpp -- the MSM kernels of bls12_381_amd/csrc compiled for the HOST (test infrastructure only): the segmented MSM
// (msm_seg.hip.h), the scalar decompositions, the endomorphism images, the subgroup check, the bucket accumulations of msm.hip.h and the
// point kernels behind them (cut-bucket fold, level forms, tree sums, shift-add, window combine), one stage per entry point.
// The entry points launch the __global__ functions themselves with the grid and block shapes of api_msm.hip (restated below, each with
// the lines it restates), every lane a host thread where lanes cooperate (tests/simt/hip/hip_runtime.h), so that the CPU suite can
// compare the very code the GPU runs with the oracle (tests/test_simt_msm.py, tests/test_simt_msm_points.py).
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

// ---- the point kernels behind the sort of the large MSM, one stage per entry point (tests/test_simt_msm_points.py) ----------------
// records are PROJ records (Store<F>::PROJ_WORDS words each) in buffers of exactly the size the test states; group 1 = G1, 2 = G2
void emu_proj_import(int group, const u32* xyz, u32* rec, size_t n) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_proj_import<FpPolicy>(xyz, rec, n); });
  else launch_loop(nblk(n, 256), 256, [=] { k_proj_import<Fp2Policy>(xyz, rec, n); });
}
// api_msm.hip :428 (G2): one lane pair per item, the grid covers 2 * max_items lanes
void emu_msm_accumulate_g2(const u32* bases, const u32* sorted, const u32* items, const u32* ctrl, u32* records, u32 max_items) {
  launch_threads(nblk(2 * (size_t)max_items, BLS_G2ACC_BLOCK), BLS_G2ACC_BLOCK,
                 [=] { k_msm_accumulate_g2pair(bases, sorted, reinterpret_cast<const ItemDesc*>(items), ctrl, records); });
}
// api_msm.hip :437-438: one lane per bucket of the call, then HEAVY_BIG_BLOCKS blocks for the block-folded buckets
void emu_msm_heavy(int group, const u32* heavy, const u32* ctrl, u32* records, u32 gnb) {
  const u32 small_blocks = nblk(gnb, 256);
  const uint4* h = reinterpret_cast<const uint4*>(heavy);
  if (group == 1) launch_threads(small_blocks + HEAVY_BIG_BLOCKS, 256, [=] { k_msm_heavy<FpPolicy>(h, ctrl, records, gnb, small_blocks); });
  else launch_threads(small_blocks + HEAVY_BIG_BLOCKS, 256, [=] { k_msm_heavy<Fp2Policy>(h, ctrl, records, gnb, small_blocks); });
}
// api_msm.hip :486-494, one reduction level in the form asked for: 0 = team2 (:487), 1 = team (:490), 2 = the pair form of the group
// (:492 g2pair, :494 pair).  The product picks the form by the lane count; here every form runs on the same inputs.
void emu_wsum_level(int group, int form, const u32* E, u32* Rout, u32* Tout, int nseg, int n, int M, int off) {
  const size_t chains = (size_t)nseg * (n / M);
  if (form == 0) {
    if (group == 1) launch_threads(nblk(chains * 2 * TEAM, 256), 256, [=] { k_wsum_level_team2<FpPolicy>(E, Rout, Tout, nseg, n, M, off); });
    else launch_threads(nblk(chains * 2 * TEAM, 256), 256, [=] { k_wsum_level_team2<Fp2Policy>(E, Rout, Tout, nseg, n, M, off); });
  } else if (form == 1) {
    if (group == 1) launch_threads(nblk(chains * TEAM, 256), 256, [=] { k_wsum_level_team<FpPolicy>(E, Rout, Tout, nseg, n, M, off); });
    else launch_threads(nblk(chains * TEAM, 256), 256, [=] { k_wsum_level_team<Fp2Policy>(E, Rout, Tout, nseg, n, M, off); });
  } else {
    if (group == 1) launch_threads(nblk(chains * 2, BLS_WSUM_BLOCK), BLS_WSUM_BLOCK, [=] { k_wsum_level_pair(E, Rout, Tout, nseg, n, M, off); });
    else launch_threads(nblk(chains * 2, 256), 256, [=] { k_wsum_level_g2pair(E, Rout, Tout, nseg, n, M, off); });
  }
}
// api_msm.hip :469 / :509: the one-lane tree pass
void emu_tree_sum(int group, const u32* E, u32* out, int nseg, int n, int M) {
  const int TG = (n + M - 1) / M;
  if (group == 1) launch_loop(nblk((size_t)nseg * TG, 256), 256, [=] { k_tree_sum<FpPolicy>(E, out, nseg, n, M); });
  else launch_loop(nblk((size_t)nseg * TG, 256), 256, [=] { k_tree_sum<Fp2Policy>(E, out, nseg, n, M); });
}
// api_msm.hip tree_step (:459-473): one pass of njobs trees in one launch; job j sums n[j] records per window in groups of M[j].
// tree_step itself always takes M = min(8, n); the kernel's contract is wider (any M <= maxM), and the tests use both.
void emu_tree_sum_multi(int group, int njobs, const u32* const* in, u32* const* out, const int* n, const int* M, int nseg) {
  TreeJobs J; J.njobs = 0; J.nseg = nseg; J.first_team[0] = 0; J.maxM = 0;
  for (int t = 0; t < njobs; t++) {
    int TM = M[t], TG = (n[t] + TM - 1) / TM;
    int j = J.njobs++;
    J.in[j] = in[t]; J.out[j] = out[t]; J.n[j] = n[t]; J.M[j] = TM; J.G[j] = TG; J.first_team[j + 1] = J.first_team[j] + nseg * TG;
    if (TM > J.maxM) J.maxM = TM;
  }
  if (group == 1) launch_threads(nblk((size_t)J.first_team[J.njobs] * TEAM, 256), 256, [=] { k_tree_sum_team_multi<FpPolicy>(J); });
  else launch_threads(nblk((size_t)J.first_team[J.njobs] * TEAM, 256), 256, [=] { k_tree_sum_team_multi<Fp2Policy>(J); });
}
// api_msm.hip :536
void emu_shift_add(int group, const u32* x, const u32* y, u32* out, int nseg, int k) {
  if (group == 1) launch_threads(nblk((size_t)nseg * TEAM, 256), 256, [=] { k_shift_add_team<FpPolicy>(x, y, out, nseg, k); });
  else launch_threads(nblk((size_t)nseg * TEAM, 256), 256, [=] { k_shift_add_team<Fp2Policy>(x, y, out, nseg, k); });
}
// api_msm.hip :544
void emu_msm_combine(int group, const u32* wsums, u32* out, int nwin, int c) {
  if (group == 1) launch_threads(1, TEAM, [=] { k_msm_combine_team<FpPolicy>(wsums, out, nwin, c); });
  else launch_threads(1, TEAM, [=] { k_msm_combine_team<Fp2Policy>(wsums, out, nwin, c); });
}
}
