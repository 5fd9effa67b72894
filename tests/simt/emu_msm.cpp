// tests/simt/emu_msm.cpp -- the MSM kernels of bls12_381_amd/csrc compiled for the HOST (test infrastructure only): the segmented MSM
// (msm_seg.hip.h), the scalar decompositions, the endomorphism images, the subgroup check, the bucket accumulations of msm.hip.h and the
// point kernels behind them (cut-bucket fold, level forms, tree sums, shift-add, window combine), one stage per entry point.
// The entry points launch the __global__ functions themselves with the grid and block shapes of api_msm.hip (each names the function it
// follows); the level forms, their grids, the tree jobs and the whole reduction schedule come from csrc/msm_plan.h, the header the
// product launches from.  Every lane is a host thread where lanes cooperate (tests/simt/hip/hip_runtime.h), so that the CPU suite can
// compare the very code the GPU runs with the oracle (tests/test_simt_msm.py, tests/test_simt_msm_points.py).
//
// The lane pool, the launchers, the trapping checks and emu_guarded() are those of tests/simt/emu_harness.h; the tests call this
// library from a child process (tests/simt_msm_child.py).
#define EMU_LANES 256
#include "emu_harness.h"

#include "msm_seg.hip.h"
#include "abi_kernels.hip.h"
#include "msm_plan.h"

using namespace bls;

namespace {

// api_msm.hip msm_segments_launch: the batch loop, accumulate -> combine -> export per batch of `batch` segments
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

// api_msm.hip bases_import, bases_make_endo; group 1 = G1, 2 = G2
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
  // api_msm.hip msm_segments_device
  if (group == 1) {
    if (split) segments<FpPolicy, SEG_GLV, FpPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
    else segments<FpPolicy, SEG_PLAIN, FpPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
  } else {
    if (split) segments<Fp2Policy, SEG_GLS, Fp2PairPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
    else segments<Fp2Policy, SEG_PLAIN, Fp2PairPolicy>(rec, endo, nbases, base_first, offsets, scalars, k, batch, total, form, status, wsums, seg_rec, out);
  }
}

// api_msm.hip msm_sort_fast: the decomposition in front of the sort
void emu_decompose(int group, const u32* scalars, u32* out, int n, u32* status, int form) {
  if (group == 1) launch_loop(nblk(n, 256), 256, [=] { k_glv_decompose(scalars, out, n, status, form); });
  else launch_loop(nblk(n, 256), 256, [=] { k_gls_decompose(scalars, out, n, status, form); });
}

// api_msm.hip msm_accumulate (G1); ctrl[2] = number of items
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
// api_msm.hip msm_accumulate (G2): one lane pair per item, the grid covers 2 * max_items lanes
void emu_msm_accumulate_g2(const u32* bases, const u32* sorted, const u32* items, const u32* ctrl, u32* records, u32 max_items) {
  launch_threads(nblk(2 * (size_t)max_items, BLS_G2ACC_BLOCK), BLS_G2ACC_BLOCK,
                 [=] { k_msm_accumulate_g2pair(bases, sorted, reinterpret_cast<const ItemDesc*>(items), ctrl, records); });
}
// api_msm.hip msm_accumulate, the fold: one lane per bucket of the call, then HEAVY_BIG_BLOCKS blocks for the block-folded buckets
void emu_msm_heavy(int group, const u32* heavy, const u32* ctrl, u32* records, u32 gnb) {
  const u32 small_blocks = nblk(gnb, 256);
  const uint4* h = reinterpret_cast<const uint4*>(heavy);
  if (group == 1) launch_threads(small_blocks + HEAVY_BIG_BLOCKS, 256, [=] { k_msm_heavy<FpPolicy>(h, ctrl, records, gnb, small_blocks); });
  else launch_threads(small_blocks + HEAVY_BIG_BLOCKS, 256, [=] { k_msm_heavy<Fp2Policy>(h, ctrl, records, gnb, small_blocks); });
}
}  // extern "C"

namespace {

// one reduction level in a given form (msm_plan.h MSM_FORM_*: 0 = team2, 1 = team, 2 = the pair form of the group), as api_msm.hip
// msm_reduce launches it; the lanes of a form are msm_level_lanes
template <class F>
void level(int form, const u32* E, u32* Rout, u32* Tout, int nseg, int n, int M, int off) {
  const size_t lanes = msm_level_lanes(form, (size_t)nseg * (n / M));
  const unsigned grid = (unsigned)msmp_nblk(lanes, MSMP_BLOCK);
  if (form == MSM_FORM_TEAM2) launch_threads(grid, MSMP_BLOCK, [=] { k_wsum_level_team2<F>(E, Rout, Tout, nseg, n, M, off); });
  else if (form == MSM_FORM_TEAM) launch_threads(grid, MSMP_BLOCK, [=] { k_wsum_level_team<F>(E, Rout, Tout, nseg, n, M, off); });
  else if constexpr (std::is_same<F, Fp2Policy>::value) launch_threads(grid, MSMP_BLOCK, [=] { k_wsum_level_g2pair(E, Rout, Tout, nseg, n, M, off); });
  else launch_threads(nblk(lanes, BLS_WSUM_BLOCK), BLS_WSUM_BLOCK, [=] { k_wsum_level_pair(E, Rout, Tout, nseg, n, M, off); });
}
// the multi-job tree launch of one step
template <class F>
void tree_multi(const TreeJobs& J) {
  if (J.njobs) launch_threads(msm_tree_multi_grid((size_t)J.first_team[J.njobs]), MSMP_BLOCK, [=] { k_tree_sum_team_multi<F>(J); });
}
template <class F>
void tree_one(const u32* E, u32* out, int nseg, int n, int M) {
  launch_loop(nblk((size_t)nseg * ((n + M - 1) / M), 256), 256, [=] { k_tree_sum<F>(E, out, nseg, n, M); });
}
template <class F>
void shift_add(const u32* x, const u32* y, u32* out, int nseg, int k) {
  launch_threads(nblk((size_t)nseg * TEAM, 256), 256, [=] { k_shift_add_team<F>(x, y, out, nseg, k); });
}

// The whole bucket reduction by the schedule of msm_plan.h, as api_msm.hip msm_reduce / msm_tree_step walk it (one stream here):
// records: nseg * nbw bucket records; lvlR[2], lvlT, tsum[2], wacc[2] (Horner table, Horner accumulator), wsums: the slot's buffers at
// the sizes of msm_sizes.  fault: 1 = the bottom level runs with off = 0 (a seeded fault the test must catch).
template <class F>
void reduce(const MsmReduction& red, const u32* records, u32* const* lvlR, u32* lvlT, u32* const* tsum, u32* const* wacc, u32* wsums, int fault) {
  constexpr int PW = Store<F>::PROJ_WORDS;
  const int nseg = red.nseg;
  auto row = [=](int l) { return wacc[0] + (size_t)l * nseg * PW; };
  auto tree_step = [&](const MsmTreeStep& st) {
    auto in = [=](const MsmTreePass& p) -> const u32* { return (p.src < 0 ? lvlT : tsum[p.src]) + p.off * PW; };
    auto out = [=](const MsmTreePass& p) -> u32* { return p.to_horner ? row(p.level) : tsum[p.pp] + p.off * PW; };
    for (int i = 0; i < st.npass; i++)
      if (!st.pass[i].multi) tree_one<F>(in(st.pass[i]), out(st.pass[i]), nseg, st.pass[i].n, st.pass[i].TM);
    TreeJobs J;
    msm_tree_jobs(J, nseg, st, in, out);
    tree_multi<F>(J);
  };
  const u32* E = records;
  for (int l = 0; l < red.levels; l++) {
    const MsmLevel& L = red.level[l];
    u32* Rout = lvlR[l & 1];
    level<F>(L.form, E, Rout, L.to_horner ? row(l) : lvlT + L.toff * PW, nseg, L.n, L.M, fault && l == 0 ? 0 : L.off);
    tree_step(red.step[l]);
    E = Rout;
  }
  for (int t = red.levels; t < red.nsteps; t++) tree_step(red.step[t]);
  if (red.levels == 0) { memcpy(wsums, records, (size_t)nseg * PW * 4); return; }
  u32* acc = wacc[1];
  memcpy(acc, row(red.levels - 1), (size_t)nseg * PW * 4);
  for (int l = red.levels - 2; l >= 0; l--) shift_add<F>(acc, row(l), acc, nseg, red.level[l].shift);
  memcpy(wsums, acc, (size_t)nseg * PW * 4);
}

}  // namespace

extern "C" {

// one level in the form asked for.  The product picks the form by the lane count (msm_reduction); here every form runs on the same inputs.
void emu_wsum_level(int group, int form, const u32* E, u32* Rout, u32* Tout, int nseg, int n, int M, int off) {
  if (group == 1) level<FpPolicy>(form, E, Rout, Tout, nseg, n, M, off);
  else level<Fp2Policy>(form, E, Rout, Tout, nseg, n, M, off);
}
// the one-lane tree pass (api_msm.hip msm_tree_step, a pass that is no job of the multi launch)
void emu_tree_sum(int group, const u32* E, u32* out, int nseg, int n, int M) {
  if (group == 1) tree_one<FpPolicy>(E, out, nseg, n, M);
  else tree_one<Fp2Policy>(E, out, nseg, n, M);
}
// one pass of njobs trees in one launch; job j sums n[j] records per window in groups of M[j], assembled by msm_tree_jobs as the
// product's are.  The schedule always takes M = min(8, n); the kernel's contract is wider (any M <= maxM), and the tests use both.
void emu_tree_sum_multi(int group, int njobs, const u32* const* in, u32* const* out, const int* n, const int* M, int nseg) {
  if (njobs > MSMP_MAX_LEVELS) __builtin_trap();
  MsmTreeStep st;
  st.npass = st.njobs = njobs; st.multi_grid = 0;
  for (int t = 0; t < njobs; t++) {
    MsmTreePass& p = st.pass[t];
    p.level = t; p.n = n[t]; p.TM = M[t]; p.TG = (n[t] + M[t] - 1) / M[t]; p.src = -1; p.pp = 0; p.to_horner = false; p.multi = true; p.off = 0;
  }
  TreeJobs J;
  msm_tree_jobs(J, nseg, st, [=](const MsmTreePass& p) { return in[p.level]; }, [=](const MsmTreePass& p) { return out[p.level]; });
  if (group == 1) tree_multi<FpPolicy>(J);
  else tree_multi<Fp2Policy>(J);
}
// the Horner step of api_msm.hip msm_reduce
void emu_shift_add(int group, const u32* x, const u32* y, u32* out, int nseg, int k) {
  if (group == 1) shift_add<FpPolicy>(x, y, out, nseg, k);
  else shift_add<Fp2Policy>(x, y, out, nseg, k);
}
// api_msm.hip msm_combine
void emu_msm_combine(int group, const u32* wsums, u32* out, int nwin, int c) {
  if (group == 1) launch_threads(1, TEAM, [=] { k_msm_combine_team<FpPolicy>(wsums, out, nwin, c); });
  else launch_threads(1, TEAM, [=] { k_msm_combine_team<Fp2Policy>(wsums, out, nwin, c); });
}
// the words of the reduction's buffers for nseg bucket sets of nbw buckets (msm_sizes): lvlR, lvlT, tsum, wacc, wsums
void emu_msm_reduce_words(int group, int nseg, u32 nbw, size_t* words) {
  MsmShape s;
  s.nseg = s.nwin = nseg; s.nbw = nbw; s.nb = (size_t)nseg * nbw;
  const MsmSizes z = msm_sizes(s, group == 1 ? Store<FpPolicy>::PROJ_WORDS : Store<Fp2Policy>::PROJ_WORDS, false);
  const size_t v[5] = {z.lvlR / 4, z.lvlT / 4, z.tsum / 4, z.wacc / 4, z.wsums / 4};
  for (int i = 0; i < 5; i++) words[i] = v[i];
}
// the whole reduction: bucket records in, one window sum per bucket set out; returns the number of levels, -1 for a refused schedule
int emu_msm_reduce(int group, const u32* records, int nseg, u32 nbw, u32* const* lvlR, u32* lvlT, u32* const* tsum, u32* const* wacc, u32* wsums, int fault) {
  const MsmReduction red = msm_reduction(nseg, nbw);
  if (red.refusal) return -1;
  if (group == 1) reduce<FpPolicy>(red, records, lvlR, lvlT, tsum, wacc, wsums, fault);
  else reduce<Fp2Policy>(red, records, lvlR, lvlT, tsum, wacc, wsums, fault);
  return red.levels;
}
}
