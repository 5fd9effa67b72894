// msm_plan.h -- the large MSM (blsgpu_g{1,2}_msm*; api_msm.hip msm_device) as plain host code: the shape of a call (decomposition,
// window, sort-key split, item cap, the three refusals), the byte size of every slot buffer, and the schedule of the bucket reduction
// (level forms and grids, the tree passes after every level, the Horner shifts).  No HIP calls here: api_msm.hip launches from the
// plan, tests/simt/emu_msm.cpp and tests/simt/emu_msm_front.cpp walk the same plan on the host, tests/cpp/msm_plan_main.cpp sweeps
// it under sanitizers and tests/test_msm_plan.py compares the sweep with the Python model (tests/msm_pipe_model.py).
#pragma once
#include <stddef.h>
#include "limits.h"

namespace bls {

// restated from msm.hip.h / team.hip.h, which are device code (api_msm.hip static_asserts every one against its origin)
constexpr int MSMP_TEAM = 8;                         // team.hip.h TEAM
constexpr int MSMP_SORT_MAX_COUNTERS = 8192;         // msm.hip.h SORT_MAX_COUNTERS
constexpr int MSMP_TREE_JOBS_MAX = 8;                // msm.hip.h TREE_JOBS_MAX
constexpr int MSMP_CTRL_WORDS = 4 + 2 * (ITEM_CAP_MAX + 1);      // msm.hip.h: 4 control words, ITEM_BINS bins, ITEM_BINS cursors
constexpr size_t MSMP_ITEM_BYTES = 12;               // sizeof(ItemDesc)
constexpr size_t MSMP_HEAVY_BYTES = 16;              // sizeof(uint4)
constexpr unsigned MSMP_BLOCK = 256;                 // threads per block of every reduction launch
// a reduction level runs one chain per TEAM of lanes when that still fits comfortably on the chip
constexpr size_t TEAM_LANES_MAX = 131072;
constexpr int MSMP_MAX_LEVELS = 8;                   // Slot::ev_lvl has one event per level
constexpr int MSMP_MAX_STEPS = 2 * MSMP_MAX_LEVELS;

inline size_t msmp_nblk(size_t n, size_t bs) { return (n + bs - 1) / bs; }

inline int msm_pick_window(size_t n, int bits) {
  // minimise  n*W (mixed adds) + 2*W*2^(c-1)*1.2 (bucket reduction), W = ceil(bits/c); n = scalars of `bits` bits
  int best = 8; double bc = 1e300;
  for (int c = 6; c <= 16; c++) {
    int W = (bits + c - 1) / c;
    double cost = (double)n * W + 2.4 * W * (double)(1u << (c - 1));
    if (cost < bc) { bc = cost; best = c; }
  }
  return best;
}

// the two-level counting sort cuts its key (bucket set, |digit| - 1) into a coarse part that counts in LDS -- nc = nseg * ncoarse
// counters -- and a fine part of at most 7 bits (k_sort_fine: 128 counters per workgroup)
struct MsmSortSplit { int fine_bits, ncoarse, nc; };
inline MsmSortSplit msm_sort_split(int cw, int nseg, bool merged) {
  const int key_bits = cw - 1;
  const int coarse_bits = merged ? (key_bits > 7 ? key_bits - 7 : 0) : (key_bits < 8 ? key_bits : 8);
  return {key_bits - coarse_bits, 1 << coarse_bits, nseg * (1 << coarse_bits)};
}

// ---- the shape of a call -----------------------------------------------------------------------------------------------------------
struct MsmShape {
  const char* refusal = nullptr;       // NULL: accepted; else the text of the refusal (nothing may be enqueued)
  bool merged = false;                 // resident window-shifted tables (blsgpu_bases_precompute): all windows share one bucket set
  bool glv = false;                    // G1: 2n points (the bases and their images under the endomorphism) with balanced 127-bit scalars -> half the windows
  bool gls = false;                    // G2: 4n points (every base with its images under psi, psi^2, psi^3) with 63-bit scalars -> a quarter of the windows
  size_t n = 0, ns = 0;                // scalars of the call / scalars the sort sees
  int sbits = 0;                       // ... and their width (incl. the spare bit of the signed recoding)
  int cw = 0, nwin = 0, nseg = 0;      // window bits, digit windows per scalar, independent bucket sets
  uint32_t nbw = 0;                    // buckets per set
  size_t nb = 0, total = 0;            // buckets, sort entries
  bool fast_sort = false;              // the two-level counting sort; else the global-atomic fallback
  int fine_bits = 0, ncoarse = 0, nc = 0;      // the split of the key (window, |digit| - 1): fine part <= 7 bits, nc = nseg * ncoarse LDS counters
  uint32_t cap = 0;                    // entries per work item
  size_t max_items = 0, max_records = 0;       // every bucket has >= 1 item; bucket sums + partial sums of cut buckets
};
// group: 1 = G1, 2 = G2; n in [1, 2^27]; table_c: the window of the bases' resident tables ([9, 21]; 0 = none); images: the bases carry
// their endomorphism images; msm_c: the forced window ([4, 16]; 0 = automatic); item_cap: the forced cap (0 = automatic)
inline MsmShape msm_shape(int group, size_t n, int table_c, bool images, bool no_glv, bool force_slow_sort, int msm_c, uint32_t item_cap) {
  MsmShape s;
  s.n = n;
  s.merged = table_c != 0;
  // Calls beyond the sort's index width with the endomorphism split (G1: 2 n > 2^24, G2: 4 n > 2^24) run on plain windows.
  // Cutting them into passes that each keep the split was measured (round 3, 2^24 G1 points on one MI355X: two GLV passes
  // 52.6 ms against 45.9 ms for one plain pass): the split halves the WINDOWS, not the bucket additions, and at this size
  // the additions are everything -- two tails and gathers over twice the memory only add to them.
  const bool split = !s.merged && images && !no_glv && !force_slow_sort;
  s.glv = group == 1 && split && 2 * n <= ((size_t)1 << 24);
  s.gls = group == 2 && split && 4 * n <= ((size_t)1 << 24);
  s.ns = s.glv ? 2 * n : s.gls ? 4 * n : n;
  s.sbits = s.glv ? 128 : s.gls ? 64 : 256;
  s.cw = s.merged ? table_c : (msm_c ? msm_c : msm_pick_window(s.ns, s.sbits));
  s.nwin = (s.sbits + s.cw - 1) / s.cw;
  s.nseg = s.merged ? 1 : s.nwin;
  s.nbw = 1u << (s.cw - 1);
  s.nb = (size_t)s.nseg * s.nbw;
  s.total = (size_t)s.nwin * s.ns;
  s.fast_sort = s.merged || ((s.ns <= ((size_t)1 << 24)) && s.cw <= 16 && s.cw >= 2 && !force_slow_sort);
  const MsmSortSplit split_key = msm_sort_split(s.cw, s.nseg, s.merged);
  s.fine_bits = split_key.fine_bits; s.ncoarse = split_key.ncoarse; s.nc = split_key.nc;
  // item cap: ~4x the mean bucket load, so that with uniform scalars (almost) no bucket is cut
  s.cap = 128;
  while (s.cap < (uint32_t)ITEM_CAP_MAX && (size_t)s.cap * s.nbw < 4 * s.ns) s.cap *= 2;
  if (item_cap) s.cap = item_cap;
  // with resident tables the single bucket set holds the entries of ALL nwin windows: `total` counts them either way (the
  // accumulation kernels run one lane per item without a grid stride, so their grid must cover max_items)
  s.max_items = s.total / s.cap + s.nb + 1;
  s.max_records = s.nb + s.max_items;
  if (s.total > 0xfffffff0ull) s.refusal = "msm: n * windows exceeds 2^32 entries";
  else if (s.fast_sort && s.nc > MSMP_SORT_MAX_COUNTERS) s.refusal = "msm: window configuration exceeds the sort's counter table";
  else if (!s.fast_sort && msmp_nblk(s.nb, 1024) > 4096) s.refusal = "msm: too many buckets for the fallback sort (use a window <= 16)";
  return s;
}

// ---- scratch: the bytes msm_device reserves in its slot, in the order it reserves them ------------------------------------------------
struct MsmSizes {
  size_t ent, sorted, hist, cursor, glv, offs, bsum, items, heavy, ctrl;
  size_t buckets, lvlR, lvlT, tsum, wacc, wsums, result;       // lvlR, tsum, wacc: each of the two
};
// pw: words of a projective record (Store<F>::PROJ_WORDS); mont: the scalars arrive as Montgomery limbs
inline MsmSizes msm_sizes(const MsmShape& s, int pw, bool mont) {
  MsmSizes z;
  const size_t rec = (size_t)pw * 4;
  z.ent = s.total * 4;
  z.sorted = s.total * 4;
  // the fast sort's fixed layout [MAX] counts | [MAX + 1] bases | [MAX] cursors; the fallback's histogram over every bucket
  z.hist = (s.nb > 3 * (size_t)MSMP_SORT_MAX_COUNTERS + 4 ? s.nb : 3 * (size_t)MSMP_SORT_MAX_COUNTERS + 4) * 4;
  z.cursor = s.fast_sort ? 0 : s.total * 4;                   // per-entry rank inside its bucket (fallback sort only)
  // the split scalars, or (no decomposition kernel touches the scalars) their reduction from Montgomery form
  z.glv = s.glv ? s.ns * 16 : s.gls ? s.ns * 8 : mont ? s.n * 32 : 0;
  z.offs = (s.nb + 1) * 4;
  z.bsum = 4096 * 4;
  z.items = s.max_items * MSMP_ITEM_BYTES;
  z.heavy = 2 * s.nb * MSMP_HEAVY_BYTES;                      // the heavy list, then the indices of its block-folded entries
  z.ctrl = (size_t)MSMP_CTRL_WORDS * 4;
  z.buckets = s.max_records * rec;
  z.lvlR = (s.nb / 2 + 1) * rec;
  z.lvlT = 2 * z.lvlR;                                        // every level's T records side by side
  z.tsum = z.lvlR;
  z.wacc = (size_t)s.nwin * 32 * rec;
  z.wsums = (size_t)s.nwin * rec;
  z.result = rec;
  return z;
}

// ---- the bucket reduction ------------------------------------------------------------------------------------------------------------
// Per window  wsum = sum_b (b + 1) E_b  over nbw bucket records, by levels of fan 8: level l cuts its n records into G chunks of M and
// writes R_g = sum E_j and T_g = sum (j - g M + off) E_j; the next level runs over the R records, and
// wsum = Horner over the levels of (sum_g T_g), acc_l = T_l + M_l * acc_{l+1}.  The G T-records of a level are summed down to one by a
// tree of fan 8 on a second stream, one pass of every unfinished tree per step, so the trees finish while the R chain is still running.
enum { MSM_FORM_TEAM2 = 0, MSM_FORM_TEAM = 1, MSM_FORM_PAIR = 2 };
struct MsmLevel {
  int n, M, G, off;                    // off: 1 at the bottom level (bucket b weighs b + 1), 0 above
  int form;                            // team2: the two running sums of a chain (R and T) on two teams, T one step behind R; team: one team
                                       // per chain; pair: the lane-pair form of the group (k_wsum_level_pair / k_wsum_level_g2pair)
  size_t lanes;                        // lanes the form needs
  unsigned grid;                       // blocks of MSMP_BLOCK threads
  size_t toff;                         // offset (records) of this level's T block inside lvlT
  bool to_horner;                      // G == 1: T goes straight into the Horner table
  int shift;                           // log2(M): the Horner step across this level doubles `shift` times
};
struct MsmTreePass {
  int level;                           // the tree of this level's T records
  int n, TM, TG;                       // n records per window in, TG = ceil(n / TM) out
  int src;                             // -1: lvlT (the first pass), else tsum[src]; both at `off` records
  int pp;                              // out: tsum[pp] at `off` records ...
  bool to_horner;                      // ... unless TG == 1: the last pass lands in the Horner table
  bool multi;                          // a job of the step's one k_tree_sum_team_multi launch; else a k_tree_sum launch of its own
  size_t off;
};
struct MsmTreeStep {
  int npass, njobs;                    // passes of this step, and how many of them are jobs of the multi launch
  unsigned multi_grid;                 // blocks of MSMP_BLOCK threads of that launch: nseg * sum TG teams
  MsmTreePass pass[MSMP_MAX_LEVELS];
};
struct MsmReduction {
  const char* refusal;
  int nseg, levels, nsteps;            // steps [0, levels): after each level; [levels, nsteps): what is left when the last level has run
  MsmLevel level[MSMP_MAX_LEVELS];
  MsmTreeStep step[MSMP_MAX_STEPS];
};
// lanes of a level of `chains` = nseg * G chains in a given form, and the blocks of the multi-job tree launch over `teams` teams
inline size_t msm_level_lanes(int form, size_t chains) { return chains * (form == MSM_FORM_TEAM2 ? 2 * MSMP_TEAM : form == MSM_FORM_TEAM ? MSMP_TEAM : 2); }
inline unsigned msm_tree_multi_grid(size_t teams) { return (unsigned)msmp_nblk(teams * MSMP_TEAM, MSMP_BLOCK); }
// the TreeJobs argument of k_tree_sum_team_multi (msm.hip.h; a template parameter: no device types here) from the multi passes of a
// step; in(p) / out(p): the records a pass reads / writes
template <class Jobs, class In, class Out>
inline void msm_tree_jobs(Jobs& J, int nseg, const MsmTreeStep& st, In in, Out out) {
  J.njobs = 0; J.nseg = nseg; J.first_team[0] = 0; J.maxM = 0;
  for (int i = 0; i < st.npass; i++) {
    const MsmTreePass& p = st.pass[i];
    if (!p.multi) continue;
    const int j = J.njobs++;
    J.in[j] = in(p); J.out[j] = out(p); J.n[j] = p.n; J.M[j] = p.TM; J.G[j] = p.TG; J.first_team[j + 1] = J.first_team[j] + nseg * p.TG;
    if (p.TM > J.maxM) J.maxM = p.TM;
  }
}
inline MsmReduction msm_reduction(int nseg, uint32_t nbw) {
  MsmReduction r;
  r.refusal = nullptr; r.nseg = nseg; r.levels = 0; r.nsteps = 0;
  struct Tree { int level, n, src, pp; size_t off; } tree[MSMP_MAX_LEVELS];
  int ntree = 0;
  // one pass of every unfinished tree; false when none had a pass left
  auto tree_step = [&](MsmTreeStep& st) {
    st.npass = 0; st.njobs = 0; st.multi_grid = 0;
    size_t teams = 0;
    for (int t = 0; t < ntree; t++) {
      Tree& tr = tree[t];
      if (tr.n <= 1) continue;
      MsmTreePass& p = st.pass[st.npass++];
      p.level = tr.level; p.n = tr.n; p.TM = tr.n >= 8 ? 8 : tr.n; p.TG = (tr.n + p.TM - 1) / p.TM;
      p.src = tr.src; p.pp = tr.pp; p.off = tr.off; p.to_horner = p.TG == 1;
      p.multi = (size_t)nseg * p.TG * MSMP_TEAM <= TEAM_LANES_MAX && st.njobs < MSMP_TREE_JOBS_MAX;
      if (p.multi) { st.njobs++; teams += (size_t)nseg * p.TG; }
      tr.src = tr.pp; tr.n = p.TG; tr.pp ^= 1;
    }
    st.multi_grid = msm_tree_multi_grid(teams);
    return st.npass != 0;
  };
  int nn = (int)nbw, off = 1;
  size_t toff = 0;
  while (nn > 1) {
    if (r.levels == MSMP_MAX_LEVELS) { r.refusal = "msm: reduction depth"; return r; }
    MsmLevel& L = r.level[r.levels];
    L.n = nn; L.M = nn >= 8 ? 8 : nn; L.G = nn / L.M; L.off = off; L.toff = toff; L.to_horner = L.G == 1;
    L.shift = 0; while ((1 << L.shift) < L.M) L.shift++;
    const size_t chains = (size_t)nseg * L.G;
    L.form = msm_level_lanes(MSM_FORM_TEAM2, chains) <= TEAM_LANES_MAX ? MSM_FORM_TEAM2 : msm_level_lanes(MSM_FORM_TEAM, chains) <= TEAM_LANES_MAX ? MSM_FORM_TEAM : MSM_FORM_PAIR;
    L.lanes = msm_level_lanes(L.form, chains);
    L.grid = (unsigned)msmp_nblk(L.lanes, MSMP_BLOCK);
    if (L.G > 1) tree[ntree++] = {r.levels, L.G, -1, 0, toff};
    tree_step(r.step[r.levels]);
    toff += chains;
    nn = L.G; off = 0; r.levels++;
  }
  r.nsteps = r.levels;
  for (;;) {
    if (r.nsteps == MSMP_MAX_STEPS) { r.refusal = "msm: reduction depth"; return r; }
    if (!tree_step(r.step[r.nsteps])) break;
    r.nsteps++;
  }
  return r;
}

}  // namespace bls
