// tests/cpp/msm_plan_main.cpp -- csrc/msm_plan.h on its own, built with the address and undefined-behaviour sanitizers and run directly
// (tests/test_msm_plan.py).  It sweeps the shape of a call over both groups, n = the powers of two up to 2^27 and +-1 around 2^22, 2^23
// and 2^24 (where the endomorphism split switches off), every forced window 4..16, every table window 9..21, with and without images,
// no_glv, force_slow_sort and an item cap of 16; it holds every accepted shape, its buffer sizes and its reduction schedule to the
// properties below, hands each of the three refusals one call, and prints every shape and every schedule in a fixed text form that
// tests/test_msm_plan.py compares with the Python model.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>
#include "msm_plan.h"
using namespace bls;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

static const char* const ENTRIES = "msm: n * windows exceeds 2^32 entries";
static const char* const COUNTERS = "msm: window configuration exceeds the sort's counter table";
static const char* const FALLBACK = "msm: too many buckets for the fallback sort (use a window <= 16)";
static const int PROJ_WORDS[3] = {0, 44, 84};        // Store<F>::PROJ_WORDS of G1 / G2

static const char* tag(const char* refusal) {
  if (!refusal) return "none";
  if (!std::strcmp(refusal, ENTRIES)) return "entries";
  if (!std::strcmp(refusal, COUNTERS)) return "counters";
  if (!std::strcmp(refusal, FALLBACK)) return "fallback";
  REQUIRE(!"a refusal with an unknown text");
  return "";
}

// the schedule of one (nseg, nbw) against the sizes of the shape it belongs to
static void check_reduction(const MsmShape& s, const MsmSizes& z, size_t rec) {
  const MsmReduction r = msm_reduction(s.nseg, s.nbw);
  REQUIRE(!r.refusal && r.nseg == s.nseg);
  REQUIRE(r.levels >= 1 && r.levels <= 7 && r.nsteps >= r.levels && r.nsteps <= MSMP_MAX_STEPS);
  size_t trecords = 0;
  int n = (int)s.nbw;
  for (int l = 0; l < r.levels; l++) {
    const MsmLevel& L = r.level[l];
    REQUIRE(L.n == n && L.M == (n >= 8 ? 8 : n) && L.G * L.M == n && L.off == (l == 0 ? 1 : 0) && (1 << L.shift) == L.M);
    REQUIRE(L.toff == trecords && L.to_horner == (L.G == 1));
    const size_t chains = (size_t)s.nseg * L.G;
    REQUIRE(L.lanes == chains * (L.form == MSM_FORM_TEAM2 ? 2 * MSMP_TEAM : L.form == MSM_FORM_TEAM ? MSMP_TEAM : 2));
    REQUIRE(L.form == MSM_FORM_PAIR || L.lanes <= TEAM_LANES_MAX);
    REQUIRE((size_t)L.grid * MSMP_BLOCK >= L.lanes && (size_t)(L.grid - 1) * MSMP_BLOCK < L.lanes);
    REQUIRE(chains * rec <= z.lvlR);                           // the level's R records
    trecords += chains;
    n = L.G;
  }
  REQUIRE(n == 1);
  REQUIRE(trecords * rec <= z.lvlT);                           // every level's T records side by side
  REQUIRE((size_t)r.levels * s.nseg * rec <= z.wacc);          // the Horner table: one row of nseg records per level
  // the trees: every level with G > 1 has one, it takes a pass in every step from its own level on until one record is left
  int left[MSMP_MAX_LEVELS];
  for (int l = 0; l < r.levels; l++) left[l] = r.level[l].G;
  for (int t = 0; t < r.nsteps; t++) {
    const MsmTreeStep& st = r.step[t];
    int np = 0, jobs = 0;
    size_t teams = 0;
    for (int l = 0; l < r.levels && l <= t; l++) {
      if (left[l] <= 1) continue;
      REQUIRE(np < st.npass);
      const MsmTreePass& p = st.pass[np++];
      REQUIRE(p.level == l && p.n == left[l] && p.TM == (p.n >= 8 ? 8 : p.n) && p.TG == (p.n + p.TM - 1) / p.TM && p.off == r.level[l].toff);
      REQUIRE(p.src == (p.n == r.level[l].G ? -1 : (p.pp ^ 1)) && (p.pp == 0 || p.pp == 1) && p.to_horner == (p.TG == 1));
      REQUIRE(p.multi);                                        // k_tree_sum is never scheduled
      REQUIRE((p.off + (size_t)s.nseg * p.TG) * rec <= z.tsum);        // the pass's output fits tsum at its offset
      teams += (size_t)s.nseg * p.TG; jobs++;
      left[l] = p.TG;
    }
    REQUIRE(np == st.npass && jobs == st.njobs && jobs <= MSMP_TREE_JOBS_MAX);
    REQUIRE(teams * MSMP_TEAM <= (size_t)st.multi_grid * MSMP_BLOCK && (jobs == 0) == (st.multi_grid == 0));
    REQUIRE(t < r.levels || np > 0);
  }
  for (int l = 0; l < r.levels; l++) REQUIRE(left[l] == 1);    // every tree reaches n = 1
}

static void print_reduction(int nseg, uint32_t nbw) {
  const MsmReduction r = msm_reduction(nseg, nbw);
  std::printf("sched nseg=%d nbw=%u levels=%d nsteps=%d :", nseg, nbw, r.levels, r.nsteps);
  for (int l = 0; l < r.levels; l++) {
    const MsmLevel& L = r.level[l];
    std::printf(" L%d,%d,%d,%d,%d,%u,%zu,%d", L.n, L.M, L.G, L.off, L.form, L.grid, L.toff, (int)L.to_horner);
  }
  std::printf(" :");
  for (int t = 0; t < r.nsteps; t++) {
    const MsmTreeStep& st = r.step[t];
    std::printf(" S%d,%u", st.njobs, st.multi_grid);
    for (int i = 0; i < st.npass; i++) {
      const MsmTreePass& p = st.pass[i];
      std::printf("/%d,%d,%d,%d,%d,%d,%d,%d,%zu", p.level, p.n, p.TM, p.TG, p.src, p.pp, (int)p.to_horner, (int)p.multi, p.off);
    }
  }
  std::printf(" : H");
  for (int l = r.levels - 2; l >= 0; l--) std::printf(" %d", r.level[l].shift);
  std::printf("\n");
}

static void sweep() {
  std::vector<size_t> ns;
  for (int l = 0; l <= 27; l++) ns.push_back((size_t)1 << l);
  for (int l = 22; l <= 24; l++) { ns.push_back(((size_t)1 << l) - 1); ns.push_back(((size_t)1 << l) + 1); }
  std::set<std::pair<int, uint32_t>> reductions;
  size_t accepted = 0, refused = 0;
  for (int group = 1; group <= 2; group++)
    for (size_t n : ns)
      for (int w = 0; w < 27; w++) {
        const int msm_c = w == 0 ? 0 : w <= 13 ? w + 3 : 0;    // automatic, forced 4..16
        const int table_c = w <= 13 ? 0 : w - 14 + 9;           // tables 9..21
        for (int flags = 0; flags < 16; flags++) {
          const bool images = flags & 1, no_glv = flags & 2, slow = flags & 4;
          const uint32_t item_cap = flags & 8 ? 16 : 0;
          const MsmShape s = msm_shape(group, n, table_c, images, no_glv, slow, msm_c, item_cap);
          std::printf("shape group=%d n=%zu table_c=%d images=%d no_glv=%d slow=%d msm_c=%d item_cap=%u : glv=%d gls=%d ns=%zu sbits=%d cw=%d nwin=%d nseg=%d "
                      "nbw=%u nb=%zu total=%zu fast=%d fine=%d ncoarse=%d nc=%d cap=%u items=%zu records=%zu refusal=%s\n",
                      group, n, table_c, (int)images, (int)no_glv, (int)slow, msm_c, item_cap, (int)s.glv, (int)s.gls, s.ns, s.sbits, s.cw, s.nwin, s.nseg,
                      s.nbw, s.nb, s.total, (int)s.fast_sort, s.fine_bits, s.ncoarse, s.nc, s.cap, s.max_items, s.max_records, tag(s.refusal));
          REQUIRE(s.n == n && s.merged == (table_c != 0) && !(s.glv && s.gls) && s.ns == n * (s.glv ? 2 : s.gls ? 4 : 1));
          REQUIRE(s.cw >= 4 && s.cw <= 21 && s.nwin * s.cw >= s.sbits && (s.nwin - 1) * s.cw < s.sbits && s.nbw == 1u << (s.cw - 1));
          REQUIRE(s.nb == (size_t)s.nseg * s.nbw && s.total == (size_t)s.nwin * s.ns && s.nseg == (s.merged ? 1 : s.nwin));
          REQUIRE(s.fine_bits >= 0 && s.fine_bits <= 7 && s.nc == s.nseg * s.ncoarse && s.ncoarse << s.fine_bits == (int)s.nbw);
          // of the three refusals only the first is within reach of the windows the product accepts, and it means what it says
          REQUIRE(!s.refusal || (!std::strcmp(s.refusal, ENTRIES) && s.total > 0xfffffff0ull));
          if (s.refusal) { refused++; continue; }
          accepted++;
          REQUIRE(s.total <= 0xfffffff0ull);
          REQUIRE(!s.fast_sort || s.nc <= MSMP_SORT_MAX_COUNTERS);
          REQUIRE(s.fast_sort || msmp_nblk(s.nb, 1024) <= 4096);
          REQUIRE(s.fast_sort || s.ns > ((size_t)1 << 24) || slow);
          REQUIRE(s.cap == (item_cap ? item_cap : s.cap) && (item_cap || (s.cap >= 128 && s.cap <= (uint32_t)ITEM_CAP_MAX && (s.cap & (s.cap - 1)) == 0)));
          // every bucket keeps one item and a bucket of load L has ceil(L / cap) <= L / cap + 1 of them: the lanes of the accumulation
          // grid (one per item, G2: two) cover the worst case, and the grid fits the 32-bit launch dimension
          REQUIRE(s.max_items >= s.total / s.cap + s.nb && s.max_records == s.nb + s.max_items);
          const size_t acc_lanes = (group == 2 ? 2 : 1) * s.max_items;
          REQUIRE(msmp_nblk(acc_lanes, 256) * 256 >= acc_lanes && msmp_nblk(acc_lanes, 256) < ((size_t)1 << 31));
          const size_t rec = (size_t)PROJ_WORDS[group] * 4;
          for (int mont = 0; mont < 2; mont++) {
            const MsmSizes z = msm_sizes(s, PROJ_WORDS[group], mont != 0);
            REQUIRE(z.ent == s.total * 4 && z.sorted == z.ent && z.cursor == (s.fast_sort ? 0 : z.ent));
            REQUIRE(z.hist >= s.nb * 4 && z.hist >= (3 * (size_t)MSMP_SORT_MAX_COUNTERS + 4) * 4 && z.offs == (s.nb + 1) * 4);
            REQUIRE(z.glv == (s.glv || s.gls ? s.ns * (size_t)(s.sbits / 8) : mont ? n * 32 : 0));
            REQUIRE(z.items == s.max_items * MSMP_ITEM_BYTES && z.heavy == 2 * s.nb * MSMP_HEAVY_BYTES && z.ctrl == (size_t)MSMP_CTRL_WORDS * 4);
            REQUIRE(z.buckets == s.max_records * rec && z.wsums == (size_t)s.nwin * rec && z.result == rec && z.bsum >= msmp_nblk(s.nb, 1024) * 4);
            if (!mont) check_reduction(s, z, rec);
          }
          reductions.insert({s.nseg, s.nbw});
        }
      }
  REQUIRE(accepted > 20000 && refused > 0);
  for (const auto& r : reductions) print_reduction(r.first, r.second);
  std::printf("sweep\n");
}

static void refusals() {
  // one call each; none of the last two is a window the product lets through (blsgpu_set_msm_window: 4..16, blsgpu_bases_precompute: 9..21)
  REQUIRE(!std::strcmp(tag(msm_shape(1, (size_t)1 << 27, 0, false, false, false, 8, 0).refusal), "entries"));
  REQUIRE(!std::strcmp(tag(msm_shape(1, 256, 22, true, false, false, 0, 0).refusal), "counters"));
  REQUIRE(!std::strcmp(tag(msm_shape(2, 256, 0, true, false, true, 20, 0).refusal), "fallback"));
  REQUIRE(!msm_shape(1, (size_t)1 << 27, 0, false, false, false, 9, 0).refusal);
  // a schedule deeper than the slot has level events is a refusal, not an overrun: 2^25 buckets would take nine levels
  REQUIRE(!msm_reduction(1, 1u << 24).refusal && msm_reduction(1, 1u << 24).levels == 8);
  REQUIRE(msm_reduction(1, 1u << 25).refusal && !std::strcmp(msm_reduction(1, 1u << 25).refusal, "msm: reduction depth"));
  // the one-lane tree pass stays in the schedule as data: it takes a tree whose next pass is wider than the team form allows
  const MsmReduction wide = msm_reduction(64, 1u << 23);
  REQUIRE(!wide.refusal && !wide.step[0].pass[0].multi && wide.step[0].njobs == 0 && wide.step[0].multi_grid == 0);
  std::printf("refusals\n");
}

int main() {
  sweep();
  refusals();
  std::printf("all ok\n");
  return 0;
}
