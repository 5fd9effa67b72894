// tests/cpp/gsum_plan_main.cpp -- bls12_381_amd/csrc/gsum_plan.h on its own (tests/test_gsum_plan.py builds this with host clang++
// -fsanitize=address,undefined and runs it; it includes nothing of the library but that header).
//
// The two passes are run as a MODEL over 64-bit integers with wrapping addition in place of points: the walk of a lane's slice, the
// destination of every partial and the jobs of the combine pass are taken from the header's functions exactly as gsum.hip.h takes
// them, and every buffer has exactly the size the plan tells the host to reserve.  Checked per case: every term is added exactly once,
// every segment's sum is written exactly once and is right, every partial record that is written is read by exactly one job, no record
// or meta word outside the plan's scratch is touched.  Then one call per refusal of the argument checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gsum_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct Lane { uint32_t key = GSUM_NONE; bool has_head = false; uint64_t head = 0, slot = 0; };

static void model(int group, const std::vector<uint64_t>& offsets, GsumShape shape, const char* what) {
  const size_t nseg = offsets.size() - 1;
  const size_t total = (size_t)offsets[nseg];
  const GsumPlan plan = gsum_plan(group, nseg, total, shape);
  CHECK(plan.ok, "%s: plan refused", what);
  if (!plan.ok) return;
  CHECK(plan.lds <= GSUM_LDS_LIMIT, "%s: LDS %zu", what, plan.lds);
  CHECK(plan.chunk == plan.block * plan.terms && plan.nchunks * plan.chunk >= total && (plan.nchunks == 0 || (plan.nchunks - 1) * plan.chunk < total), "%s: chunk count", what);
  CHECK(plan.combine_grid >= 2 * plan.nchunks && (size_t)plan.combine_grid * plan.block >= nseg, "%s: combine grid", what);
  const unsigned long long* off = (const unsigned long long*)offsets.data();
  const uint32_t ns = (uint32_t)nseg, tot = (uint32_t)total, chunk = plan.chunk, B = plan.block;
  std::vector<uint64_t> w(total), expect(nseg, 0), out(nseg, 0), part(plan.records, 0);
  std::vector<int> visits(total, 0), outw(nseg, 0), partw(plan.records, 0), partr(plan.records, 0), metaw(plan.meta_words, 0);
  std::vector<uint32_t> meta(plan.meta_words, GSUM_NONE);
  for (auto& x : w) x = rnd();
  for (size_t s = 0; s < nseg; s++) for (uint64_t t = offsets[s]; t < offsets[s + 1]; t++) expect[s] += w[t];
  auto write_out = [&](uint32_t s, uint64_t v) { CHECK(s < nseg, "%s: out index %u", what, s); if (s < nseg) { out[s] = v; outw[s]++; } };
  auto write_part = [&](size_t r, uint64_t v) { CHECK(r < plan.records, "%s: record %zu of %zu", what, r, plan.records); if (r < plan.records) { part[r] = v; partw[r]++; } };
  // pass 1
  for (size_t c = 0; c < plan.chunks_grid; c++) {
    const uint32_t cb = (uint32_t)c * chunk, ce = tot - cb < chunk ? tot : cb + chunk;
    std::vector<Lane> lane(B);
    for (uint32_t l = 0; l < B; l++) {
      const uint32_t b = (size_t)cb + (size_t)l * plan.terms < ce ? cb + l * plan.terms : ce, e = ce - b < plan.terms ? ce : b + plan.terms;
      if (b >= e) continue;
      uint32_t s = gsum_seg_of(off, ns, tot, b);
      CHECK(gsum_off(off, ns, tot, s) <= b && b < gsum_off(off, ns, tot, s + 1), "%s: seg_of(%u) = %u", what, b, s);
      const uint32_t first = s;
      uint32_t send = gsum_off(off, ns, tot, s + 1);
      uint64_t acc = 0;
      for (uint32_t t = b; t < e; t++) {
        if (t >= send) {
          const uint32_t so = gsum_off(off, ns, tot, s);
          if (s == first && so < b) {
            if (l == 0) write_part(gsum_record(c, so, cb), acc);
            else { lane[l].head = acc; lane[l].has_head = true; }
          } else {
            write_out(s, acc);
          }
          acc = 0;
          do { s++; send = gsum_off(off, ns, tot, s + 1); } while (t >= send);
        }
        acc += w[t]; visits[t]++;
      }
      lane[l].key = s; lane[l].slot = acc;
      if (l == 0) { CHECK(2 * c < plan.meta_words, "%s: meta", what); meta[2 * c] = gsum_seg_of(off, ns, tot, cb); metaw[2 * c]++; }
      if (e == ce) { CHECK(2 * c + 1 < plan.meta_words, "%s: meta", what); meta[2 * c + 1] = s; metaw[2 * c + 1]++; }
    }
    for (uint32_t l = 0; l + 1 < B; l++)
      if (lane[l].key != GSUM_NONE && lane[l + 1].has_head) {
        CHECK(gsum_seg_of(off, ns, tot, cb + (l + 1) * plan.terms) == lane[l].key, "%s: a head meets another segment", what);
        lane[l].slot += lane[l + 1].head;
      }
    for (uint32_t l = 0; l < B; l++) {
      if (lane[l].key == GSUM_NONE || (l && lane[l - 1].key == lane[l].key)) continue;
      uint64_t sum = 0;
      for (uint32_t k = l; k < B && lane[k].key == lane[l].key; k++) sum += lane[k].slot;
      const uint32_t s = lane[l].key, so = gsum_off(off, ns, tot, s), se = gsum_off(off, ns, tot, s + 1);
      if (gsum_inside(so, se, cb, chunk)) write_out(s, sum);
      else write_part(gsum_record(c, so, cb), sum);
    }
  }
  for (size_t i = 0; i < plan.meta_words; i++) CHECK(metaw[i] == 1, "%s: meta word %zu written %d times", what, i, metaw[i]);
  // pass 2
  size_t jobs = 0;
  for (size_t j = 0; j < plan.combine_grid; j++) {
    for (uint32_t l = 0; l < B; l++) {
      const size_t i = j * B + l;
      if (i < nseg && gsum_off(off, ns, tot, (uint32_t)i) >= gsum_off(off, ns, tot, (uint32_t)i + 1)) write_out((uint32_t)i, 0);
    }
    if (j >= 2 * plan.nchunks) continue;
    const size_t c = j >> 1;
    uint32_t s = 0; size_t c_last = 0;
    if (!gsum_job(off, ns, tot, chunk, c, (int)(j & 1), meta[2 * c], meta[2 * c + 1], &s, &c_last)) continue;
    jobs++;
    CHECK(c_last > c && c_last < plan.nchunks, "%s: job %zu ends in chunk %zu", what, j, c_last);
    uint64_t sum = 0;
    for (size_t k = 0; k <= c_last - c; k++) {
      const size_t r = k ? 2 * (c + k) : j;
      CHECK(r < plan.records && partw[r] == 1, "%s: job %zu reads record %zu that was not written once", what, j, r);
      if (r < plan.records) { sum += part[r]; partr[r]++; }
    }
    write_out(s, sum);
  }
  for (size_t t = 0; t < total; t++) CHECK(visits[t] == 1, "%s: term %zu added %d times", what, t, visits[t]);
  for (size_t s = 0; s < nseg; s++) CHECK(outw[s] == 1 && out[s] == expect[s], "%s: segment %zu written %d times, %s", what, s, outw[s], out[s] == expect[s] ? "right" : "WRONG");
  for (size_t r = 0; r < plan.records; r++) CHECK(partw[r] == partr[r] && partw[r] <= 1, "%s: record %zu written %d, read %d", what, r, partw[r], partr[r]);
  size_t multi = 0;
  for (size_t s = 0; s < nseg; s++) if (offsets[s + 1] > offsets[s] && offsets[s] / chunk != (offsets[s + 1] - 1) / chunk) multi++;
  CHECK(jobs == multi, "%s: %zu jobs for %zu multi-chunk segments", what, jobs, multi);
}

static std::vector<uint64_t> csr(const std::vector<uint64_t>& len) {
  std::vector<uint64_t> o(len.size() + 1, 0);
  for (size_t i = 0; i < len.size(); i++) o[i + 1] = o[i] + len[i];
  return o;
}

static void sweep(int group, GsumShape shape) {
  const uint64_t chunk = (uint64_t)shape.block * shape.terms;
  char what[160];
  for (size_t nseg : {(size_t)0, (size_t)1, (size_t)2, (size_t)1000}) {
    auto go = [&](const char* pat, const std::vector<uint64_t>& len) {
      snprintf(what, sizeof what, "G%d block %d terms %d nseg %zu %s", group, shape.block, shape.terms, nseg, pat);
      model(group, csr(len), shape, what);
    };
    go("all 0", std::vector<uint64_t>(nseg, 0));
    go("all 1", std::vector<uint64_t>(nseg, 1));
    go("all chunk - 1", std::vector<uint64_t>(nseg, chunk - 1));
    go("all chunk", std::vector<uint64_t>(nseg, chunk));
    go("all chunk + 1", std::vector<uint64_t>(nseg, chunk + 1));
    go("all terms + 1", std::vector<uint64_t>(nseg, shape.terms + 1));
    if (!nseg) continue;
    const uint64_t longest = 3 * chunk + 1, everything = 5 * chunk + 3;
    for (size_t at : {(size_t)0, nseg / 2, nseg - 1}) {
      std::vector<uint64_t> len(nseg, 0);
      len[at] = everything;
      go(at == 0 ? "one holds everything (first)" : at == nseg - 1 ? "one holds everything (last)" : "one holds everything (middle)", len);
      std::vector<uint64_t> mix(nseg, 3);
      mix[at] = longest;
      go(at == 0 ? "long first" : at == nseg - 1 ? "long last" : "long in the middle", mix);
    }
    std::vector<uint64_t> r(nseg);
    for (auto& x : r) { const uint64_t k = rnd() % 16; x = k == 0 ? rnd() % (3 * chunk) : k < 4 ? 0 : rnd() % 12; }
    go("random", r);
  }
}

static void refusals() {
  alignas(16) static uint64_t buf[64] = {};
  auto good = [&](bool device) {
    GsumArgs a; a.group = 1; a.xy = buf; a.inf = buf; a.npoints = 4; a.idx = buf; a.offsets = buf; a.nseg = 2; a.total = 3; a.out = buf; a.device = device;
    return a;
  };
  for (bool dev : {false, true}) {
    CHECK(!gsum_check(good(dev)), "a good call is refused: %s", gsum_check(good(dev)));
    GsumArgs a = good(dev); a.nseg = 0; a.total = 0; a.offsets = nullptr; a.out = nullptr; a.xy = nullptr; a.inf = nullptr; a.idx = nullptr;
    CHECK(!gsum_check(a), "nseg == 0 with NULLs is a no-op");
    a = good(dev); a.total = 0; a.xy = nullptr; a.inf = nullptr; a.idx = nullptr; CHECK(!gsum_check(a), "no terms: the points may be NULL");
    a = good(dev); a.xy = nullptr; CHECK(gsum_check(a), "NULL xy with terms");
    a = good(dev); a.inf = nullptr; CHECK(gsum_check(a), "NULL infinity with terms");
    a = good(dev); a.offsets = nullptr; CHECK(gsum_check(a), "NULL offsets");
    a = good(dev); a.out = nullptr; CHECK(gsum_check(a), "NULL out");
    a = good(dev); a.total = GSUM_MAX_TOTAL + 1; a.npoints = GSUM_MAX_POINTS - 1; CHECK(gsum_check(a), "total > 2^28");
    a = good(dev); a.total = GSUM_MAX_TOTAL; a.npoints = 4; CHECK(!gsum_check(a), "total == 2^28 with idx");
    a = good(dev); a.total = ~(uint64_t)0; CHECK(gsum_check(a), "total = 2^64 - 1");
    a = good(dev); a.nseg = GSUM_MAX_SEGS + 1; CHECK(gsum_check(a), "nseg > 2^28");
    a = good(dev); a.nseg = ~(uint64_t)0; CHECK(gsum_check(a), "nseg = 2^64 - 1: (nseg + 1) * 8 would wrap");
    a = good(dev); a.npoints = GSUM_MAX_POINTS; CHECK(gsum_check(a), "npoints == 2^32");
    a = good(dev); a.npoints = GSUM_MAX_POINTS - 1; CHECK(!gsum_check(a), "npoints == 2^32 - 1");
    a = good(dev); a.idx = nullptr; a.total = 5; CHECK(gsum_check(a), "no idx and total > npoints");
    a = good(dev); a.idx = nullptr; a.total = 4; CHECK(!gsum_check(a), "no idx and total == npoints");
    a = good(dev); a.group = 3; CHECK(gsum_check(a), "group 3");
  }
  const char* p = (const char*)buf;
  GsumArgs a = good(true); a.xy = p + 4; CHECK(gsum_check(a), "misaligned d_xy");
  a = good(true); a.offsets = p + 4; CHECK(gsum_check(a), "misaligned d_offsets");
  a = good(true); a.out = p + 2; CHECK(gsum_check(a), "misaligned d_out");
  a = good(true); a.idx = p + 2; CHECK(gsum_check(a), "misaligned d_idx");
  a = good(false); a.xy = p + 4; a.idx = p + 2; CHECK(!gsum_check(a), "host pointers need no alignment");
  // what only the host forms see
  const uint32_t idx[5] = {0, 3, 3, 1, 2};
  { const uint64_t o[3] = {0, 2, 5}; CHECK(!gsum_check_host(o, 2, 5, idx, 4), "good offsets"); CHECK(!gsum_check_host(o, 2, 5, nullptr, 5), "good offsets, no idx"); }
  { const uint64_t o[3] = {0, 3, 2}; CHECK(gsum_check_host(o, 2, 2, idx, 4), "decreasing offsets"); }
  { const uint64_t o[3] = {1, 2, 5}; CHECK(gsum_check_host(o, 2, 5, idx, 4), "offsets[0] != 0"); }
  { const uint64_t o[3] = {0, 2, 4}; CHECK(gsum_check_host(o, 2, 5, idx, 4), "offsets[nseg] != total"); }
  { const uint64_t o[3] = {0, ~(uint64_t)0, 5}; CHECK(gsum_check_host(o, 2, 5, idx, 4), "an offset of 2^64 - 1 in the middle"); }
  { const uint64_t o[3] = {0, (uint64_t)1 << 63, ~(uint64_t)0}; GsumArgs b = good(false); b.total = o[2]; CHECK(gsum_check(b), "offsets up to 2^64 - 1: total is refused first"); }
  { const uint64_t o[3] = {0, 2, 5}; CHECK(gsum_check_host(o, 2, 5, idx, 3), "an index == npoints"); const uint32_t big[5] = {0, 1, 0xffffffffu, 1, 2}; CHECK(gsum_check_host(o, 2, 5, big, 4), "an index of 2^32 - 1"); }
  CHECK(!gsum_check_host(nullptr, 0, 0, nullptr, 0), "nseg == 0 reads nothing");
  // the device's reading of offsets it cannot refuse: clamped, the two ends forced, never an index outside [0, nseg)
  { const unsigned long long o[5] = {7, ~0ull, 3, 1ull << 40, 0};
    CHECK(gsum_off(o, 4, 10, 0) == 0 && gsum_off(o, 4, 10, 1) == 10 && gsum_off(o, 4, 10, 2) == 3 && gsum_off(o, 4, 10, 3) == 10 && gsum_off(o, 4, 10, 4) == 10, "clamping");
    for (uint32_t t = 0; t < 10; t++) CHECK(gsum_seg_of(o, 4, 10, t) < 4, "seg_of stays inside");
  }
  // the plan's own refusals
  CHECK(!gsum_plan(1, 1, GSUM_MAX_TOTAL + 1).ok && !gsum_plan(1, GSUM_MAX_SEGS + 1, 0).ok && !gsum_plan(3, 1, 1).ok, "plan sizes");
  CHECK(!gsum_plan(1, 1, 1, GsumShape{3, 8}).ok && !gsum_plan(1, 1, 1, GsumShape{256, 0}).ok && !gsum_plan(2, 1, 1, GsumShape{256, 8}).ok, "plan shapes (G2 at 256 lanes is past 64 KB of LDS)");
  const GsumPlan big = gsum_plan(1, GSUM_MAX_SEGS, GSUM_MAX_TOTAL);
  CHECK(big.ok && big.nchunks == GSUM_MAX_TOTAL / big.chunk && big.combine_grid == GSUM_MAX_SEGS / big.block && big.part_bytes == big.records * 176, "the largest call");
}

int main() {
  printf("plans\n");
  sweep(1, GsumShape{4, 2});
  sweep(2, GsumShape{4, 2});
  sweep(1, GsumShape{1, 1});
  sweep(1, GsumShape{64, 8});
  sweep(1, gsum_shape(1));
  sweep(2, gsum_shape(2));
  printf("refusals\n");
  refusals();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
