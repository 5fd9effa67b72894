// tests/cpp/fr_lagrange_plan_main.cpp -- bls12_381_amd/csrc/fr_lagrange_plan.h on its own (tests/test_fr_lagrange_plan.py builds this
// with host clang++ -fsanitize=address,undefined and runs it; it includes nothing of the library but that header).
//
// The launch is walked as a MODEL: workgroups, teams, lanes, passes and tiles are taken from the header's functions exactly as
// fr_lagrange.hip.h takes them, and every buffer has exactly the size the plan tells the host to reserve.  Checked per case: every
// segment belongs to exactly one team, every node of it to exactly one (lane, k), every (node, tile) pair is visited exactly once and
// the tiles cover the segment once, a team's LDS lies inside the workgroup's, every scratch slot lies inside what the plan reserves, a
// segment that breaks the offsets contract is refused by flg_segment.  Then one call per refusal of the argument checks.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fr_lagrange_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

static uint64_t g_rng = 0x13198a2e03707344ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static void model(const std::vector<uint32_t>& offsets, uint32_t total, bool want_lambda, FlgShape shape, const char* what) {
  const size_t nseg = offsets.size() - 1;
  const FlgPlan plan = flg_plan(nseg, total, want_lambda, shape);
  CHECK(plan.ok, "%s: plan refused", what);
  if (!plan.ok) return;
  CHECK(plan.lds <= FLG_LDS_LIMIT, "%s: LDS %zu", what, plan.lds);
  CHECK(plan.teams * plan.team == plan.block && (size_t)plan.grid * plan.teams >= nseg && (nseg == 0 || (size_t)(plan.grid - 1) * plan.teams < nseg), "%s: grid", what);
  CHECK((plan.shape == FLG_SHAPE_BLOCK) == (plan.team == plan.block), "%s: shape", what);
  CHECK(plan.pre_bytes == (nseg ? (size_t)total * 32 : 0) && plan.work_bytes == (want_lambda || !nseg ? 0 : (size_t)total * 32), "%s: scratch", what);
  std::vector<uint8_t> pre(plan.pre_bytes), work(plan.work_bytes);
  std::vector<int> seg_seen(nseg, 0), owner(total, 0);
  for (unsigned g = 0; g < plan.grid; g++)
    for (unsigned tm = 0; tm < plan.teams; tm++) {
      const size_t s = (size_t)g * plan.teams + tm;
      if (s >= nseg) continue;
      seg_seen[s]++;
      const size_t lds_end = ((size_t)tm + 1) * flg_team_lds_words(plan.team, plan.tile) * 4;
      CHECK(lds_end <= plan.lds, "%s: team %u LDS ends at %zu of %zu", what, tm, lds_end, plan.lds);
      uint32_t so = 0, t = 0;
      const bool good = offsets[s + 1] >= offsets[s] && offsets[s + 1] - offsets[s] <= FLG_LEN_MAX && offsets[s + 1] <= total;
      CHECK(flg_segment(offsets.data(), total, s, &so, &t) == good, "%s: flg_segment(%zu)", what, s);
      if (!good) continue;
      CHECK(so == offsets[s] && t == offsets[s + 1] - offsets[s], "%s: segment %zu", what, s);
      const uint32_t passes = flg_passes(t, plan.team, plan.r), tiles = flg_tiles(t, plan.tile);
      // the tiles cover [0, t) once
      uint32_t covered = 0;
      for (uint32_t q = 0; q < tiles; q++) { const uint32_t base = q * plan.tile, left = t - base; CHECK(base < t, "%s: empty tile", what); covered += left < plan.tile ? left : plan.tile; }
      CHECK(covered == t, "%s: tiles cover %u of %u", what, covered, t);
      std::vector<int> pair((size_t)t * (tiles ? tiles : 1), 0);
      uint32_t counted = 0;
      for (uint32_t l = 0; l < plan.team; l++) {
        uint32_t mine = 0;
        for (uint32_t p = 0; p < passes; p++)
          for (uint32_t r = 0; r < plan.r; r++) {
            const uint32_t i = flg_node(p * plan.r + r, l, plan.team);
            if (i >= t) continue;
            mine++;
            for (uint32_t q = 0; q < tiles; q++) pair[(size_t)i * tiles + q]++;
            const size_t slot = ((size_t)so + i) * 32;
            CHECK(slot + 32 <= pre.size(), "%s: pre slot %zu of %zu", what, slot, pre.size());
            if (slot + 32 <= pre.size()) pre[slot] = 1;
            if (!want_lambda) { CHECK(slot + 32 <= work.size(), "%s: work slot %zu of %zu", what, slot, work.size()); if (slot + 32 <= work.size()) work[slot] = 1; }
            owner[so + i]++;
          }
        CHECK(mine == flg_count(t, l, plan.team), "%s: lane %u owns %u, flg_count says %u", what, l, mine, flg_count(t, l, plan.team));
        for (uint32_t k = 0; k < mine; k++) CHECK(flg_node(k, l, plan.team) < t, "%s: node %u of lane %u", what, k, l);
        counted += mine;
      }
      CHECK(counted == t, "%s: %u of %u nodes owned", what, counted, t);
      for (size_t k = 0; k < pair.size() && t; k++) CHECK(pair[k] == 1, "%s: (node, tile) pair %zu visited %d times", what, k, pair[k]);
    }
  for (size_t s = 0; s < nseg; s++) CHECK(seg_seen[s] == 1, "%s: segment %zu met %d teams", what, s, seg_seen[s]);
  // (with valid offsets every node belongs to one segment)
  bool valid = offsets[0] == 0 && offsets[nseg] == total;
  for (size_t s = 0; s < nseg && valid; s++) valid = offsets[s] <= offsets[s + 1] && offsets[s + 1] - offsets[s] <= FLG_LEN_MAX;
  if (valid) for (uint32_t i = 0; i < total; i++) CHECK(owner[i] == 1, "%s: node %u owned %d times", what, i, owner[i]);
}

static std::vector<uint32_t> equal_lengths(size_t nseg, uint32_t len) {
  std::vector<uint32_t> o(nseg + 1, 0);
  for (size_t s = 0; s < nseg; s++) o[s + 1] = o[s] + len;
  return o;
}

static void sweep(FlgShape shape, const char* name) {
  char what[160];
  const uint32_t tile = (uint32_t)shape.tile;
  const size_t nsegs[] = {0, 1, 2, 1000};
  const uint32_t lens[] = {0, 1, tile - 1, tile, tile + 1, FLG_LEN_MAX};
  for (size_t nseg : nsegs) {
    for (uint32_t len : lens) {
      if (len == FLG_LEN_MAX && nseg == 1000) continue;          // (2 x 4096 is the same walk)
      const std::vector<uint32_t> o = equal_lengths(nseg, len);
      snprintf(what, sizeof what, "%s nseg %zu len %u", name, nseg, len);
      model(o, o[nseg], true, shape, what);
      model(o, o[nseg], false, shape, what);
    }
    for (int mix = 0; mix < 3; mix++) {
      std::vector<uint32_t> o(nseg + 1, 0);
      for (size_t s = 0; s < nseg; s++) {
        const uint64_t k = rnd() % 8;
        // (a long segment among 1000 would only repeat the walk of the 4096 above, a (node, tile) pair at a time)
        const uint32_t len = k == 0 ? 0 : k == 1 && (nseg <= 2 || s % 250 == 7) ? (uint32_t)(rnd() % (FLG_LEN_MAX + 1)) : (uint32_t)(rnd() % (3 * tile + 2));
        o[s + 1] = o[s] + (len > FLG_LEN_MAX ? FLG_LEN_MAX : len);
      }
      snprintf(what, sizeof what, "%s nseg %zu mix %d", name, nseg, mix);
      model(o, o[nseg], mix != 1, shape, what);
    }
  }
  // what only the device sees: decreasing, too long, beyond total
  const std::vector<uint32_t> bad = {0, 6, 4, 4101, 4110, 4130, 4127, 0xffffffffu, 7};
  snprintf(what, sizeof what, "%s bad segments", name);
  model(bad, 4127, true, shape, what);
}

int main() {
  printf("plans\n");
  sweep(flg_shape(1, 4096, FLG_SHAPE_BLOCK), "shipped block");
  sweep(flg_shape(1, 64, FLG_SHAPE_WAVE), "shipped wave 64");
  sweep(flg_shape(1, 8, FLG_SHAPE_WAVE), "shipped wave 8");
  sweep(FlgShape{4, 4, 4, 2, 4}, "tiny block");
  sweep(FlgShape{8, 4, 4, 2, 4}, "tiny wave");
  sweep(FlgShape{64, 16, 24, 3, 64}, "odd tile");
  {  // the choice between the shapes is a function of (nseg, total)
    FlgShape a = flg_shape(2048, 2048 * 512, FLG_AUTO), b = flg_shape(1 << 16, 8 << 16, FLG_AUTO), c = flg_shape(100, 4000, FLG_AUTO), d = flg_shape(0, 0, FLG_AUTO);
    CHECK(a.team == a.block && a.tile == FLG_TILE, "2048 x 512 must take the BLOCK shape");
    CHECK(b.team == 8 && b.tile == 8 && b.block == FLG_BLOCK, "2^16 x 8 must take teams of 8");
    CHECK(c.team == 64 && c.tile == 64, "100 x 40 must take teams of 64");
    CHECK(flg_shape_ok(d) && d.team == 8, "an empty call still has a shape");
    CHECK(flg_shape(8, 8 * 513, FLG_SHAPE_WAVE).team == 64 && flg_shape(1 << 12, 8 << 12, FLG_SHAPE_BLOCK).team == FLG_BLOCK, "forced shapes");
    CHECK(flg_shape_from(nullptr) == FLG_AUTO && flg_shape_from("block") == FLG_SHAPE_BLOCK && flg_shape_from("wave") == FLG_SHAPE_WAVE && flg_shape_from("x") == FLG_AUTO, "shape names");
    CHECK(flgc_block(1, 2048, 2048 * 512) == 256 && flgc_block(2, 2048, 2048 * 512) == 128 && flgc_block(1, 1 << 16, 8 << 16) == 64 && flgc_block(2, 0, 0) == 64, "sum blocks");
  }
  printf("refusals\n");
  {
    alignas(16) static unsigned char buf[4096];
    const void* p = buf;
    auto args = [&]() { FlgArgs a; a.nodes = buf; a.offsets = buf + 512; a.nseg = 2; a.total = 8; a.points = buf + 640; a.values = buf + 1024; a.lambda = buf + 2048; a.y = buf + 3072;
                        a.flags = buf + 3200; a.device = true; return a; };
    FlgArgs a = args();
    CHECK(!flg_check(a), "a good call: %s", flg_check(a));
    a = args(); a.nseg = FLG_MAX_SEGS + 1; CHECK(flg_check(a), "nseg over the limit");
    a = args(); a.nseg = ~(uint64_t)0; CHECK(flg_check(a), "nseg 2^64 - 1");
    a = args(); a.total = FLG_MAX_TOTAL + 1; CHECK(flg_check(a), "total over the limit");
    a = args(); a.total = ~(uint64_t)0; CHECK(flg_check(a), "total 2^64 - 1");
    a = args(); a.nseg = 0; CHECK(flg_check(a), "nodes without a segment");
    a = args(); a.nseg = 0; a.total = 0; a.nodes = a.offsets = a.lambda = a.y = nullptr; CHECK(!flg_check(a), "nseg == 0 is a no-op");
    a = args(); a.offsets = nullptr; CHECK(flg_check(a), "NULL offsets");
    a = args(); a.nodes = nullptr; CHECK(flg_check(a), "NULL nodes");
    a = args(); a.values = nullptr; CHECK(flg_check(a), "y without values");
    a = args(); a.lambda = a.y = nullptr; CHECK(flg_check(a), "neither lambda nor y");
    a = args(); a.lambda = a.y = nullptr; a.lambda_in_scratch = true; CHECK(!flg_check(a), "the combines keep lambda in scratch");
    a = args(); a.points = nullptr; a.values = nullptr; a.y = nullptr; a.flags = nullptr; CHECK(!flg_check(a), "the optional arrays");
    a = args(); a.nodes = buf + 8; CHECK(flg_check(a), "misaligned nodes");
    a = args(); a.points = buf + 648; CHECK(flg_check(a), "misaligned points");
    a = args(); a.values = buf + 1028; CHECK(flg_check(a), "misaligned values");
    a = args(); a.lambda = buf + 2052; CHECK(flg_check(a), "misaligned lambda");
    a = args(); a.y = buf + 3080; CHECK(flg_check(a), "misaligned y");
    a = args(); a.offsets = buf + 514; CHECK(flg_check(a), "misaligned offsets");
    a = args(); a.device = false; a.nodes = buf + 8; a.lambda = buf + 2052; CHECK(!flg_check(a), "the host form takes any alignment");
    a = args(); a.lambda = buf; CHECK(flg_check(a), "lambda on the nodes");
    a = args(); a.lambda = buf + 1024 + 7 * 32 - 16; a.device = false; CHECK(flg_check(a), "lambda on the end of the values");
    a = args(); a.y = buf + 640; CHECK(flg_check(a), "y on the points");
    a = args(); a.flags = buf + 512 + 11; CHECK(flg_check(a), "flags on the offsets");
    a = args(); a.y = buf + 2048 + 7 * 32; CHECK(flg_check(a), "y on the end of lambda");
    a = args(); a.flags = buf + 3072 + 63; CHECK(flg_check(a), "flags on the end of y");
    (void)p;
    const uint32_t good[] = {0, 3, 3, 8}, nonzero[] = {1, 3, 3, 8}, dec[] = {0, 5, 3, 8}, longs[] = {0, 4097, 4097, 4100}, edge[] = {0, 4096, 4096, 4100};
    CHECK(!flg_check_host(good, 3, 8) && !flg_check_host(edge, 3, 4100) && !flg_check_host(nullptr, 0, 0), "good offsets");
    CHECK(flg_check_host(nonzero, 3, 8), "offsets[0] != 0");
    CHECK(flg_check_host(dec, 3, 8), "decreasing offsets");
    CHECK(flg_check_host(longs, 3, 4100), "a segment of 4097");
    CHECK(flg_check_host(good, 3, 9), "total != offsets[nseg]");
    auto cargs = [&]() { FlgcArgs c; c.group = 1; c.xy = buf; c.inf = buf + 1000; c.nodes = buf + 1024; c.offsets = buf + 1536; c.nseg = 2; c.total = 8; c.points = buf + 1600;
                         c.out = buf + 2048; c.flags = buf + 2400; c.device = true; return c; };
    FlgcArgs c = cargs();
    CHECK(!flgc_check(c), "a good combine: %s", flgc_check(c));
    c = cargs(); c.group = 3; CHECK(flgc_check(c), "group 3");
    c = cargs(); c.out = nullptr; CHECK(flgc_check(c), "NULL output");
    c = cargs(); c.xy = nullptr; CHECK(flgc_check(c), "NULL shares");
    c = cargs(); c.inf = nullptr; CHECK(flgc_check(c), "NULL infinity bytes");
    c = cargs(); c.xy = buf + 4; CHECK(flgc_check(c), "misaligned shares");
    c = cargs(); c.out = buf + 2052; CHECK(flgc_check(c), "misaligned output");
    c = cargs(); c.nodes = buf + 1032; CHECK(flgc_check(c), "misaligned nodes");
    c = cargs(); c.out = buf + 8 * 96 - 8; CHECK(flgc_check(c), "the output on the end of the shares");
    c = cargs(); c.flags = buf + 1000 + 7; CHECK(flgc_check(c), "the flags on the infinity bytes");
    c = cargs(); c.flags = buf + 2048 + 2 * 144 - 1; CHECK(flgc_check(c), "the flags on the end of the output");
    c = cargs(); c.total = FLG_MAX_TOTAL + 1; CHECK(flgc_check(c), "total over the limit");
    c = cargs(); c.nseg = 0; c.total = 0; c.out = nullptr; CHECK(!flgc_check(c), "nseg == 0 is a no-op");
    // shapes the plan refuses
    CHECK(!flg_plan(1, 1, true, FlgShape{256, 96, 64, 4, 64}).ok, "a team that is no power of two");
    CHECK(!flg_plan(1, 1, true, FlgShape{256, 128, 64, 4, 64}).ok, "a WAVE team wider than the wavefront");
    CHECK(!flg_plan(1, 1, true, FlgShape{256, 256, 4096, 4, 64}).ok, "more LDS than a kernel gets");
    CHECK(!flg_plan(1, 1, true, FlgShape{256, 256, 512, 0, 64}).ok && !flg_plan(1, 1, true, FlgShape{2048, 2048, 512, 4, 64}).ok, "r and block out of range");
    CHECK(!flg_plan(FLG_MAX_SEGS + 1, 1, true).ok && !flg_plan(1, FLG_MAX_TOTAL + 1, true).ok && !flg_plan(~(size_t)0, ~(size_t)0, false).ok, "sizes out of range");
    CHECK(flg_plan(FLG_MAX_SEGS, FLG_MAX_TOTAL, false).ok && flg_plan(0, 0, true).grid == 0, "the limits themselves");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
