// tests/cpp/fr_frac_plan_main.cpp -- csrc/fr_frac_plan.h (and fr_scan_plan.h under it) on their own: a stand-alone program, built with
// -fsanitize=address,undefined -fno-sanitize-recover by tests/test_fr_frac_plan.py and run directly.  It sweeps (op, c, len, k, pitch)
// over the shipped shapes and small ones, 64-bit-overflowing products included, and checks of every accepted plan that each step's
// reach -- the elements its grid covers, the records it reads and writes -- stays inside the sizes the plan itself reports, and of
// every out-of-range argument that it is refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "fr_frac_plan.h"

using namespace bls;

static long checks = 0;
#define REQUIRE(c) do { checks++; if (!(c)) { std::printf("FAILED: %s (line %d) op=%d c=%d len=%zu k=%zu pitch=%zu\n", #c, __LINE__, g_op, g_c, g_len, g_k, g_pitch); std::exit(1); } } while (0)
static int g_op, g_c;
static size_t g_len, g_k, g_pitch;

static bool mul_fits(size_t a, size_t b, size_t limit) { return a == 0 || b <= limit / a; }

// what the plan must do with these arguments, from the contract alone
static bool acceptable(int op, int c, size_t len, size_t k, size_t pitch) {
  if (op < 0 || op > 1 || c < 1 || c > FRF_MAX_COLS) return false;
  if (!len || !k) return true;
  if (!mul_fits(len, k, FRS_MAX_TOTAL)) return false;
  const size_t total = len * k;
  if (pitch < total || pitch > FRS_MAX_TOTAL) return false;
  return (size_t)(c - 1) * pitch + total <= FRS_MAX_TOTAL;
}

static void check_plan(const FrFracPlan& p, int op, int c, size_t len, size_t k, size_t pitch, bool shipped) {
  g_op = op; g_c = c; g_len = len; g_k = k; g_pitch = pitch;
  const bool want = acceptable(op, c, len, k, pitch);
  if (!want) { REQUIRE(p.n_steps == -1); return; }
  if (!len || !k) { REQUIRE(p.n_steps == 0); return; }
  const size_t total = len * k, tile = (size_t)p.shape.block * p.shape.chunk;
  if (p.n_steps == -1) {                                          // only a small shape may fail to reach: tile^3 < total
    REQUIRE(!shipped && tile * tile * tile < total);
    return;
  }
  REQUIRE(p.n_steps == 1 || p.n_steps == 3 || p.n_steps == 5);
  REQUIRE(p.total == total && p.tile == tile && p.table_reach == (size_t)(c - 1) * pitch + total && p.table_reach <= FRS_MAX_TOTAL);
  const size_t tiles = (total + tile - 1) / tile;
  const FrScanStep& f = p.step[0];
  REQUIRE(f.kernel == FRF_K_FRONT && f.grid == tiles && f.block == (unsigned)p.shape.block && f.items == total);
  REQUIRE(f.lds == frs_lds_bytes(p.shape) && f.lds >= ((size_t)p.shape.block * (p.shape.chunk * 8 + 4) + (size_t)(p.shape.block / 64) * 8) * 4);
  if (shipped) REQUIRE(f.lds <= FRF_LDS_LIMIT && p.shape.chunk <= FRF_CHUNK_MAX && p.shape.block == FRS_BLOCK);
  REQUIRE((size_t)f.grid * tile >= total && (size_t)(f.grid - 1) * tile < total);
  if (p.n_steps == 1) {
    REQUIRE(f.src == FRS_K_SINGLE && tiles == 1 && f.dst == FRS_BUF_NONE);
    for (int i = 0; i < 5; i++) REQUIRE(p.recs[i] == 0);
    return;
  }
  REQUIRE(f.src == FRS_K_REDUCE && f.dst == FRS_BUF_AGG0 && p.recs[FRS_BUF_AGG0] >= f.grid && p.recs[FRS_BUF_LANE] >= (size_t)f.grid * f.block);
  for (int i = 1; i < p.n_steps; i++) {
    const FrScanStep& s = p.step[i];
    REQUIRE(s.block == (unsigned)p.shape.block && s.grid >= 1);
    if (s.kernel == FRS_K_SCAN) {
      REQUIRE(i == p.n_steps - 1 && s.grid == f.grid && s.items == total && s.lds == f.lds);
      REQUIRE(s.carry >= 0 && p.recs[s.carry] >= s.grid && p.recs[FRS_BUF_LANE] >= (size_t)s.grid * s.block);
      continue;
    }
    REQUIRE(s.kernel == FRS_K_AGG_REDUCE || s.kernel == FRS_K_AGG_SCAN);
    REQUIRE(s.lds == frs_agg_lds_bytes(p.shape));
    REQUIRE(s.src >= 0 && p.recs[s.src] >= s.items);               // the records it reads
    REQUIRE((size_t)s.grid * tile >= s.items && (size_t)(s.grid - 1) * tile < s.items);
    REQUIRE(s.dst >= 0 && p.recs[s.dst] >= (s.kernel == FRS_K_AGG_REDUCE ? (size_t)s.grid : s.items));      // ... and writes
    if (s.carry >= 0) REQUIRE(p.recs[s.carry] >= s.grid);
    else if (s.kernel == FRS_K_AGG_SCAN) REQUIRE(s.grid == 1);    // without a carry-in one workgroup scans everything
  }
  // every record a later step reads was written by an earlier one
  REQUIRE(p.step[1].src == FRS_BUF_AGG0 && p.step[1].items == tiles);
  if (p.n_steps == 5) {
    REQUIRE(p.step[1].kernel == FRS_K_AGG_REDUCE && p.step[1].dst == FRS_BUF_AGG1 && p.step[2].src == FRS_BUF_AGG1 && p.step[2].dst == FRS_BUF_CARRY1);
    REQUIRE(p.step[3].src == FRS_BUF_AGG0 && p.step[3].carry == FRS_BUF_CARRY1 && p.step[3].dst == FRS_BUF_CARRY0 && p.step[4].carry == FRS_BUF_CARRY0);
    REQUIRE(p.step[2].items == p.step[1].grid && p.step[3].grid == p.step[1].grid);
  } else {
    REQUIRE(p.step[1].kernel == FRS_K_AGG_SCAN && p.step[1].dst == FRS_BUF_CARRY0 && p.step[2].carry == FRS_BUF_CARRY0);
  }
}

int main() {
  const size_t M = FRS_MAX_TOTAL;
  const size_t lens[] = {0, 1, 2, 3, 63, 64, 100, 511, 512, 513, 1023, 1024, 1025, 2048, 4097, (size_t)1 << 16, ((size_t)1 << 20) - 1, (size_t)1 << 20, ((size_t)1 << 20) + 1,
                         (size_t)1 << 24, M / 8, M / 3, M - 1, M, M + 1, (size_t)1 << 32, ((size_t)1 << 63) + 5, ~(size_t)0};
  const size_t ks[] = {0, 1, 2, 3, 7, 256, 1048, 4096, (size_t)1 << 20, M, M + 1, (size_t)1 << 32, ((size_t)1 << 63) + 1, ~(size_t)0};
  // the shipped shapes
  for (int op = -1; op <= 2; op++)
    for (int c = -1; c <= FRF_MAX_COLS + 1; c++)
      for (size_t len : lens)
        for (size_t k : ks) {
          const bool fits = mul_fits(len, k, M);
          const size_t total = fits ? len * k : 0;
          const size_t pitches[] = {total, total + 1, total ? total - 1 : 0, 2 * total + 5, M, M + 1, ~(size_t)0};
          for (size_t pitch : pitches) check_plan(fr_frac_plan(op, c, len, k, pitch), op, c, len, k, pitch, true);
        }
  std::printf("shipped\n");
  // the chosen tiles: LDS for two workgroups per CU, fewer elements per lane for the wide fraction sums, every admissible total within reach
  for (int op = 0; op <= 1; op++)
    for (int c = 1; c <= FRF_MAX_COLS; c++) {
      g_op = op; g_c = c;
      const FrScanShape s = frf_shape(op, c);
      const size_t tile = (size_t)s.block * s.chunk;
      REQUIRE(s.block == FRS_BLOCK && s.chunk >= 1 && s.chunk <= FRF_CHUNK_MAX && 2 * frs_lds_bytes(s) <= 160 * 1024);
      REQUIRE(c == 1 || frf_shape(op, c).chunk <= frf_shape(op, c - 1).chunk);
      REQUIRE(tile * tile * tile >= M / (size_t)c);               // (c - 1) * pitch + total <= 2^28 bounds the total by 2^28 / c
      REQUIRE(fr_frac_plan(op, c, M / c, 1, M / c).n_steps == 5);
    }
  std::printf("tiles\n");
  // small shapes: the three branches within a few thousand elements, and shapes the plan must refuse
  const int blocks[] = {64, 128, 256}, chunks[] = {1, 2, 3, 4};
  for (int b : blocks)
    for (int ch : chunks)
      for (int op = 0; op <= 1; op++)
        for (size_t total : {(size_t)1, (size_t)b * ch - 1, (size_t)b * ch, (size_t)b * ch + 1, (size_t)b * ch * b * ch, (size_t)b * ch * b * ch + 1, (size_t)b * ch * b * ch * 3 + 7, M})
          for (size_t k : {(size_t)1, (size_t)3, (size_t)100}) {
            const size_t len = (total + k - 1) / k;
            if (!mul_fits(len, k, M)) continue;
            check_plan(fr_frac_plan(op, 3, len, k, len * k, FrScanShape{b, ch}), op, 3, len, k, len * k, false);
          }
  for (const FrScanShape s : {FrScanShape{0, 2}, FrScanShape{32, 2}, FrScanShape{96, 2}, FrScanShape{64, 0}, FrScanShape{64, FRF_CHUNK_MAX + 1}, FrScanShape{1024, 4}}) {
    g_op = 0; g_c = 1;
    REQUIRE(fr_frac_plan(0, 1, 10, 10, 100, s).n_steps == -1);
  }
  std::printf("small\n");
  std::printf("%ld checks\nall ok\n", checks);
  return 0;
}
