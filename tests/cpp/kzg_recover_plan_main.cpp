// tests/cpp/kzg_recover_plan_main.cpp -- bls12_381_amd/csrc/kzg_recover_plan.h on its own (tests/test_kzg_recover_plan.py builds this with
// host clang++ -fsanitize=address,undefined and runs it; it includes nothing of the library but that header and, to compare the maps,
// kzg_plan.h).
//
// Checked for every (log_n <= 8, log_l <= log_n), both orders and count in {0, 1, 3}: the map natural index -> (cell, entry) is the
// inverse of kzg_cell_src and a bijection, the residue of a cell is the index of its entries mod 2c, the scatter's tiles read every
// (residue, entry) once and write every scalar of EZ once inside the working vector, every scratch range lies inside what the plan
// reserves and none overlaps another, every grid covers its items; the effective offsets and the host-form checks on a few offset
// arrays.  Then one call per refusal of the argument checks, 64-bit extremes included.  The maps are printed for the Python side.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kzg_plan.h"
#include "kzg_recover_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

static void maps_model(int log_n, int log_l, int order) {
  const int log_c = log_n - log_l;
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, c2 = (uint64_t)2 << log_c;
  std::vector<int> hit(2 * n, 0);
  for (uint64_t i = 0; i < c2; i++) {
    const uint64_t rho = kzgr_residue(i, log_c, order);
    CHECK(rho < c2 && kzgr_cell_of_residue(rho, log_c, order) == i, "(%d, %d) order %d: residue of cell %llu", log_n, log_l, order, (unsigned long long)i);
    for (uint64_t t = 0; t < l; t++) {
      const uint64_t j = kzg_cell_src(i, t, log_c, log_l, order);
      CHECK(j < 2 * n, "(%d, %d) order %d: cell source", log_n, log_l, order);
      if (j >= 2 * n) continue;
      hit[j]++;
      CHECK(kzgr_index_of(i, t, log_c, log_l, order) == j, "(%d, %d) order %d: index_of is not kzg_cell_src", log_n, log_l, order);
      CHECK(kzgr_cell_of(j, log_c, order) == i && kzgr_entry_of(j, log_c, log_l, order) == t, "(%d, %d) order %d: the map is not the inverse at (%llu, %llu)", log_n, log_l, order,
            (unsigned long long)i, (unsigned long long)t);
      CHECK((j & (c2 - 1)) == rho, "(%d, %d) order %d: an entry of cell %llu outside its residue", log_n, log_l, order, (unsigned long long)i);
    }
    if (log_n <= 4) printf("map %d %d %d %llu %llu %llu\n", log_n, log_l, order, (unsigned long long)i, (unsigned long long)rho, (unsigned long long)kzg_cell_src(i, l - 1, log_c, log_l, order));
  }
  for (uint64_t j = 0; j < 2 * n; j++) CHECK(hit[j] == 1, "(%d, %d) order %d: the map is no bijection", log_n, log_l, order);
}

static void plan_model(int log_n, int log_l, uint64_t count, int order, bool coef, unsigned tile) {
  char what[112];
  snprintf(what, sizeof what, "(%d, %d) x %llu order %d coef %d tile %u", log_n, log_l, (unsigned long long)count, order, (int)coef, tile);
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, c = n >> log_l, m = count * (c + 1);
  const KzgrPlan p = kzgr_plan(log_n, log_l, count, m, coef, tile);
  CHECK(p.ok, "%s: refused", what);
  if (!p.ok) return;
  CHECK(p.n == n && p.l == l && p.cells == 2 * c && p.scalars == count * 2 * n && p.tables == count * 2 * c && p.log_c == log_n - log_l, "%s: shape", what);
  if (!count) { CHECK(p.bytes == 0 && p.slots_grid == 0 && p.scatter_grid == 0, "%s: count = 0 reserves and launches nothing", what); return; }
  // the scratch: every range inside the block, in order, none overlapping the next
  const struct { const char* name; size_t at; uint64_t bytes; } r[9] = {{"eff", p.eff, (count + 1) * 4}, {"mis", p.mis, count + 1}, {"slot", p.slot, p.tables * 4}, {"status", p.status, count * 4},
    {"upper", p.upper, count * 4}, {"zd", p.zd, p.tables * 32}, {"zc", p.zc, p.tables * 32}, {"work", p.work, p.scalars * 32}, {"coef", p.coef, coef ? count * n * 32 : 0}};
  for (int i = 0; i < 9; i++) {
    CHECK(r[i].at % 256 == 0 && r[i].at + r[i].bytes <= p.bytes, "%s: %s leaves the block", what, r[i].name);
    if (i + 1 < 9) CHECK(r[i].at + r[i].bytes <= r[i + 1].at, "%s: %s overlaps %s", what, r[i].name, r[i + 1].name);
  }
  // the root tables: a block of their own, of one size whatever the shape
  CHECK(p.rootd + p.cells * 32 <= p.rootc && p.rootc + p.cells * 32 <= p.roots_bytes && p.roots_bytes == ((size_t)64 << KZGR_MAX_LOG_CELLS), "%s: the root tables", what);
  // the grids
  CHECK(p.offsets_grid == 1 && p.slots_grid == count, "%s: offsets / slots grids", what);
  CHECK((uint64_t)p.roots_grid * KZGR_BLOCK >= p.cells, "%s: roots grid", what);
  CHECK((uint64_t)p.vanish_per_poly * KZGR_BLOCK >= 2 * p.cells && (uint64_t)(p.vanish_per_poly - 1) * KZGR_BLOCK < 2 * p.cells && p.vanish_grid == count * p.vanish_per_poly, "%s: vanish grid", what);
  CHECK((uint64_t)p.scale_grid * KZGR_BLOCK >= p.scalars, "%s: scale grid", what);
  CHECK((uint64_t)p.finish_per_poly * KZGR_BLOCK >= n && (uint64_t)(p.finish_per_poly - 1) * KZGR_BLOCK < n && p.finish_grid == count * p.finish_per_poly, "%s: finish grid", what);
  CHECK(KZGR_ROOT_TILE <= KZGR_BLOCK && p.cells <= ((uint64_t)1 << KZGR_MAX_LOG_CELLS), "%s: the LDS arrays", what);
  // the scatter, walked as the kernel walks it: every (residue, entry) read once, every scalar of EZ written once
  const uint64_t T = p.tile;
  CHECK(p.scatter_block == T * T && p.scatter_grid == count * p.tiles_r * p.tiles_c && p.tiles_r * T >= l && p.tiles_c * T >= 2 * c && T <= 16, "%s: scatter plan", what);
  std::vector<int> rd(count * 2 * n, 0), wr(p.scalars, 0);
  for (uint64_t b0 = 0; b0 < p.scatter_grid; b0++) {
    uint64_t b = b0;
    const uint64_t tc = b % p.tiles_c; b /= p.tiles_c;
    const uint64_t tr = b % p.tiles_r; b /= p.tiles_r;
    const uint64_t v = b;
    CHECK(v < count, "%s: a workgroup beyond the last polynomial", what);
    for (uint64_t y = 0; y < T; y++) for (uint64_t x = 0; x < T; x++) {
      const uint64_t rho = tc * T + y, e = tr * T + x;
      if (rho < 2 * c && e < l) {
        const uint64_t i = kzgr_cell_of_residue(rho, p.log_c, order);
        CHECK(i < 2 * c, "%s: the slot index leaves the table", what);
        rd[v * 2 * n + i * l + e]++;
      }
      const uint64_t we = tr * T + y, wrho = tc * T + x;
      if (wrho < 2 * c && we < l) {
        const uint64_t row = order == KZGR_ORDER_BITREV ? kzgr_bitrev(we, log_l) : we;
        const uint64_t at = (v << (log_n + 1)) + (row << (p.log_c + 1)) + wrho;
        CHECK(at < p.scalars, "%s: the scatter writes outside the working vector", what);
        if (at < p.scalars) wr[at]++;
        CHECK((at & (2 * n - 1)) == kzg_cell_src(kzgr_cell_of_residue(wrho, p.log_c, order), we, p.log_c, log_l, order), "%s: the scatter's target is not kzg_cell_src", what);
      }
    }
  }
  for (size_t i = 0; i < rd.size(); i++) CHECK(rd[i] == 1 && wr[i] == 1, "%s: element %zu read %d / written %d times", what, i, rd[i], wr[i]);
}

static void offsets_model() {
  uint32_t eff[6]; uint8_t mis[6];
  const uint32_t good[5] = {0, 4, 9, 9, 17};
  kzgr_effective(good, 4, 17, eff, mis);
  for (int i = 0; i < 5; i++) CHECK(eff[i] == good[i] && !mis[i], "valid offsets are their own effective offsets");
  const uint32_t dec[5] = {0, 4, 3, 9, 17};
  kzgr_effective(dec, 4, 17, eff, mis);
  CHECK(eff[2] == 4 && mis[2] && !mis[0] && !mis[1] && !mis[3] && !mis[4], "a decreasing offset flags itself alone");
  const uint32_t far[5] = {0, 4, 22, 9, 17};
  kzgr_effective(far, 4, 17, eff, mis);
  CHECK(eff[2] == 17 && eff[3] == 17 && mis[2] && mis[3] && !mis[4] && !mis[1], "an offset beyond m flags itself and the smaller ones behind it");
  const uint32_t ends[3] = {1, 4, 9};
  kzgr_effective(ends, 2, 10, eff, mis);
  CHECK(eff[0] == 0 && eff[2] == 10 && mis[0] && mis[2] && !mis[1], "offsets[0] != 0 and offsets[count] != m");
  // the host form on (4, 2): c = 4, 2c = 8
  const uint32_t off[3] = {0, 4, 9};
  const uint32_t col[9] = {0, 1, 2, 3, 7, 6, 5, 4, 3};
  CHECK(!kzgr_check_host(off, 2, col, 4, 2), "host: the good call is refused");
  CHECK(!kzgr_check_host(nullptr, 0, nullptr, 4, 2), "host: count = 0");
  { const uint32_t o2[3] = {1, 4, 9}; CHECK(kzgr_check_host(o2, 2, col, 4, 2), "host: offsets[0] != 0"); }
  { const uint32_t o2[3] = {0, 5, 4}; CHECK(kzgr_check_host(o2, 2, col, 4, 2), "host: decreasing offsets"); }
  { const uint32_t o2[3] = {0, 3, 9}; CHECK(kzgr_check_host(o2, 2, col, 4, 2), "host: fewer than c cells"); }
  { uint32_t c2[9]; for (int i = 0; i < 9; i++) c2[i] = col[i]; c2[2] = 8; CHECK(kzgr_check_host(off, 2, c2, 4, 2), "host: col = 2c"); }
  { uint32_t c2[9]; for (int i = 0; i < 9; i++) c2[i] = col[i]; c2[2] = 0xFFFFFFFFu; CHECK(kzgr_check_host(off, 2, c2, 4, 2), "host: col = 2^32 - 1"); }
  { uint32_t c2[9]; for (int i = 0; i < 9; i++) c2[i] = col[i]; c2[8] = 7; CHECK(kzgr_check_host(off, 2, c2, 4, 2), "host: a duplicate"); }
  { uint32_t big[4096]; for (uint32_t i = 0; i < 4096; i++) big[i] = 4095 - i; const uint32_t o2[2] = {0, 4096}; CHECK(!kzgr_check_host(o2, 1, big, 12, 1), "host: all 4096 cells of the largest 2c"); }
}

static int g_refusals = 0;
static void refused(const KzgrArgs& a, const char* what) { g_refusals++; CHECK(kzgr_check(a), "%s is not refused", what); }

static void refusals() {
  alignas(16) static char buf[1 << 16];
  KzgrArgs g;
  g.col = buf; g.offsets = buf + 256; g.cells = buf + 512; g.count = 3; g.m = 15; g.log_n = 4; g.log_l = 2;       // cells: 15 * 4 * 32 = 1920 bytes
  g.polys = buf + 4096; g.out_cells = buf + 8192; g.ok = buf + 16384; g.device = true;                            // polys 1536, out_cells 3072 bytes
  CHECK(!kzgr_check(g), "the good call is refused: %s", kzgr_check(g));
  { KzgrArgs a = g; a.polys = nullptr; CHECK(!kzgr_check(a), "out_cells alone is fine"); }
  { KzgrArgs a = g; a.out_cells = nullptr; CHECK(!kzgr_check(a), "polys alone is fine"); }
  { KzgrArgs a = g; a.count = 0; a.m = 0; a.col = a.offsets = a.cells = a.polys = a.out_cells = a.ok = nullptr; CHECK(!kzgr_check(a), "count = 0 is a no-op"); }
  { KzgrArgs a = g; a.cells = buf + 520; a.device = false; CHECK(!kzgr_check(a), "the host form takes any alignment"); }
  { KzgrArgs a = g; a.col = nullptr; refused(a, "NULL col"); }
  { KzgrArgs a = g; a.offsets = nullptr; refused(a, "NULL offsets"); }
  { KzgrArgs a = g; a.cells = nullptr; refused(a, "NULL cells"); }
  { KzgrArgs a = g; a.ok = nullptr; refused(a, "NULL ok"); }
  { KzgrArgs a = g; a.polys = nullptr; a.out_cells = nullptr; refused(a, "both outputs NULL"); }
  { KzgrArgs a = g; a.count = 0; refused(a, "cells but no polynomial"); }
  { KzgrArgs a = g; a.order = 2; refused(a, "order 2"); }
  { KzgrArgs a = g; a.order = -1; refused(a, "order -1"); }
  { KzgrArgs a = g; a.log_n = -1; refused(a, "log_n < 0"); }
  { KzgrArgs a = g; a.log_n = 28; refused(a, "log_n = 28"); }
  { KzgrArgs a = g; a.log_l = -1; refused(a, "log_l < 0"); }
  { KzgrArgs a = g; a.log_l = 5; refused(a, "log_l > log_n"); }
  { KzgrArgs a = g; a.log_n = 14; a.log_l = 13; refused(a, "log_l = 13"); }
  { KzgrArgs a = g; a.log_n = 13; a.log_l = 1; refused(a, "2c = 8192"); }
  { KzgrArgs a = g; a.log_n = 27; a.log_l = 12; refused(a, "(27, 12): 2c = 2^16"); }
  { KzgrArgs a = g; a.count = ((uint64_t)1 << 23) + 1; refused(a, "count * 2n > 2^28"); }
  { KzgrArgs a = g; a.count = (uint64_t)1 << 63; refused(a, "count = 2^63"); }
  { KzgrArgs a = g; a.count = ~(uint64_t)0; refused(a, "count = 2^64 - 1"); }
  { KzgrArgs a = g; a.count = ((uint64_t)1 << 59) + 1; refused(a, "count * 2n wraps"); }
  { KzgrArgs a = g; a.m = ((uint64_t)1 << 24) + 1; refused(a, "m > 2^24"); }
  { KzgrArgs a = g; a.m = (uint64_t)1 << 63; refused(a, "m = 2^63"); }
  { KzgrArgs a = g; a.m = ~(uint64_t)0; refused(a, "m = 2^64 - 1"); }
  { KzgrArgs a = g; a.log_n = 13; a.log_l = 12; a.m = ((uint64_t)1 << 16) + 1; refused(a, "m * l > 2^28"); }
  { KzgrArgs a = g; a.cells = buf + 520; refused(a, "misaligned cells"); }
  { KzgrArgs a = g; a.polys = buf + 4104; refused(a, "misaligned polys"); }
  { KzgrArgs a = g; a.out_cells = buf + 8200; refused(a, "misaligned out_cells"); }
  { KzgrArgs a = g; a.col = buf + 2; refused(a, "misaligned col"); }
  { KzgrArgs a = g; a.offsets = buf + 257; refused(a, "misaligned offsets"); }
  { KzgrArgs a = g; a.polys = buf + 512 + 1920 - 16; refused(a, "polys start inside cells"); }
  { KzgrArgs a = g; a.polys = buf + 512 + 1920; CHECK(!kzgr_check(a), "polys right behind cells"); }
  { KzgrArgs a = g; a.out_cells = buf + 512; refused(a, "out_cells over cells"); }
  { KzgrArgs a = g; a.ok = buf + 59; refused(a, "ok inside col"); }
  { KzgrArgs a = g; a.ok = buf + 60; CHECK(!kzgr_check(a), "ok right behind col"); }
  { KzgrArgs a = g; a.ok = buf + 256 + 15; refused(a, "ok inside offsets"); }
  { KzgrArgs a = g; a.out_cells = buf + 4096 + 1536 - 16; refused(a, "out_cells starts inside polys"); }
  { KzgrArgs a = g; a.ok = buf + 4096 + 7; refused(a, "ok inside polys"); }
  { KzgrArgs a = g; a.ok = buf + 8192 + 3071; refused(a, "ok on the last byte of out_cells"); }
  { KzgrArgs a = g; a.ok = buf + 8192 + 3072; CHECK(!kzgr_check(a), "ok right behind out_cells"); }
  { KzgrArgs a = g; a.log_n = 27; a.log_l = 16; refused(a, "log_l = 16"); }
  CHECK(!kzgr_plan(28, 0, 1, 0, false).ok && !kzgr_plan(13, 1, 1, 0, false).ok && !kzgr_plan(4, 2, ((uint64_t)1 << 23) + 1, 0, false).ok && !kzgr_plan(4, 2, 1, ((uint64_t)1 << 24) + 1, false).ok &&
        !kzgr_plan(4, 2, 0, 5, false).ok && !kzgr_plan(4, 2, 1, 5, false, 17).ok && !kzgr_plan(4, 5, 1, 0, false).ok && !kzgr_plan(4, 2, ~(uint64_t)0, 0, false).ok, "plan refusals");
  CHECK(!kzgr_plan(27, 12, 1, 0, false).ok, "the plan refuses (27, 12)");
  CHECK(kzgr_plan(23, 12, 16, (uint64_t)1 << 16, true).ok && kzgr_plan(11, 0, 1, 4096, false).ok, "the largest shapes pass");
}

int main() {
  for (int log_n = 0; log_n <= 8; log_n++)
    for (int log_l = 0; log_l <= log_n; log_l++)
      for (int order = 0; order < 2; order++) {
        maps_model(log_n, log_l, order);
        for (uint64_t count : {0, 1, 3})
          for (unsigned tile : {4u, 0u}) { plan_model(log_n, log_l, count, order, false, tile); plan_model(log_n, log_l, count, order, true, tile); }
      }
  printf("plans\n");
  offsets_model();
  printf("offsets\n");
  refusals();
  printf("refusals %d\n", g_refusals);
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
