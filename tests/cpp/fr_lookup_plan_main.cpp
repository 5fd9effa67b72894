// tests/cpp/fr_lookup_plan_main.cpp -- csrc/fr_lookup_plan.h on its own, built with the address and undefined-behaviour sanitizers and
// run directly (tests/test_fr_lookup_plan.py).  It sweeps the plan over rows = 1 .. 2^24 at the powers of two and +-1 and c = 1 .. 8
// (slots a power of two >= 2 rows, LDS within 64 KB, the path flipping exactly at FRL_LDS_ROWS, the grids covering n exactly), hands
// the two argument checks one call per refusal, and holds the hash to its property: two keys that differ in one word hash differently.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fr_lookup_plan.h"
using namespace bls;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next64() { g_s += 0x9E3779B97F4A7C15ull; uint64_t z = g_s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

static void plans() {
  std::vector<size_t> rows_list;
  for (int l = 0; l <= 24; l++) for (long d = -1; d <= 1; d++) { const long r = (1l << l) + d; if (r >= 1 && r <= (1l << 24)) rows_list.push_back((size_t)r); }
  const size_t ns[] = {0, 1, FRL_BLOCK - 1, FRL_BLOCK, FRL_BLOCK + 1, (size_t)1 << 28};
  for (size_t rows : rows_list) {
    const size_t slots = frl_slots(rows);
    REQUIRE((slots & (slots - 1)) == 0 && slots >= 2 * rows && (rows == 1 || slots < 4 * rows));
    for (size_t n : ns) {
      const FrLookupPlan p = fr_lookup_plan(rows, n);
      REQUIRE(p.ok && p.slots == slots && p.block == (unsigned)FRL_BLOCK);
      REQUIRE(p.lds_path == (rows <= FRL_LDS_ROWS ? 1 : 0));
      REQUIRE(p.count_lds <= FRL_LDS_LIMIT && p.count_lds == (p.lds_path ? rows * 4 : (size_t)FRL_CACHE * 8));
      REQUIRE((size_t)p.build_grid * p.block >= rows && (size_t)(p.build_grid - 1) * p.block < rows && p.finish_grid == p.build_grid);
      const size_t per = (size_t)p.count_grid * p.block;
      if (n == 0) REQUIRE(p.count_grid == 0 && p.iters == 0);
      else REQUIRE(p.count_grid >= 1 && p.count_grid <= FRL_COUNT_GRID_MAX && per * p.iters >= n && per * (p.iters - 1) < n);
      // no batch of the last iteration starts beyond n + per: every lane's row number fits 64 bits and the last batch holds a row
      if (n) REQUIRE(((size_t)(p.iters - 1) * p.count_grid) * p.block < n);
    }
    // the test-only threshold and the small block
    for (size_t lds_rows : {(size_t)64, (size_t)1000}) {
      const FrLookupPlan p = fr_lookup_plan(rows, 777, 64, lds_rows);
      REQUIRE(p.ok && p.lds_path == (rows <= lds_rows ? 1 : 0) && p.block == 64 && p.count_grid == 13 && p.iters == 1);
    }
  }
  REQUIRE(fr_lookup_plan(FRL_LDS_ROWS, 5).lds_path == 1 && fr_lookup_plan(FRL_LDS_ROWS + 1, 5).lds_path == 0);
  REQUIRE(!fr_lookup_plan(0, 1).ok && !fr_lookup_plan(FRL_MAX_ROWS + 1, 1).ok && !fr_lookup_plan(5, FRL_MAX_TOTAL + 1).ok);
  REQUIRE(!fr_lookup_plan(5, 5, 32).ok && !fr_lookup_plan(5, 5, 96).ok && !fr_lookup_plan(5, 5, 2048).ok && !fr_lookup_plan(5, 5, 256, FRL_LDS_ROWS + 1).ok);
  std::printf("plans\n");
}

static bool has(const char* text, const char* part) { return text && std::strstr(text, part); }

static void refusals() {
  alignas(16) static char mem[4096];
  const size_t big = (size_t)1 << 63;
  // building
  for (int device = 0; device <= 1; device++) {
    REQUIRE(frl_table_check(2, mem, 100, 100, device) == nullptr);
    REQUIRE(has(frl_table_check(0, mem, 100, 100, device), "c must be") && has(frl_table_check(9, mem, 100, 100, device), "c must be") && has(frl_table_check(-1, mem, 100, 100, device), "c must be"));
    REQUIRE(has(frl_table_check(2, mem, 100, 0, device), "rows") && has(frl_table_check(2, mem, big, FRL_MAX_ROWS + 1, device), "rows"));
    REQUIRE(has(frl_table_check(2, nullptr, 100, 100, device), "NULL"));
    REQUIRE(has(frl_table_check(2, mem, 99, 100, device), "pitch"));
    REQUIRE(has(frl_table_check(2, mem, big, 100, device), "2^28") && has(frl_table_check(2, mem, ~(size_t)0, 100, device), "2^28") && has(frl_table_check(8, mem, FRL_MAX_TOTAL / 7, 100, device), "2^28"));
    REQUIRE(frl_table_check(1, mem, FRL_MAX_TOTAL, FRL_MAX_ROWS, device) == nullptr);
  }
  REQUIRE(has(frl_table_check(2, mem + 8, 100, 100, true), "aligned") && frl_table_check(2, mem + 8, 100, 100, false) == nullptr);
  // counting: f 2 x 30 scalars at pitch 30 (1920 bytes), mult 10 scalars, index 30 words, missing
  FrlCountArgs ok;
  ok.c = 2; ok.rows = 10; ok.f = mem; ok.pitch = 30; ok.n = 30; ok.mult = mem + 2048; ok.index = mem + 2048 + 320; ok.missing = mem + 2048 + 320 + 120;
  for (int device = 0; device <= 1; device++) {
    ok.device = device != 0;
    REQUIRE(frl_count_check(ok) == nullptr);
    FrlCountArgs a = ok;
    a.c = 0; REQUIRE(has(frl_count_check(a), "handle")); a = ok;
    a.rows = 0; REQUIRE(has(frl_count_check(a), "handle")); a = ok;
    a.negate = 2; REQUIRE(has(frl_count_check(a), "negate")); a.negate = -1; REQUIRE(has(frl_count_check(a), "negate")); a = ok;
    a.n = FRL_MAX_TOTAL + 1; a.pitch = a.n; REQUIRE(has(frl_count_check(a), "2^28")); a = ok;
    a.f = nullptr; REQUIRE(has(frl_count_check(a), "NULL")); a = ok;
    a.pitch = 29; REQUIRE(has(frl_count_check(a), "pitch")); a = ok;
    a.pitch = big; REQUIRE(has(frl_count_check(a), "2^28")); a.pitch = ~(size_t)0; REQUIRE(has(frl_count_check(a), "2^28")); a.pitch = FRL_MAX_TOTAL - 29; REQUIRE(has(frl_count_check(a), "2^28")); a = ok;
    a.mult = mem; REQUIRE(has(frl_count_check(a), "overlaps f")); a.mult = mem + 1920 - 32; REQUIRE(has(frl_count_check(a), "overlaps f")); a.mult = mem + 1920; REQUIRE(frl_count_check(a) == nullptr); a = ok;
    a.index = mem + 1916; REQUIRE(has(frl_count_check(a), "overlaps f")); a = ok;
    a.missing = mem + 1912; REQUIRE(has(frl_count_check(a), "overlaps f")); a = ok;
    a.index = mem + 2048 + 316; REQUIRE(has(frl_count_check(a), "each other")); a = ok;
    a.missing = mem + 2048; REQUIRE(has(frl_count_check(a), "each other")); a.missing = mem + 2048 + 320 + 112; REQUIRE(has(frl_count_check(a), "each other")); a = ok;
    // n == 0: f may be NULL, nothing of f can overlap
    a.n = 0; a.pitch = 0; a.f = nullptr; REQUIRE(frl_count_check(a) == nullptr); a.f = mem; a.mult = mem; REQUIRE(frl_count_check(a) == nullptr); a = ok;
    // every output NULL
    a.mult = a.index = a.missing = nullptr; REQUIRE(frl_count_check(a) == nullptr);
  }
  ok.device = true;
  { FrlCountArgs a = ok; a.f = mem + 8; REQUIRE(has(frl_count_check(a), "16-byte")); a = ok; a.mult = mem + 2048 + 8; REQUIRE(has(frl_count_check(a), "16-byte")); a = ok;
    a.index = mem + 2048 + 322; REQUIRE(has(frl_count_check(a), "4-byte")); a = ok; a.missing = mem + 2048 + 320 + 124; REQUIRE(has(frl_count_check(a), "8-byte")); }
  ok.device = false;
  { FrlCountArgs a = ok; a.f = mem + 1; a.mult = mem + 2049; a.index = mem + 2048 + 321; a.missing = mem + 2048 + 320 + 121; REQUIRE(frl_count_check(a) == nullptr); }
  std::printf("refusals\n");
}

// two keys that differ in any single word: at most 1 collision in 10^5 pairs of 32-bit outputs (the rounds are bijections, so the
// shipped hash has none), every key width; and tiny-limbed keys (multiples of R^-1) spread over the low bits a slot index keeps
static void hash() {
  for (uint64_t seed : {1ull, 2ull, 0xB1512381ull}) {
    g_s = seed;
    int collisions = 0;
    for (int pair = 0; pair < 100000; pair++) {
      const int c = 1 + (int)(next64() % FRL_MAX_COLS);
      uint32_t a[8 * FRL_MAX_COLS], b[8 * FRL_MAX_COLS];
      for (int i = 0; i < 8 * c; i++) a[i] = b[i] = (uint32_t)next64();
      const int w = (int)(next64() % (uint64_t)(8 * c));
      uint32_t d = (uint32_t)next64();
      b[w] ^= d ? d : 1u;
      if (frl_hash(a, c) == frl_hash(b, c)) collisions++;
    }
    REQUIRE(collisions <= 1);
  }
  // keys 0 .. 4095 in the low word only: the low 13 bits (a table of 4096 rows has 8192 slots) take at least half as many values as keys
  std::vector<char> seen(8192, 0);
  int distinct = 0;
  for (uint32_t v = 0; v < 4096; v++) {
    uint32_t k[8] = {v, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t h = frl_hash(k, 1) & 8191u;
    if (!seen[h]) { seen[h] = 1; distinct++; }
  }
  REQUIRE(distinct >= 2048);
  // the width is part of the hash: a key of zeros hashes differently at every c
  uint32_t zeros[8 * FRL_MAX_COLS] = {};
  for (int c = 1; c < FRL_MAX_COLS; c++) REQUIRE(frl_hash(zeros, c) != frl_hash(zeros, c + 1));
  for (uint32_t row : {0u, 1u, 4096u, (1u << 24) - 1}) REQUIRE(frl_cache_entry(row) < FRL_CACHE);
  std::printf("hash\n");
}

int main() {
  plans();
  refusals();
  hash();
  std::printf("all ok\n");
  return 0;
}
