// tests/cpp/fr_edwards_plan_main.cpp -- bls12_381_amd/csrc/fr_edwards_plan.h on its own (tests/test_fr_edwards_plan.py builds this with
// host clang++ -fsanitize=address,undefined and runs it; it includes nothing of the library but that header and what the header includes).
//
//   recoding   for every (bits, window) in [1, 256] x [2, 8] and the edge scalars -- 0, 1, 2^bits - 1, 2^(bits-1), every window at exactly
//              2^(window-1) (0x88...8 for window 4), the top window full (a carry out of it), 2^256 - 1 at bits 256, random ones -- the
//              digits sum back to the scalar, each lies in [-2^(window-1), 2^(window-1)], there are as many as the layout reserves, and
//              fred_scalar_fits agrees with the integer
//   tables     sizes, the entry index of every (base, window, multiple) inside the table, the byte limit
//   plans      launch shapes cover their items, LDS and scratch bytes hold what the kernels index (records, meta words, offsets)
//   complete   Jubjub 1, Bandersnatch 0, a square with d square 0, a non-square with d square 0
//   refusals   one call per refusal of every argument check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fr_edwards_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

struct K { uint32_t w[8]; };
static K k_zero() { K k; memset(k.w, 0, sizeof k.w); return k; }
static void k_set(K* k, int bit) { if (bit >= 0 && bit < 256) k->w[bit >> 5] |= 1u << (bit & 31); }
static K k_mask(K k, int bits) { for (int b = bits; b < 256; b++) k.w[b >> 5] &= ~(1u << (b & 31)); return k; }
static K k_ones(int bits) { K k = k_zero(); for (int b = 0; b < bits; b++) k_set(&k, b); return k; }

// sum_w digit_w 2^(w window) in a signed accumulator of 32-bit words (12 words: 9 windows above 256 bits never happen, the top word keeps the sign)
static bool digits_restate(const K& k, int bits, int window, int* bad_digit) {
  const int W = fred_windows(bits, window), H = fred_table_half(window);
  int64_t acc[12] = {0};
  *bad_digit = 0;
  for (int w = 0; w < W; w++) {
    const int d = fred_digit(k.w, bits, window, w);
    if (d < -H || d > H) *bad_digit = 1;
    const int pos = w * window;
    const int64_t v = (int64_t)d * ((int64_t)1 << (pos & 31));     // |d| <= 128, shift <= 31: below 2^39
    acc[pos >> 5] += v;
  }
  int64_t carry = 0;
  uint32_t got[12];
  for (int i = 0; i < 12; i++) { const int64_t v = acc[i] + carry; got[i] = (uint32_t)v; carry = v >> 32; }
  const K want = k_mask(k, bits);
  for (int i = 0; i < 8; i++) if (got[i] != want.w[i]) return false;
  for (int i = 8; i < 12; i++) if (got[i] != 0) return false;
  return carry == 0;
}

static void recoding() {
  size_t cases = 0;
  for (int bits = 1; bits <= 256; bits++)
    for (int window = FRED_WINDOW_MIN; window <= FRED_WINDOW_MAX; window++) {
      const int W = fred_windows(bits, window);
      CHECK(W == (bits + 1 + window - 1) / window && W * window > bits, "W for bits %d window %d", bits, window);
      const FredTablePlan tp = fred_table_plan(1, bits, window);
      CHECK(tp.ok && tp.W == W && tp.H == 1 << (window - 1), "the layout reserves another W: bits %d window %d", bits, window);
      std::vector<K> ks;
      ks.push_back(k_zero());
      { K k = k_zero(); k_set(&k, 0); ks.push_back(k); }
      ks.push_back(k_ones(bits));
      { K k = k_zero(); k_set(&k, bits - 1); ks.push_back(k); }
      { K k = k_zero(); for (int w = 0; w * window < 256; w++) k_set(&k, w * window + window - 1); ks.push_back(k_mask(k, bits)); }      // every window at 2^(window-1)
      { K k = k_zero(); for (int b = (W - 1) * window - 1; b < bits; b++) k_set(&k, b); ks.push_back(k); }                               // the top window full, and the bit below it
      { K k = k_zero(); for (int b = bits - window; b < bits; b++) k_set(&k, b); ks.push_back(k); }                                      // the last `window` bits set
      ks.push_back(k_ones(256));                                     // bits above `bits` must not be read (at bits 256: 2^256 - 1 itself)
      for (int i = 0; i < 6; i++) { K k; for (int j = 0; j < 8; j++) k.w[j] = (uint32_t)rnd(); ks.push_back(k); }
      for (const K& k : ks) {
        int bad = 0;
        CHECK(digits_restate(k, bits, window, &bad), "digits do not sum to the scalar: bits %d window %d", bits, window);
        CHECK(!bad, "a digit outside the table's range: bits %d window %d", bits, window);
        bool over = false;
        for (int b = bits; b < 256; b++) over |= ((k.w[b >> 5] >> (b & 31)) & 1u) != 0;
        CHECK(fred_scalar_fits(k.w, bits) == !over, "scalar_fits: bits %d", bits);
        cases++;
      }
    }
  printf("recoding %zu\n", cases);
}

static void tables() {
  for (int bits : {1, 3, 64, 253, 256})
    for (int window = FRED_WINDOW_MIN; window <= FRED_WINDOW_MAX; window++)
      for (size_t n : {(size_t)1, (size_t)8, (size_t)64, (size_t)1000}) {
        const FredTablePlan p = fred_table_plan(n, bits, window);
        CHECK(p.ok, "table plan refused n %zu bits %d window %d", n, bits, window);
        CHECK(p.entries == n * p.W * p.H && p.bytes == p.entries * FRED_ENTRY_WORDS * 4 && p.bytes <= FRED_TABLE_MAX_BYTES, "table sizes");
        CHECK((size_t)p.build.grid * p.build.block >= n * p.W && (size_t)p.norm.grid * p.norm.block >= p.entries, "table grids");
        CHECK(p.norm.lds >= (p.norm.block / 64) * 32 && p.norm.block % 64 == 0, "normalise: a scalar per wavefront");
        std::vector<char> seen(p.entries, 0);
        for (size_t b = 0; b < n; b++)
          for (int w = 0; w < p.W; w++)
            for (int k = 1; k <= p.H; k++) {
              const size_t e = fred_entry(b, w, k, p.W, p.H);
              CHECK(e < p.entries && !seen[e], "entry index");
              if (e < p.entries) seen[e] = 1;
            }
      }
  // the largest table the limit allows, and the first one it refuses
  const size_t per = (size_t)fred_windows(253, 8) * 128 * 96;
  CHECK(fred_table_plan(FRED_TABLE_MAX_BYTES / per, 253, 8).ok && !fred_table_plan(FRED_TABLE_MAX_BYTES / per + 1, 253, 8).ok, "the byte limit");
  printf("tables\n");
}

static void plans() {
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)257, FRED_MAX_POINTS}) {
    const FredLaunch l = fred_points_launch(n);
    CHECK((size_t)l.grid * l.block >= n && (size_t)(l.grid - 1) * l.block < n && l.block % 64 == 0, "points launch");
    for (int bits : {1, 3, 64, 253, 256}) {
      const FredMulPlan p = fred_mul_plan(n, bits);
      CHECK(p.ok && (size_t)p.mul.grid * p.mul.block >= n && p.mul.lds == (size_t)p.mul.block * FRED_MUL_ENTRIES * 32 * 4 && p.mul.lds <= FRED_LDS_LIMIT, "mul plan");
      CHECK(p.W == fred_windows(bits, FRED_MUL_WINDOW) && p.doublings == FRED_MUL_WINDOW * (p.W - 1), "mul windows");
    }
  }
  CHECK(fred_mul_plan(1, 64).doublings * 3 < fred_mul_plan(1, 256).doublings, "bits = 64 must do about a quarter of the doublings of 256");
  const FredMsmShape shapes[] = {FredMsmShape(), FredMsmShape{4, 2}, FredMsmShape{64, 1}};
  for (const FredMsmShape& s : shapes)
    for (size_t k : {(size_t)1, (size_t)2, (size_t)300, (size_t)5000})
      for (size_t total : {(size_t)0, (size_t)1, (size_t)s.block * s.terms - 1, (size_t)s.block * s.terms, (size_t)s.block * s.terms + 1, (size_t)3 * s.block * s.terms + 5, (size_t)100000}) {
        const FredMsmPlan p = fred_msm_plan(k, total, s);
        CHECK(p.ok, "msm plan refused");
        CHECK(p.cut.chunk == (uint32_t)(s.block * s.terms) && p.cut.nchunks * p.cut.chunk >= total, "msm chunks");
        CHECK((size_t)p.prep.grid * p.prep.block >= k + 1 && p.off_bytes == (k + 1) * 8, "msm prep");
        CHECK(p.chunks.grid == p.cut.nchunks && p.combine.grid >= 2 * p.cut.nchunks && (size_t)p.combine.grid * p.combine.block >= k, "msm grids");
        CHECK(p.chunks.lds >= (size_t)s.block * (FRED_LDS_REC_WORDS + 2) * 4 && p.chunks.lds <= FRED_LDS_LIMIT && FRED_LDS_REC_WORDS >= FRED_REC_WORDS, "msm LDS");
        // every record and meta word a chunk can name lies inside the scratch
        for (size_t c = 0; c < p.cut.nchunks; c++) {
          const uint32_t cb = (uint32_t)(c * p.cut.chunk);
          CHECK((gsum_record(c, cb, cb) + 1) * FRED_REC_WORDS * 4 <= p.part_bytes && (gsum_record(c, cb + 1, cb) + 1) * FRED_REC_WORDS * 4 <= p.part_bytes, "msm records");
          CHECK((2 * c + 2) * 4 <= p.meta_bytes, "msm meta");
        }
      }
  CHECK(!fred_msm_plan(FRED_MAX_SEGS + 1, 0).ok && !fred_msm_plan(1, FRED_MAX_TOTAL + 1).ok && fred_msm_plan(FRED_MAX_SEGS, FRED_MAX_TOTAL).ok, "msm limits");
  printf("plans\n");
}

static FrpFe fe_u64(uint64_t v) {
  FrpFe r = frp_zero();
  for (int i = 63; i >= 0; i--) { r = frp_dbl(r); if ((v >> i) & 1) r = frp_add(r, frp_one()); }
  return r;
}
static FrpFe fe_u128(uint64_t hi, uint64_t lo) { return frp_add(frp_scale(fe_u64(hi), 64), fe_u64(lo)); }

static void complete() {
  const FrpFe jub_a = frp_neg(frp_one()), jub_d = frp_neg(frp_mul(fe_u64(10240), frp_inv(fe_u64(10241))));
  const uint64_t jub_d_int[4] = {0x01065fd6d6343eb1ull, 0x292d7f6d37579d26ull, 0xf5fd9207e6bd7fd4ull, 0x2a9318e74bfa2b48ull};
  {                                                                // the quotient is the integer the issue prints
    FrpFe raw{{jub_d_int[0], jub_d_int[1], jub_d_int[2], jub_d_int[3]}};
    CHECK(frp_eq(frp_scale(raw, 256), jub_d), "Jubjub's d");
  }
  const FrpFe ban_a = frp_neg(fe_u64(5));
  const FrpFe ban_d = frp_mul(fe_u128(0x687125d125a827fdull, 0xa03bbf93b28099bbull), frp_inv(fe_u128(0x80fc02f153d6afefull, 0x99b1d66761b34aa1ull)));
  CHECK(fred_is_square(jub_a) && !fred_is_square(jub_d) && fred_complete(jub_a, jub_d) == 1, "Jubjub is complete");
  CHECK(!fred_is_square(ban_a) && !fred_is_square(ban_d) && fred_complete(ban_a, ban_d) == 0, "Bandersnatch is not complete");
  CHECK(fred_complete(fe_u64(4), fe_u64(9)) == 0, "a square, d square");
  CHECK(fred_complete(ban_a, fe_u64(9)) == 0, "a non-square, d square");
  CHECK(fred_complete(fe_u64(4), jub_d) == 1, "a square, d non-square");
  FredCurve cv;
  CHECK(fred_curve_check(jub_a.v, jub_d.v, &cv) == nullptr && cv.complete == 1, "curve_check takes Jubjub");
  CHECK(fred_curve_check(ban_a.v, ban_d.v, &cv) == nullptr && cv.complete == 0, "curve_check takes Bandersnatch");
  // (0, 1) and (0, -1) are on every curve; (1, 1) is on none with a != d
  uint64_t p[8];
  const FrpFe one = frp_one(), zero = frp_zero(), m1 = frp_neg(one);
  memcpy(p, zero.v, 32); memcpy(p + 4, one.v, 32);
  CHECK(fred_on_curve(cv, p), "(0, 1)");
  memcpy(p + 4, m1.v, 32);
  CHECK(fred_on_curve(cv, p), "(0, -1)");
  memcpy(p, one.v, 32); memcpy(p + 4, one.v, 32);
  CHECK(!fred_on_curve(cv, p), "(1, 1)");
  memcpy(p, FRP_R64, 32);
  CHECK(!fred_on_curve(cv, p), "limbs >= r");
  printf("complete\n");
}

static void refusals() {
  const FrpFe one = frp_one(), two = frp_dbl(one), zero = frp_zero();
  FredCurve cv;
  int n = 0;
#define REFUSED(expr) do { CHECK((expr) != nullptr, "not refused: %s", #expr); n++; } while (0)
#define TAKEN(expr) do { CHECK((expr) == nullptr, "refused: %s", #expr); } while (0)
  TAKEN(fred_curve_check(one.v, two.v, &cv));
  REFUSED(fred_curve_check(nullptr, two.v, &cv));
  REFUSED(fred_curve_check(one.v, nullptr, &cv));
  REFUSED(fred_curve_check(FRP_R64, two.v, &cv));
  REFUSED(fred_curve_check(one.v, FRP_R64, &cv));
  REFUSED(fred_curve_check(zero.v, two.v, &cv));
  REFUSED(fred_curve_check(one.v, zero.v, &cv));
  REFUSED(fred_curve_check(two.v, two.v, &cv));
  alignas(16) static char buf[4096];
  TAKEN(fred_check_args(buf, 4, buf + 1024, true));
  TAKEN(fred_check_args(nullptr, 0, nullptr, true));
  REFUSED(fred_check_args(buf, FRED_MAX_POINTS + 1, buf + 1024, false));
  REFUSED(fred_check_args(nullptr, 4, buf, false));
  REFUSED(fred_check_args(buf, 4, nullptr, false));
  REFUSED(fred_check_args(buf + 8, 4, buf + 1024, true));
  REFUSED(fred_check_args(buf, 4, buf + 255, false));
  TAKEN(fred_normalize_args(buf, 4, buf + 1024, nullptr, true));
  REFUSED(fred_normalize_args(buf, FRED_MAX_POINTS + 1, buf + 1024, nullptr, false));
  REFUSED(fred_normalize_args(nullptr, 4, buf + 1024, nullptr, false));
  REFUSED(fred_normalize_args(buf, 4, nullptr, nullptr, false));
  REFUSED(fred_normalize_args(buf + 4, 4, buf + 1024, nullptr, true));
  REFUSED(fred_normalize_args(buf, 4, buf + 1028, nullptr, true));
  REFUSED(fred_normalize_args(buf, 4, buf, nullptr, false));                     // out == in: there is no in-place form
  REFUSED(fred_normalize_args(buf, 4, buf + 96 * 4 - 1, nullptr, false));
  REFUSED(fred_normalize_args(buf, 4, buf + 1024, buf + 100, false));
  REFUSED(fred_normalize_args(buf, 4, buf + 1024, buf + 1024 + 255, false));
  TAKEN(fred_mul_args(buf, buf + 512, 253, 4, buf + 1024, true));
  REFUSED(fred_mul_args(buf, buf + 512, 0, 4, buf + 1024, true));
  REFUSED(fred_mul_args(buf, buf + 512, 257, 4, buf + 1024, true));
  REFUSED(fred_mul_args(buf, buf + 512, 253, FRED_MAX_POINTS + 1, buf + 1024, false));
  REFUSED(fred_mul_args(nullptr, buf + 512, 253, 4, buf + 1024, false));
  REFUSED(fred_mul_args(buf, nullptr, 253, 4, buf + 1024, false));
  REFUSED(fred_mul_args(buf, buf + 512, 253, 4, nullptr, false));
  REFUSED(fred_mul_args(buf + 8, buf + 512, 253, 4, buf + 1024, true));
  REFUSED(fred_mul_args(buf, buf + 512 + 8, 253, 4, buf + 1024, true));
  REFUSED(fred_mul_args(buf, buf + 512, 253, 4, buf + 1024 + 8, true));
  REFUSED(fred_mul_args(buf, buf + 512, 253, 4, buf + 128, false));
  REFUSED(fred_mul_args(buf, buf + 512, 253, 4, buf + 512 + 64, false));
#define PLAN_REFUSED(expr) do { const FredTablePlan p_ = (expr); CHECK(!p_.ok && p_.why, "not refused: %s", #expr); n++; } while (0)
  CHECK(fred_table_plan(8, 253, 4).ok, "a table plan");
  PLAN_REFUSED(fred_table_plan(8, 0, 4));
  PLAN_REFUSED(fred_table_plan(8, 257, 4));
  PLAN_REFUSED(fred_table_plan(8, 253, 1));
  PLAN_REFUSED(fred_table_plan(8, 253, 9));
  PLAN_REFUSED(fred_table_plan(0, 253, 4));
  PLAN_REFUSED(fred_table_plan(FRED_MAX_BASES + 1, 3, 2));
  PLAN_REFUSED(fred_table_plan((size_t)1 << 20, 253, 8));          // 2^20 * 32 * 128 * 96 bytes
  FredMsmArgs a;
  a.nbases = 64; a.base_first = buf; a.offsets = buf + 256; a.scalars = buf + 512; a.k = 4; a.total = 8; a.out = buf + 2048; a.device = true;
  TAKEN(fred_msm_args(a));
  { FredMsmArgs b = a; b.k = 0; b.total = 0; TAKEN(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.base_first = nullptr; TAKEN(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.k = FRED_MAX_SEGS + 1; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.total = FRED_MAX_TOTAL + 1; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.k = 0; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.offsets = nullptr; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.out = nullptr; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.scalars = nullptr; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.offsets = buf + 258; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.base_first = buf + 2; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.scalars = buf + 520; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.out = buf + 2056; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.out = buf + 512 + 32; b.device = false; REFUSED(fred_msm_args(b)); }
  { FredMsmArgs b = a; b.scalars = buf + 3000; b.out = buf + 200; b.device = false; REFUSED(fred_msm_args(b)); }      // the offsets
  { FredMsmArgs b = a; b.scalars = buf + 3000; b.base_first = buf + 2100; b.device = false; REFUSED(fred_msm_args(b)); }      // base_first
  size_t total = 99;
  { const uint32_t off[4] = {0, 2, 2, 5}; TAKEN(fred_msm_args_host(off, nullptr, 3, 5, &total)); CHECK(total == 5, "total"); }
  { const uint32_t off[4] = {0, 2, 2, 5}, bf[3] = {0, 63, 61}; TAKEN(fred_msm_args_host(off, bf, 3, 64, &total)); }
  { const uint32_t off[4] = {1, 2, 2, 5}; REFUSED(fred_msm_args_host(off, nullptr, 3, 64, &total)); }
  { const uint32_t off[4] = {0, 3, 2, 5}; REFUSED(fred_msm_args_host(off, nullptr, 3, 64, &total)); }
  { const uint32_t off[4] = {0, 2, 2, 5}; REFUSED(fred_msm_args_host(off, nullptr, 3, 4, &total)); }
  { const uint32_t off[4] = {0, 2, 2, 5}, bf[3] = {0, 0, 62}; REFUSED(fred_msm_args_host(off, bf, 3, 64, &total)); }
  { const uint32_t off[2] = {0, 0xFFFFFFFFu}, bf[1] = {0xFFFFFFFFu}; REFUSED(fred_msm_args_host(off, bf, 1, 64, &total)); }      // 64-bit sums: no wrap
  { const uint32_t off[2] = {0, (uint32_t)FRED_MAX_TOTAL + 1}, bf[1] = {0}; REFUSED(fred_msm_args_host(off, bf, 1, (size_t)1 << 30, &total)); }
  printf("refusals %d\n", n);
}

int main() {
  recoding();
  tables();
  plans();
  complete();
  refusals();
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
