// tests/cpp/kzg_verify_plan_main.cpp -- bls12_381_amd/csrc/kzg_verify_plan.h on its own (tests/test_kzg_verify_plan.py builds this with
// host clang++ -fsanitize=address,undefined and runs it; it includes nothing of the library but that header).
//
// The fold of batched KZG cell-proof verification is run as a MODEL over counters: the effective offsets are built as k_kzgv_offsets
// builds them, the lanes of both passes are walked with the plan's grids and cut exactly as kzg_verify.hip.h walks them, and every
// buffer has exactly the size the plan reserves.  Checked for every (log_n <= 8, log_l <= log_n), m in {0, 1, 5, 300}, batch cuts with
// empty, one-cell and one-batch-of-all batches, the automatic chunk and chunks of 1, 3 and 4 cells: every cell reaches the sum of its
// batch exactly once (no other batch, no cell twice), every record a combine lane reads was written, the scratch sections do not
// overlap and end inside the block.  Offsets that break the contract give a valid CSR array and flag exactly the batches they touch.
// The exponent maps are printed ("map ..." lines) for the Python side to compare with tests/kzg_ref.py.  Then one call per refusal of the
// argument checks, 64-bit extremes included.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kzg_verify_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

// k_kzgv_offsets as one lane would run it
static void effective(const std::vector<uint32_t>& off, uint32_t m, std::vector<uint32_t>& eff, std::vector<uint8_t>& mis) {
  const size_t nseg = off.size() - 1;
  eff.assign(nseg + 1, 0); mis.assign(nseg + 1, 0);
  uint32_t run = 0;
  for (size_t i = 0; i <= nseg; i++) {
    const uint32_t v = i == 0 ? 0u : i == nseg ? m : (off[i] < m ? off[i] : m);
    run = v > run ? v : run;
    eff[i] = run; mis[i] = off[i] != run;
  }
}

// both passes of the fold over counters: cnt[s][k] = how often cell k was added into batch s (column 0 stands for every column)
static void fold_model(int log_n, int log_l, const std::vector<uint32_t>& off, uint32_t chunk_arg, const char* what) {
  const uint32_t nseg = (uint32_t)off.size() - 1, m = off[nseg];
  const KzgvPlan p = kzgv_plan(log_n, log_l, m, nseg, chunk_arg);
  CHECK(p.ok, "%s (%d, %d): refused", what, log_n, log_l);
  if (!p.ok || !nseg) return;
  std::vector<uint32_t> eff; std::vector<uint8_t> mis;
  effective(off, m, eff, mis);
  for (uint32_t s = 0; s <= nseg; s++) CHECK(eff[s] == off[s] && !mis[s], "%s: valid offsets changed", what);
  const uint64_t l = (uint64_t)1 << log_l;
  CHECK(p.chunk >= 1 && p.chunk <= KZGV_CHUNK_MAX && p.nchunks * p.chunk >= m && (p.nchunks == 0 || (p.nchunks - 1) * p.chunk < m), "%s: the cut", what);
  CHECK((uint64_t)p.fold_grid * KZGV_BLOCK >= p.nchunks * l && (uint64_t)p.combine_grid * KZGV_BLOCK >= nseg * l && (uint64_t)p.weights_grid * KZGV_BLOCK >= m &&
        (uint64_t)p.copy_grid * KZGV_BLOCK >= m * l && (uint64_t)p.finish_grid * KZGV_BLOCK >= nseg, "%s: grids", what);
  // the scratch sections in order, none overlapping, all inside the block
  const size_t at[] = {p.eff, p.mis, p.badidx, p.bad, p.isone, p.off64, p.msm_off, p.base_first, p.scal, p.pxy, p.pinf, p.prod, p.sum, p.cellc, p.part, p.agg, p.msm, p.ab, p.abxy, p.abinf,
                       p.qidx, p.poff, p.gt, p.bytes};
  const uint64_t need[] = {(nseg + 1ull) * 4, nseg + 1ull, nseg, nseg, nseg, (3ull * nseg + 1) * 8, (nseg + 1ull) * 4, nseg * 4ull, 3ull * m * 32, 3ull * m * 96, 3ull * m, 3ull * m * 144,
                           3ull * nseg * 144, m * l * 32, 2 * p.nchunks * l * 32, nseg * l * 32, nseg * 144ull, 2ull * nseg * 144, 2ull * nseg * 96, 2ull * nseg, 2ull * nseg * 4,
                           (nseg + 1ull) * 8, nseg * 576ull};
  for (int i = 0; i < 23; i++) CHECK(at[i] % 256 == 0 && at[i] + need[i] <= at[i + 1], "%s: scratch section %d", what, i);
  // pass 1
  std::vector<std::vector<uint32_t>> agg(nseg), part(2 * p.nchunks);
  std::vector<int> agg_set(nseg, 0), part_set(2 * p.nchunks, 0);
  for (uint64_t q = 0; q < p.nchunks; q++) {
    const uint32_t cb = (uint32_t)(q * p.chunk), ce = m - cb < p.chunk ? m : cb + p.chunk;
    uint32_t s = kzgv_seg_of(eff.data(), nseg, cb), so = eff[s], se = eff[s + 1];
    CHECK(so <= cb && cb < se, "%s: seg_of(%u) = %u", what, cb, s);
    std::vector<uint32_t> acc;
    auto close = [&]() {
      if (se <= so) return;
      if (kzgv_inside(so, se, cb, p.chunk)) { agg[s] = acc; agg_set[s]++; }
      else { const size_t rec = kzgv_record(q, so, cb); CHECK(rec < part.size(), "%s: record", what); part[rec] = acc; part_set[rec]++; }
    };
    for (uint32_t k = cb; k < ce; k++) {
      while (k >= se) { close(); s++; CHECK(s < nseg, "%s: walked past the last batch", what); so = se; se = eff[s + 1]; acc.clear(); }
      acc.push_back(k);
    }
    close();
  }
  // pass 2
  for (uint32_t s = 0; s < nseg; s++) {
    const uint32_t so = eff[s], se = eff[s + 1];
    if (se <= so) { agg[s].clear(); agg_set[s]++; continue; }
    const size_t q0 = so / p.chunk, q1 = (se - 1) / p.chunk;
    if (q0 == q1) continue;
    std::vector<uint32_t> acc;
    for (size_t q = q0; q <= q1; q++) {
      const size_t rec = kzgv_record(q, so, (uint32_t)(q * p.chunk));
      CHECK(rec < part.size() && part_set[rec] == 1, "%s: batch %u reads record %zu, written %d times", what, s, rec, rec < part.size() ? part_set[rec] : -1);
      if (rec < part.size()) acc.insert(acc.end(), part[rec].begin(), part[rec].end());
    }
    agg[s] = acc; agg_set[s]++;
  }
  for (uint32_t s = 0; s < nseg; s++) {
    CHECK(agg_set[s] == 1, "%s: batch %u written %d times", what, s, agg_set[s]);
    CHECK(agg[s].size() == off[s + 1] - off[s], "%s: batch %u holds %zu cells of %u", what, s, agg[s].size(), off[s + 1] - off[s]);
    for (size_t i = 0; i < agg[s].size() && i < off[s + 1] - off[s]; i++) CHECK(agg[s][i] == off[s] + i, "%s: batch %u cell %zu", what, s, i);
  }
}

static std::vector<std::vector<uint32_t>> cuts(uint32_t m) {
  std::vector<std::vector<uint32_t>> out;
  out.push_back({0, m});                                       // one batch of all
  std::vector<uint32_t> ones;                                  // one cell each
  for (uint32_t k = 0; k <= m; k++) ones.push_back(k);
  out.push_back(ones);
  out.push_back({0, 0, m, m});                                 // empty batches around
  std::vector<uint32_t> mixed = {0};                           // 0, 3, 0, 2, 7, 1, ... cells
  const uint32_t lens[] = {0, 3, 0, 2, 7, 1, 0, 64, 5};
  for (int i = 0; mixed.back() < m; i++) mixed.push_back(mixed.back() + lens[i % 9] > m ? m : mixed.back() + lens[i % 9]);
  mixed.push_back(m);
  out.push_back(mixed);
  return out;
}

static void broken_offsets() {
  struct { std::vector<uint32_t> off; uint32_t m; std::vector<int> bad; } cases[] = {
      {{0, 5, 3, 8}, 8, {0, 1, 1}},            // a decrease: the batch that decreases and the one behind it
      {{0, 7, 2, 4, 8}, 8, {0, 1, 1, 1}},      // ... and every batch that begins below the running maximum
      {{1, 4, 8}, 8, {1, 0}},                  // offsets[0] != 0
      {{0, 4, 9}, 8, {0, 1}},                  // beyond m
      {{0, 4, 6}, 8, {0, 1}},                  // offsets[nseg] != m
      {{0, 0xffffffffu, 3, 8}, 8, {1, 1, 1}},  // a huge value: clamped to m, everything behind it is empty and flagged
  };
  for (auto& c : cases) {
    std::vector<uint32_t> eff; std::vector<uint8_t> mis;
    effective(c.off, c.m, eff, mis);
    const size_t nseg = c.off.size() - 1;
    CHECK(eff[0] == 0 && eff[nseg] == c.m, "broken: the ends");
    for (size_t s = 0; s < nseg; s++) {
      CHECK(eff[s] <= eff[s + 1], "broken: the effective offsets decrease");
      CHECK((mis[s] || mis[s + 1]) == (c.bad[s] != 0), "broken: batch %zu flagged %d, wanted %d", s, mis[s] || mis[s + 1], c.bad[s]);
    }
    for (uint32_t k = 0; k < c.m; k++) { const uint32_t s = kzgv_seg_of(eff.data(), (uint32_t)nseg, k); CHECK(s < nseg && eff[s] <= k && k < eff[s + 1], "broken: seg_of"); }
  }
}

static void refusals() {
  alignas(16) static unsigned char buf[4096];
  KzgvArgs ok;
  ok.handle_given = true; ok.log_n = 4; ok.log_l = 2; ok.commit_xy = buf; ok.commit_inf = buf + 512; ok.ncommit = 2; ok.row = buf + 640; ok.col = buf + 704; ok.cells = buf + 1024;
  ok.proof_xy = buf + 2048; ok.proof_inf = buf + 2560; ok.offsets = buf + 2624; ok.nseg = 2; ok.m = 4; ok.r = buf + 2688; ok.verdict = buf + 2816; ok.out_ab = buf + 3072; ok.device = true;
  CHECK(kzgv_check(ok) == nullptr, "the good call is refused: %s", kzgv_check(ok));
  int n = 0;
  auto refuse = [&](KzgvArgs a, const char* what) { n++; CHECK(kzgv_check(a) != nullptr, "not refused: %s", what); };
  { KzgvArgs a = ok; a.handle_given = false; refuse(a, "NULL handle"); }
  { KzgvArgs a = ok; a.order = 2; refuse(a, "order 2"); }
  { KzgvArgs a = ok; a.order = -1; refuse(a, "order -1"); }
  { KzgvArgs a = ok; a.m = ((uint64_t)1 << 24) + 1; refuse(a, "m > 2^24"); }
  { KzgvArgs a = ok; a.nseg = ((uint64_t)1 << 24) + 1; refuse(a, "nseg > 2^24"); }
  { KzgvArgs a = ok; a.m = ~(uint64_t)0; refuse(a, "m = 2^64 - 1"); }
  { KzgvArgs a = ok; a.nseg = ~(uint64_t)0; refuse(a, "nseg = 2^64 - 1"); }
  { KzgvArgs a = ok; a.m = (uint64_t)1 << 62; refuse(a, "m * l wraps"); }
  { KzgvArgs a = ok; a.ncommit = (uint64_t)1 << 32; refuse(a, "ncommit = 2^32"); }
  { KzgvArgs a = ok; a.log_n = 20; a.log_l = 12; a.m = ((uint64_t)1 << 15) + 1; refuse(a, "m * l > 2^27"); }
  { KzgvArgs a = ok; a.log_n = 20; a.log_l = 12; a.m = 4; a.nseg = ((uint64_t)1 << 15) + 1; refuse(a, "nseg * l > 2^27"); }
  { KzgvArgs a = ok; a.nseg = 0; refuse(a, "cells but no batch"); }
  { KzgvArgs a = ok; a.offsets = nullptr; refuse(a, "NULL offsets"); }
  { KzgvArgs a = ok; a.r = nullptr; refuse(a, "NULL r"); }
  { KzgvArgs a = ok; a.verdict = nullptr; refuse(a, "NULL verdict"); }
  { KzgvArgs a = ok; a.row = nullptr; refuse(a, "NULL row"); }
  { KzgvArgs a = ok; a.col = nullptr; refuse(a, "NULL col"); }
  { KzgvArgs a = ok; a.cells = nullptr; refuse(a, "NULL cells"); }
  { KzgvArgs a = ok; a.proof_xy = nullptr; refuse(a, "NULL proofs"); }
  { KzgvArgs a = ok; a.proof_inf = nullptr; refuse(a, "NULL proof flags"); }
  { KzgvArgs a = ok; a.commit_xy = nullptr; refuse(a, "NULL commitments"); }
  { KzgvArgs a = ok; a.commit_inf = nullptr; refuse(a, "NULL commitment flags"); }
  { KzgvArgs a = ok; a.cells = buf + 1024 + 8; refuse(a, "misaligned cells"); }
  { KzgvArgs a = ok; a.r = buf + 2688 + 8; refuse(a, "misaligned r"); }
  { KzgvArgs a = ok; a.proof_xy = buf + 2048 + 4; refuse(a, "misaligned proofs"); }
  { KzgvArgs a = ok; a.commit_xy = buf + 4; refuse(a, "misaligned commitments"); }
  { KzgvArgs a = ok; a.out_ab = buf + 3072 + 4; refuse(a, "misaligned out_ab"); }
  { KzgvArgs a = ok; a.row = buf + 640 + 2; refuse(a, "misaligned row"); }
  { KzgvArgs a = ok; a.col = buf + 704 + 1; refuse(a, "misaligned col"); }
  { KzgvArgs a = ok; a.offsets = buf + 2624 + 2; refuse(a, "misaligned offsets"); }
  { KzgvArgs a = ok; a.verdict = buf + 1024 + 3; refuse(a, "verdict inside cells"); }
  { KzgvArgs a = ok; a.verdict = buf + 2688 + 63; refuse(a, "verdict on the last byte of r"); }
  { KzgvArgs a = ok; a.out_ab = buf + 2048; refuse(a, "out_ab on the proofs"); }
  { KzgvArgs a = ok; a.out_ab = buf + 2816 - 568; refuse(a, "out_ab over the verdicts"); }
  { KzgvArgs a = ok; a.device = false; a.cells = buf + 1024 + 8; CHECK(kzgv_check(a) == nullptr, "the host form has no alignment rule"); }
  { KzgvArgs a = ok; a.nseg = 0; a.m = 0; a.offsets = a.r = a.verdict = nullptr; CHECK(kzgv_check(a) == nullptr, "nseg = 0 is a no-op with NULL pointers"); }
  { KzgvArgs a = ok; a.m = 0; a.row = a.col = a.cells = a.proof_xy = a.proof_inf = nullptr; CHECK(kzgv_check(a) == nullptr, "empty batches need no cell arrays"); }
  // the shapes
  int shapes = 0;
  const int bad_shape[][2] = {{-1, 0}, {24, 0}, {4, -1}, {4, 5}, {20, 13}, {0x7fffffff, 0}, {4, (int)0x80000000}};
  for (auto& s : bad_shape) { shapes++; CHECK(kzgv_check_shape(s[0], s[1]) != nullptr, "shape (%d, %d) not refused", s[0], s[1]); CHECK(!kzgv_plan(s[0], s[1], 1, 1).ok, "plan of a bad shape"); }
  CHECK(kzgv_check_shape(23, 12) == nullptr && kzgv_check_shape(0, 0) == nullptr, "the extreme shapes are refused");
  CHECK(!kzgv_plan(4, 2, ~(uint64_t)0, 1).ok && !kzgv_plan(4, 2, 1, ~(uint64_t)0).ok && !kzgv_plan(4, 2, 1, 0).ok && !kzgv_plan(4, 2, 1, 1, 257).ok, "plan extremes");
  CHECK(kzgv_plan(23, 12, (uint64_t)1 << 15, (uint64_t)1 << 15).ok && kzgv_plan(23, 0, (uint64_t)1 << 24, (uint64_t)1 << 24).ok, "the largest calls are refused");
  // create
  KzgvCreateArgs c;
  c.srs_given = c.q_given = c.out_given = true; c.srs_group = 1; c.srs_len = 4; c.srs_subgroup = 1; c.log_n = 4; c.log_l = 2;
  CHECK(kzgv_check_create(c) == nullptr, "the good create is refused");
  { KzgvCreateArgs a = c; a.srs_given = false; n++; CHECK(kzgv_check_create(a), "create: NULL srs"); }
  { KzgvCreateArgs a = c; a.q_given = false; n++; CHECK(kzgv_check_create(a), "create: NULL q"); }
  { KzgvCreateArgs a = c; a.out_given = false; n++; CHECK(kzgv_check_create(a), "create: NULL out"); }
  { KzgvCreateArgs a = c; a.srs_group = 2; n++; CHECK(kzgv_check_create(a), "create: G2 srs"); }
  { KzgvCreateArgs a = c; a.srs_len = 3; n++; CHECK(kzgv_check_create(a), "create: short srs"); }
  { KzgvCreateArgs a = c; a.srs_subgroup = 0; n++; CHECK(kzgv_check_create(a), "create: subgroup state 0"); }
  { KzgvCreateArgs a = c; a.log_n = 24; n++; CHECK(kzgv_check_create(a), "create: log_n 24"); }
  { KzgvCreateArgs a = c; a.log_l = 5; n++; CHECK(kzgv_check_create(a), "create: log_l > log_n"); }
  // what only the host form sees
  const uint32_t row[4] = {0, 1, 1, 0}, col[4] = {0, 7, 3, 2};
  const uint32_t good[3] = {0, 1, 4};
  CHECK(kzgv_check_host(good, 2, 4, row, col, 2, 4, 2) == nullptr, "the good host call is refused");
  { const uint32_t o[3] = {1, 1, 4}; n++; CHECK(kzgv_check_host(o, 2, 4, row, col, 2, 4, 2), "host: offsets[0] != 0"); }
  { const uint32_t o[3] = {0, 5, 4}; n++; CHECK(kzgv_check_host(o, 2, 4, row, col, 2, 4, 2), "host: decreasing offsets"); }
  { n++; CHECK(kzgv_check_host(good, 2, 4, row, col, 1, 4, 2), "host: row >= ncommit"); }
  { const uint32_t cc[4] = {0, 8, 3, 2}; n++; CHECK(kzgv_check_host(good, 2, 4, row, cc, 2, 4, 2), "host: col >= 2c"); }
  printf("refusals %d shapes %d\n", n, shapes);
}

int main() {
  int plans = 0;
  for (int log_n = 0; log_n <= 8; log_n++)
    for (int log_l = 0; log_l <= log_n; log_l++) {
      for (uint32_t m : {0u, 1u, 5u, 300u})
        for (auto& off : cuts(m))
          for (uint32_t chunk : {0u, 1u, 3u, 4u}) { fold_model(log_n, log_l, off, chunk, "fold"); plans++; }
      // the exponent maps, for the Python side
      const uint64_t two_n = (uint64_t)2 << log_n, cells = (uint64_t)2 << (log_n - log_l);
      for (int order = 0; order < 2; order++)
        for (uint64_t col = 0; col < cells; col++) {
          const uint64_t e = kzgv_shift_exponent(col, log_n, log_l, order), a = kzgv_a_exponent(e, log_n, log_l);
          CHECK(e < cells && a < two_n && (a + (e << log_l)) % two_n == 0, "maps (%d, %d) order %d col %llu", log_n, log_l, order, (unsigned long long)col);
          for (uint64_t u : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << log_l) - 1}) CHECK(kzgv_inv_power_exponent(e, u, log_n) == (e * u) % two_n, "inverse power exponent");
          printf("map %d %d %d %llu %llu %llu\n", log_n, log_l, order, (unsigned long long)col, (unsigned long long)e, (unsigned long long)a);
        }
    }
  // the automatic cut at the sizes the measurements use and at the limits
  CHECK(kzgv_chunk(8192, 6) == 8 && kzgv_chunk(128, 6) == 1 && kzgv_chunk((uint64_t)1 << 24, 3) == KZGV_CHUNK_MAX, "the automatic chunk");
  printf("plans %d\n", plans);
  broken_offsets();
  refusals();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
