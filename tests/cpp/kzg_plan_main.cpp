// tests/cpp/kzg_plan_main.cpp -- bls12_381_amd/csrc/kzg_plan.h on its own (tests/test_kzg_plan.py builds this with host clang++
// -fsanitize=address,undefined and runs it; it includes nothing of the library but that header).
//
// The data movement of the amortised KZG openings is run as a MODEL over index arrays: every buffer has exactly the size the plan tells
// the host to reserve, every kernel's lanes are walked with the plan's grids, and the slots are filled through the header's index maps
// exactly as kzg.hip.h fills them.  Checked for every (log_n <= 8, log_l <= log_n), count in {0, 1, 3} and both tile shapes: every S^ and
// c^ slot is written exactly once and every SRS point / coefficient that belongs to a row is read exactly once, the transposition is a
// bijection onto the segment order, every segment's scalar and base range lies inside its array, both proof numberings and both cell
// numberings are bijections (and the bit-reversed ones are what bitrev(i l + t, log_n + 1) says), the scratch is never exceeded.  Then
// one call per refusal of the argument checks, 64-bit extremes included.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kzg_plan.h"

using namespace bls;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (g_fail > 20) exit(1); } } while (0)

static void create_model(int log_n, int log_l) {
  const KzgCreatePlan p = kzg_plan_create(log_n, log_l);
  CHECK(p.ok, "create %d %d refused", log_n, log_l);
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, c = n >> log_l;
  CHECK(p.n == n && p.l == l && p.c == c && p.msm == (c > 1), "create %d %d: shape", log_n, log_l);
  if (!p.msm) { CHECK(p.points == 0 && p.point_bytes == 0, "create %d %d: c = 1 reserves nothing", log_n, log_l); return; }
  CHECK(p.points == 2 * n && p.point_bytes == 2 * n * 144 && p.xy_bytes == 2 * n * 96 && p.inf_bytes == 2 * n, "create %d %d: sizes", log_n, log_l);
  CHECK((uint64_t)p.gather_grid * KZG_BLOCK >= 2 * n && (uint64_t)(p.gather_grid - 1) * KZG_BLOCK < 2 * n, "create %d %d: grid", log_n, log_l);
  // S^ [t][j]: every slot once; SRS point s is read once when s < (c - 1) l, never beyond
  std::vector<int> slot(p.point_bytes / 144, 0), read(n, 0);
  for (uint64_t g = 0; g < (uint64_t)p.gather_grid * KZG_BLOCK; g++) {
    if (g >= 2 * n) continue;
    const uint64_t t = g >> (p.log_c + 1), j = g & (2 * c - 1);
    const int64_t s = kzg_srs_slot(t, j, p.log_c, log_l);
    CHECK(s < (int64_t)n, "create %d %d: SRS index %lld", log_n, log_l, (long long)s);
    slot[g]++;
    if (s >= 0) { read[s]++; CHECK(j <= c - 2 && (uint64_t)s == (c - 2 - j) * l + t, "create %d %d: S^ slot", log_n, log_l); }
    else CHECK(j > c - 2 || c < 2, "create %d %d: an identity too early", log_n, log_l);
  }
  for (uint64_t g = 0; g < 2 * n; g++) CHECK(slot[g] == 1, "create %d %d: slot %llu written %d times", log_n, log_l, (unsigned long long)g, slot[g]);
  for (uint64_t s = 0; s < n; s++) CHECK(read[s] == (s < (c - 1) * l ? 1 : 0), "create %d %d: S[%llu] read %d times", log_n, log_l, (unsigned long long)s, read[s]);
  // [t][m] -> [m][t]
  std::vector<int> hit(2 * n, 0);
  for (uint64_t i = 0; i < 2 * n; i++) {
    const uint64_t src = kzg_transposed_src(i >> log_l, i & (l - 1), p.log_c);
    CHECK(src < 2 * n, "create %d %d: transposed source", log_n, log_l);
    if (src < 2 * n) hit[src]++;
    CHECK(src == (i & (l - 1)) * 2 * c + (i >> log_l), "create %d %d: transposition", log_n, log_l);
  }
  for (uint64_t i = 0; i < 2 * n; i++) CHECK(hit[i] == 1, "create %d %d: the transposition is no bijection", log_n, log_l);
}

static void transpose_model(const KzgTranspose& tp, uint64_t vecs, int log_r, int log_cc, int brev, const char* what) {
  const uint64_t R = (uint64_t)1 << log_r, C = (uint64_t)1 << log_cc, T = tp.tile;
  CHECK(tp.block == T * T && tp.grid == vecs * tp.tiles_r * tp.tiles_c && tp.tiles_r * T >= R && tp.tiles_c * T >= C && tp.lds <= 64 * 1024, "%s: transposition plan", what);
  std::vector<int> rd(vecs * R * C, 0), wr(vecs * R * C, 0);
  for (uint64_t b0 = 0; b0 < tp.grid; b0++) {
    uint64_t b = b0;
    const uint64_t tc = b % tp.tiles_c; b /= tp.tiles_c;
    const uint64_t tr = b % tp.tiles_r; b /= tp.tiles_r;
    const uint64_t v = b;
    CHECK(v < vecs, "%s: a workgroup beyond the last matrix", what);
    for (uint64_t y = 0; y < T; y++) for (uint64_t x = 0; x < T; x++) {
      const uint64_t r = tr * T + y, cc = tc * T + x;
      if (r < R && cc < C) {
        const uint64_t sr = brev ? kzg_bitrev(r, log_r) : r, sc = brev ? kzg_bitrev(cc, log_cc) : cc;
        CHECK(sr < R && sc < C, "%s: source outside the matrix", what);
        rd[(v << (log_r + log_cc)) + (sr << log_cc) + sc]++;
      }
      const uint64_t wc = tc * T + y, wrow = tr * T + x;
      if (wrow < R && wc < C) wr[(v << (log_r + log_cc)) + (wc << log_r) + wrow]++;
    }
  }
  for (size_t i = 0; i < rd.size(); i++) CHECK(rd[i] == 1 && wr[i] == 1, "%s: element %zu read %d / written %d times", what, i, rd[i], wr[i]);
}

static void proofs_model(int log_n, int log_l, uint64_t count, int form, unsigned tile) {
  char what[96];
  snprintf(what, sizeof what, "proofs (%d, %d) x %llu form %d tile %u", log_n, log_l, (unsigned long long)count, form, tile);
  const KzgPlan p = kzg_plan_proofs(log_n, log_l, count, form, tile);
  CHECK(p.ok, "%s: refused", what);
  if (!p.ok) return;
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, c = n >> log_l;
  CHECK(p.scalars == count * 2 * n && p.points == count * 2 * c && p.vectors == count * l && p.msm == (c > 1 && count > 0), "%s: shape", what);
  if (!p.msm) {
    CHECK(p.rows_bytes == 0 && p.point_bytes == 0 && (uint64_t)p.fill_grid * KZG_BLOCK >= p.points, "%s: nothing but the fill", what);
    return;
  }
  CHECK(p.rows_bytes == p.scalars * 32 && p.seg_bytes == p.scalars * 32 && p.point_bytes == p.points * 144 && p.offset_bytes == (p.points + 1) * 4 && p.base_first_bytes == p.points * 4,
        "%s: scratch", what);
  CHECK(p.coeff_bytes == (form == KZG_FORM_EVALS ? count * n * 32 : 0) && (form != KZG_FORM_EVALS || (uint64_t)p.copy_grid * KZG_BLOCK >= count * n), "%s: the copy", what);
  // the rows c^_t: every slot once, every coefficient p[l .. n) once, p[0 .. l) never
  std::vector<int> slot(p.rows_bytes / 32, 0), read(count * n, 0);
  for (uint64_t g = 0; g < (uint64_t)p.rows_grid * KZG_BLOCK; g++) {
    if (g >= p.scalars) continue;
    const uint64_t v = g >> (log_n + 1), t = (g >> (p.log_c + 1)) & (l - 1), j = g & (2 * c - 1);
    const int64_t s = kzg_coeff_slot(t, j, p.log_c, log_l);
    CHECK(s < (int64_t)n, "%s: coefficient index %lld", what, (long long)s);
    slot[g]++;
    if (s >= 0 && s < (int64_t)n) read[v * n + s]++;
    if (j >= 1 && j <= c + 1) CHECK(s < 0, "%s: zero slot %llu holds a coefficient", what, (unsigned long long)j);
  }
  for (uint64_t g = 0; g < p.scalars; g++) CHECK(slot[g] == 1, "%s: row slot written %d times", what, slot[g]);
  for (uint64_t i = 0; i < count * n; i++) CHECK(read[i] == ((i & (n - 1)) >= l ? 1 : 0), "%s: coefficient %llu read %d times", what, (unsigned long long)i, read[i]);
  transpose_model(p.transpose, count, log_l, p.log_c + 1, 0, what);
  // the segments
  CHECK((uint64_t)p.seg_grid * KZG_BLOCK >= p.points + 1, "%s: segment grid", what);
  std::vector<uint32_t> off(p.offset_bytes / 4, 0xFFFFFFFFu), bf(p.base_first_bytes / 4, 0xFFFFFFFFu);
  for (uint64_t s = 0; s <= p.points; s++) { off[s] = kzg_seg_offset(s, log_l); if (s < p.points) bf[s] = kzg_seg_base_first(s, p.log_c, log_l); }
  CHECK(off[0] == 0 && off[p.points] == p.scalars, "%s: offsets", what);
  for (uint64_t s = 0; s < p.points; s++) {
    CHECK(off[s + 1] - off[s] == l && off[s + 1] <= p.scalars, "%s: segment %llu scalars", what, (unsigned long long)s);
    CHECK((uint64_t)bf[s] + l <= 2 * n && bf[s] == (s % (2 * c)) * l, "%s: segment %llu bases", what, (unsigned long long)s);
  }
  // the fill and both numberings
  CHECK((uint64_t)p.fill_grid * KZG_BLOCK >= count * c && (uint64_t)p.permute_grid * KZG_BLOCK >= p.points, "%s: fill / permute grids", what);
  for (int order = 0; order < 2; order++) {
    std::vector<int> hit(2 * c, 0);
    for (uint64_t i = 0; i < 2 * c; i++) {
      const uint64_t s = kzg_proof_src(i, p.log_c, order);
      CHECK(s < 2 * c, "%s: proof source", what);
      if (s < 2 * c) hit[s]++;
      // the coset of cell i: entry 0 of the cell is the point w^(h-exponent), so the proof's transform index is that exponent
      CHECK(s == (order ? kzg_bitrev(i << log_l, log_n + 1) : i), "%s: proof %llu order %d", what, (unsigned long long)i, order);
    }
    for (uint64_t i = 0; i < 2 * c; i++) CHECK(hit[i] == 1, "%s: proof numbering %d is no bijection", what, order);
  }
}

static void cells_model(int log_n, int log_l, uint64_t count, int form, unsigned tile) {
  char what[96];
  snprintf(what, sizeof what, "cells (%d, %d) x %llu form %d tile %u", log_n, log_l, (unsigned long long)count, form, tile);
  const KzgCellsPlan p = kzg_plan_cells(log_n, log_l, count, form, tile);
  CHECK(p.ok, "%s: refused", what);
  if (!p.ok || !count) return;
  const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, c = n >> log_l;
  CHECK(p.scalars == count * 2 * n && p.ext_bytes == p.scalars * 32 && (uint64_t)p.extend_grid * KZG_BLOCK >= p.scalars, "%s: sizes", what);
  CHECK(p.coeff_bytes == (form == KZG_FORM_EVALS ? count * n * 32 : 0), "%s: the copy", what);
  for (int order = 0; order < 2; order++) {
    transpose_model(p.map, count, log_l, p.log_c + 1, order, what);
    std::vector<int> hit(2 * n, 0);
    for (uint64_t i = 0; i < 2 * c; i++) for (uint64_t t = 0; t < l; t++) {
      const uint64_t s = kzg_cell_src(i, t, p.log_c, log_l, order);
      CHECK(s < 2 * n, "%s: cell source", what);
      if (s < 2 * n) hit[s]++;
      CHECK(s == (order ? kzg_bitrev(i * l + t, log_n + 1) : i + 2 * c * t), "%s: cell (%llu, %llu) order %d", what, (unsigned long long)i, (unsigned long long)t, order);
      // the tiled map reads source row (t or its reversal), source column (i or its reversal)
      const uint64_t sr = order ? kzg_bitrev(t, log_l) : t, sc = order ? kzg_bitrev(i, p.log_c + 1) : i;
      CHECK(s == (sr << (p.log_c + 1)) + sc, "%s: the tiled map disagrees with the cell map", what);
    }
    for (uint64_t i = 0; i < 2 * n; i++) CHECK(hit[i] == 1, "%s: cell numbering %d is no bijection", what, order);
  }
}

static void refusals() {
  static char buf[1 << 16];
  const void* in = buf; const void* out = buf + (1 << 15);
  // create
  KzgCreateArgs c;
  c.srs_given = true; c.out_given = true; c.srs_group = 1; c.srs_len = 16; c.srs_subgroup = 1; c.log_n = 4; c.log_l = 2;
  CHECK(!kzg_check_create(c), "create: the good call is refused");
  { KzgCreateArgs a = c; a.srs_given = false; CHECK(kzg_check_create(a), "create: NULL srs"); }
  { KzgCreateArgs a = c; a.out_given = false; CHECK(kzg_check_create(a), "create: NULL out"); }
  { KzgCreateArgs a = c; a.srs_group = 2; CHECK(kzg_check_create(a), "create: G2"); }
  { KzgCreateArgs a = c; a.srs_len = 15; CHECK(kzg_check_create(a), "create: short SRS"); }
  { KzgCreateArgs a = c; a.srs_subgroup = 0; CHECK(kzg_check_create(a), "create: off-subgroup SRS"); }
  { KzgCreateArgs a = c; a.srs_subgroup = 2; CHECK(!kzg_check_create(a), "create: an assumed SRS is fine"); }
  { KzgCreateArgs a = c; a.log_n = -1; CHECK(kzg_check_create(a), "create: log_n < 0"); }
  { KzgCreateArgs a = c; a.log_n = 24; a.srs_len = ~(uint64_t)0; CHECK(kzg_check_create(a), "create: log_n = 24"); }
  { KzgCreateArgs a = c; a.log_n = 23; a.log_l = 12; a.srs_len = (uint64_t)1 << 23; CHECK(!kzg_check_create(a), "create: the largest shape"); }
  { KzgCreateArgs a = c; a.log_l = 5; CHECK(kzg_check_create(a), "create: log_l > log_n"); }
  { KzgCreateArgs a = c; a.log_l = -1; CHECK(kzg_check_create(a), "create: log_l < 0"); }
  { KzgCreateArgs a = c; a.log_n = 13; a.log_l = 13; a.srs_len = 1 << 13; CHECK(kzg_check_create(a), "create: log_l = 13"); }
  CHECK(!kzg_plan_create(24, 0).ok && !kzg_plan_create(4, 5).ok && !kzg_plan_create(-1, 0).ok && !kzg_plan_create(0, -1).ok, "create plan refusals");
  // proofs
  KzgProofsArgs p;
  p.handle_given = true; p.log_n = 4; p.log_l = 2; p.polys = in; p.out = out; p.count = 3; p.device = true;
  CHECK(!kzg_check_proofs(p), "proofs: the good call is refused");
  { KzgProofsArgs a = p; a.handle_given = false; CHECK(kzg_check_proofs(a), "proofs: NULL handle"); }
  { KzgProofsArgs a = p; a.polys = nullptr; CHECK(kzg_check_proofs(a), "proofs: NULL polys"); }
  { KzgProofsArgs a = p; a.out = nullptr; CHECK(kzg_check_proofs(a), "proofs: NULL out"); }
  { KzgProofsArgs a = p; a.polys = nullptr; a.out = nullptr; a.count = 0; CHECK(!kzg_check_proofs(a), "proofs: count = 0 is a no-op"); }
  { KzgProofsArgs a = p; a.form = 2; CHECK(kzg_check_proofs(a), "proofs: form 2"); }
  { KzgProofsArgs a = p; a.form = -1; CHECK(kzg_check_proofs(a), "proofs: form -1"); }
  { KzgProofsArgs a = p; a.order = 2; CHECK(kzg_check_proofs(a), "proofs: order 2"); }
  { KzgProofsArgs a = p; a.order = -1; CHECK(kzg_check_proofs(a), "proofs: order -1"); }
  { KzgProofsArgs a = p; a.count = ((uint64_t)1 << 22) + 1; CHECK(kzg_check_proofs(a), "proofs: count * 2n > 2^27"); }
  { KzgProofsArgs a = p; a.count = (uint64_t)1 << 22; a.polys = nullptr; a.out = nullptr; CHECK(kzg_check_proofs(a), "proofs: the largest count still needs its pointers"); }
  { KzgProofsArgs a = p; a.count = (uint64_t)1 << 63; CHECK(kzg_check_proofs(a), "proofs: count = 2^63"); }
  { KzgProofsArgs a = p; a.count = ~(uint64_t)0; CHECK(kzg_check_proofs(a), "proofs: count = 2^64 - 1"); }
  { KzgProofsArgs a = p; a.count = ((uint64_t)1 << 59) + 1; CHECK(kzg_check_proofs(a), "proofs: count * 2n wraps to 32"); }
  { KzgProofsArgs a = p; a.log_n = 12; a.log_l = 0; a.count = ((uint64_t)1 << 11) + 1; CHECK(kzg_check_proofs(a), "proofs: count * 2c > 2^24"); }
  { KzgProofsArgs a = p; a.log_n = 12; a.log_l = 0; a.count = (uint64_t)1 << 11; a.polys = nullptr; a.out = nullptr; const char* w = kzg_check_proofs(a);
    CHECK(w && kzg_plan_proofs(12, 0, (uint64_t)1 << 11, 0).ok, "proofs: count * 2c = 2^24 passes the limits"); }
  { KzgProofsArgs a = p; a.polys = buf + 8; CHECK(kzg_check_proofs(a), "proofs: misaligned polys"); }
  { KzgProofsArgs a = p; a.out = buf + (1 << 15) + 8; CHECK(kzg_check_proofs(a), "proofs: misaligned out"); }
  { KzgProofsArgs a = p; a.polys = buf + 8; a.device = false; CHECK(!kzg_check_proofs(a), "proofs: the host form takes any alignment"); }
  { KzgProofsArgs a = p; a.out = buf + 3 * 16 * 32 - 16; CHECK(kzg_check_proofs(a), "proofs: the output starts inside the input"); }
  { KzgProofsArgs a = p; a.out = buf + 3 * 16 * 32; CHECK(!kzg_check_proofs(a), "proofs: the output right behind the input"); }
  { KzgProofsArgs a = p; a.polys = buf + 3 * 8 * 144 - 16; a.out = buf; CHECK(kzg_check_proofs(a), "proofs: the input starts inside the output"); }
  { KzgProofsArgs a = p; a.log_n = 24; CHECK(kzg_check_proofs(a), "proofs: a handle cannot have log_n = 24"); }
  CHECK(!kzg_plan_proofs(4, 2, ((uint64_t)1 << 22) + 1, 0).ok && !kzg_plan_proofs(4, 2, ~(uint64_t)0, 0).ok && !kzg_plan_proofs(4, 2, 1, 2).ok && !kzg_plan_proofs(4, 2, 1, 0, 0).ok &&
        !kzg_plan_proofs(4, 2, 1, 0, 33).ok, "proofs plan refusals");
  // cells
  KzgCellsArgs e;
  e.polys = in; e.cells = out; e.log_n = 4; e.log_l = 2; e.count = 3; e.device = true;
  CHECK(!kzg_check_cells(e), "cells: the good call is refused");
  { KzgCellsArgs a = e; a.polys = nullptr; CHECK(kzg_check_cells(a), "cells: NULL polys"); }
  { KzgCellsArgs a = e; a.cells = nullptr; CHECK(kzg_check_cells(a), "cells: NULL cells"); }
  { KzgCellsArgs a = e; a.polys = nullptr; a.cells = nullptr; a.count = 0; CHECK(!kzg_check_cells(a), "cells: count = 0 is a no-op"); }
  { KzgCellsArgs a = e; a.log_n = 28; CHECK(kzg_check_cells(a), "cells: log_n = 28"); }
  { KzgCellsArgs a = e; a.log_n = -1; CHECK(kzg_check_cells(a), "cells: log_n < 0"); }
  { KzgCellsArgs a = e; a.log_n = 27; a.log_l = 12; a.count = 1; a.polys = nullptr; a.cells = nullptr; CHECK(kzg_check_cells(a) && kzg_plan_cells(27, 12, 1, 0).ok, "cells: the largest shape passes the limits"); }
  { KzgCellsArgs a = e; a.log_n = 27; a.count = 2; CHECK(kzg_check_cells(a), "cells: count * 2n > 2^28"); }
  { KzgCellsArgs a = e; a.log_l = 5; CHECK(kzg_check_cells(a), "cells: log_l > log_n"); }
  { KzgCellsArgs a = e; a.log_n = 14; a.log_l = 13; CHECK(kzg_check_cells(a), "cells: log_l = 13"); }
  { KzgCellsArgs a = e; a.log_l = -1; CHECK(kzg_check_cells(a), "cells: log_l < 0"); }
  { KzgCellsArgs a = e; a.form = 2; CHECK(kzg_check_cells(a), "cells: form"); }
  { KzgCellsArgs a = e; a.order = 2; CHECK(kzg_check_cells(a), "cells: order"); }
  { KzgCellsArgs a = e; a.count = ((uint64_t)1 << 23) + 1; CHECK(kzg_check_cells(a), "cells: count * 2n > 2^28"); }
  { KzgCellsArgs a = e; a.count = (uint64_t)1 << 63; CHECK(kzg_check_cells(a), "cells: count = 2^63"); }
  { KzgCellsArgs a = e; a.count = ((uint64_t)1 << 59) + 1; CHECK(kzg_check_cells(a), "cells: count * 2n wraps"); }
  { KzgCellsArgs a = e; a.polys = buf + 8; CHECK(kzg_check_cells(a), "cells: misaligned polys"); }
  { KzgCellsArgs a = e; a.cells = buf + (1 << 15) + 4; CHECK(kzg_check_cells(a), "cells: misaligned cells"); }
  { KzgCellsArgs a = e; a.cells = buf + 3 * 16 * 32 - 16; CHECK(kzg_check_cells(a), "cells: the output starts inside the input"); }
  { KzgCellsArgs a = e; a.cells = buf + 3 * 16 * 32; CHECK(!kzg_check_cells(a), "cells: the output right behind the input"); }
  { KzgCellsArgs a = e; a.cells = buf; CHECK(kzg_check_cells(a), "cells: in place"); }
  CHECK(!kzg_plan_cells(28, 0, 1, 0).ok && !kzg_plan_cells(4, 2, ((uint64_t)1 << 23) + 1, 0).ok && !kzg_plan_cells(4, 2, 1, 3).ok, "cells plan refusals");
}

int main() {
  for (int log_n = 0; log_n <= 8; log_n++)
    for (int log_l = 0; log_l <= log_n; log_l++) {
      create_model(log_n, log_l);
      for (uint64_t count : {0, 1, 3})
        for (int form = 0; form < 2; form++)
          for (unsigned tile : {4u, (unsigned)KZG_TILE}) { proofs_model(log_n, log_l, count, form, tile); cells_model(log_n, log_l, count, form, tile); }
    }
  printf("plans\n");
  refusals();
  printf("refusals\n");
  if (g_fail) { printf("%d failures\n", g_fail); return 1; }
  printf("all ok\n");
  return 0;
}
