// kzg_plan.h -- amortised KZG openings (blsgpu_kzg_multiproof_*, blsgpu_kzg_cells*) as plain host code: the limits and every argument
// check, every index map of the circulant route (FK20), the segments of the Toeplitz MSM, the scratch sizes and the launch shapes.  No
// HIP calls here: api_msm.hip launches from the plan, kzg.hip.h reads the maps through the KZG_HD functions below,
// tests/simt/emu_kzg.cpp walks the same plan on the host and tests/cpp/kzg_plan_main.cpp sweeps it under sanitizers.
//
// Notation: n = 2^log_n coefficients, l = 2^log_l points per cell, c = n / l, w the root of order 2n, 2c cells per polynomial.
//   h_d = sum_{s < c-1-d} sum_{t < l} p[(s+d+1) l + t] S[s l + t]   (d < c)        proofs (natural order) = G1-NTT_2c(h_0 .. h_{c-1}, identity x c)
// The h_d are l circulant products of size 2c, one per residue t, summed over t:
//   S^_t = (S[(c-2) l + t], ..., S[t], identity x (c+1))                  per SRS, once: X^_t = G1-NTT_2c(S^_t), resident as bases [m][t]
//   c^_t = (p[(c-1) l + t], 0 x (c+1), p[l + t], ..., p[(c-2) l + t])     per call:      f_t = fr-NTT_2c(c^_t), transposed to [v][m][t]
//   (h | junk)[m] = inverse-G1-NTT_2c over m of sum_t f_t[m] X^_t[m]      the sum over t is segment (v, m) of ONE segmented MSM
// The stages of blsgpu_kzg_multiproof_proofs_device, in order (each a launch sequence that depends on the shape alone):
//   [evals only] copy (bit-reversed for ORDER_BITREV) + inverse fr_ntt_many   ->  rows c^_t  ->  fr_ntt_many (log 2c, count l vectors)  ->
//   transposition  ->  segment offsets  ->  g1_msm_segments  ->  inverse g1_ntt_many  ->  identities over the upper c  ->  g1_ntt_many  ->
//   point permutation into the caller's array (identity, or bitrev(i, log 2c)).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KZG_HD __host__ __device__ inline
#else
#define KZG_HD inline
#endif

// side of the square LDS tile of the transposition, in scalars (-D overrides; the host emulation also runs a tile of 4)
#ifndef KZG_TILE
#define KZG_TILE 16
#endif

namespace bls {

constexpr int KZG_FORM_COEFFS = 0, KZG_FORM_EVALS = 1;       // BLSGPU_KZG_FORM_*
constexpr int KZG_ORDER_NATURAL = 0, KZG_ORDER_BITREV = 1;   // BLSGPU_FR_ORDER_*
constexpr int KZG_MAX_LOG_N = 23;                            // multiproofs: 2n points through g1_ntt_many (2^24)
constexpr int KZG_MAX_LOG_L = 12;                            // l <= BLSGPU_SEG_LEN_MAX: a segment of the Toeplitz MSM holds l terms
constexpr int KZG_MAX_LOG_TERMS = 27;                        // count * 2n: the `total` of msm_segments
constexpr int KZG_MAX_LOG_POINTS = 24;                       // count * 2c: the group transform's limit
constexpr int KZG_CELLS_MAX_LOG_N = 27;                      // cells alone: the size-2n Fr transform (log <= 28)
constexpr int KZG_CELLS_MAX_LOG_TOTAL = 28;                  // count * 2n of blsgpu_kzg_cells
constexpr unsigned KZG_BLOCK = 256;                          // lanes per workgroup of the one-item-per-lane kernels

// ---- index maps, as the kernels read them ------------------------------------------------------------------------------------------
KZG_HD uint64_t kzg_bitrev(uint64_t i, int bits) {
  uint64_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}
// S^_t[j], j < 2c: the SRS index it holds, or -1 for the identity.  c = 2^log_c, l = 2^log_l.
KZG_HD int64_t kzg_srs_slot(uint64_t t, uint64_t j, int log_c, int log_l) {
  const uint64_t c = (uint64_t)1 << log_c;
  if (j + 2 > c) return -1;                                  // j > c - 2 (c = 1: every j)
  return (int64_t)(((c - 2 - j) << log_l) + t);
}
// c^_t[j], j < 2c: the coefficient index it holds, or -1 for zero
KZG_HD int64_t kzg_coeff_slot(uint64_t t, uint64_t j, int log_c, int log_l) {
  const uint64_t c = (uint64_t)1 << log_c;
  if (j == 0) return (int64_t)(((c - 1) << log_l) + t);
  if (j < c + 2) return -1;                                  // the c + 1 zeros
  return (int64_t)(((j - c - 1) << log_l) + t);              // j = c + 2 .. 2c - 1: p[l + t] .. p[(c-2) l + t]
}
// the transposition [v][t][m] -> [v][m][t] inside one polynomial's 2n scalars: where element (m, t) of the segment order comes from
KZG_HD uint64_t kzg_transposed_src(uint64_t m, uint64_t t, int log_c) { return (t << (log_c + 1)) + m; }
// proof i of a polynomial is point kzg_proof_src(i) of the natural-order transform
KZG_HD uint64_t kzg_proof_src(uint64_t i, int log_c, int order) { return order == KZG_ORDER_BITREV ? kzg_bitrev(i, log_c + 1) : i; }
// cells[i][t] is E[kzg_cell_src], E the size-2n transform: natural i + 2c t; bit-reversed bitrev(i l + t, log_n + 1)
KZG_HD uint64_t kzg_cell_src(uint64_t i, uint64_t t, int log_c, int log_l, int order) {
  if (order == KZG_ORDER_BITREV) return (kzg_bitrev(t, log_l) << (log_c + 1)) + kzg_bitrev(i, log_c + 1);
  return i + (t << (log_c + 1));
}
// segment s = v 2c + m of the Toeplitz MSM: scalars [s l, s l + l), bases [m l, m l + l)
KZG_HD uint32_t kzg_seg_offset(uint64_t s, int log_l) { return (uint32_t)(s << log_l); }
KZG_HD uint32_t kzg_seg_base_first(uint64_t s, int log_c, int log_l) { return (uint32_t)((s & (((uint64_t)2 << log_c) - 1)) << log_l); }

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal -------------------------------------------------
inline bool kzg_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
// count * 2^log_unit <= 2^log_max without overflow
inline bool kzg_fits(uint64_t count, int log_unit, int log_max) { return log_unit <= log_max && count <= ((uint64_t)1 << (log_max - log_unit)); }

struct KzgCreateArgs {
  bool srs_given = false; int srs_group = 0; uint64_t srs_len = 0; int srs_subgroup = 0;
  int log_n = 0, log_l = 0; bool out_given = false;
};
inline const char* kzg_check_shape(int log_n, int log_l) {
  if (log_n < 0 || log_n > KZG_MAX_LOG_N) return "kzg_multiproof: log_n must be in [0, 23]";
  if (log_l < 0 || log_l > log_n || log_l > KZG_MAX_LOG_L) return "kzg_multiproof: log_l must be in [0, min(log_n, 12)]";
  return nullptr;
}
inline const char* kzg_check_create(const KzgCreateArgs& a) {
  if (!a.srs_given || !a.out_given) return "kzg_multiproof_create: NULL argument";
  if (const char* why = kzg_check_shape(a.log_n, a.log_l)) return why;
  if (a.srs_group != 1) return "kzg_multiproof_create: the SRS must be a G1 base set";
  if (a.srs_len < ((uint64_t)1 << a.log_n)) return "kzg_multiproof_create: the SRS holds fewer than 2^log_n points";
  if (a.srs_subgroup == 0) return "kzg_multiproof_create: the SRS holds a point outside the prime-order subgroup";
  return nullptr;
}

struct KzgProofsArgs {
  bool handle_given = false; int log_n = 0, log_l = 0;
  const void* polys = nullptr; uint64_t count = 0; int form = 0, order = 0; const void* out = nullptr;
  bool device = false;
};
inline const char* kzg_check_proofs(const KzgProofsArgs& a) {
  if (!a.handle_given) return "kzg_multiproof_proofs: NULL handle";
  if (const char* why = kzg_check_shape(a.log_n, a.log_l)) return why;
  if (a.form != KZG_FORM_COEFFS && a.form != KZG_FORM_EVALS) return "kzg_multiproof_proofs: unknown form";
  if (a.order != KZG_ORDER_NATURAL && a.order != KZG_ORDER_BITREV) return "kzg_multiproof_proofs: unknown order";
  if (!kzg_fits(a.count, a.log_n + 1, KZG_MAX_LOG_TERMS)) return "kzg_multiproof_proofs: count * 2n must not exceed 2^27";
  if (!kzg_fits(a.count, a.log_n - a.log_l + 1, KZG_MAX_LOG_POINTS)) return "kzg_multiproof_proofs: count * 2c must not exceed 2^24";
  if (!a.count) return nullptr;
  if (!a.polys || !a.out) return "kzg_multiproof_proofs: NULL argument with polynomials to open";
  if (a.device && (((uintptr_t)a.polys | (uintptr_t)a.out) & 15)) return "kzg_multiproof_proofs_device: device pointers must be 16-byte aligned";
  if (kzg_overlap(a.out, (a.count << (a.log_n - a.log_l + 1)) * 144, a.polys, (a.count << a.log_n) * 32)) return "kzg_multiproof_proofs: the output overlaps the input (there is no in-place form)";
  return nullptr;
}

struct KzgCellsArgs {
  const void* polys = nullptr; int log_n = 0, log_l = 0; uint64_t count = 0; int form = 0, order = 0; const void* cells = nullptr;
  bool device = false;
};
inline const char* kzg_check_cells(const KzgCellsArgs& a) {
  if (a.log_n < 0 || a.log_n > KZG_CELLS_MAX_LOG_N) return "kzg_cells: log_n must be in [0, 27]";
  if (a.log_l < 0 || a.log_l > a.log_n || a.log_l > KZG_MAX_LOG_L) return "kzg_cells: log_l must be in [0, min(log_n, 12)]";
  if (a.form != KZG_FORM_COEFFS && a.form != KZG_FORM_EVALS) return "kzg_cells: unknown form";
  if (a.order != KZG_ORDER_NATURAL && a.order != KZG_ORDER_BITREV) return "kzg_cells: unknown order";
  if (!kzg_fits(a.count, a.log_n + 1, KZG_CELLS_MAX_LOG_TOTAL)) return "kzg_cells: count * 2n must not exceed 2^28";
  if (!a.count) return nullptr;
  if (!a.polys || !a.cells) return "kzg_cells: NULL argument with polynomials to evaluate";
  if (a.device && (((uintptr_t)a.polys | (uintptr_t)a.cells) & 15)) return "kzg_cells_device: device pointers must be 16-byte aligned";
  if (kzg_overlap(a.cells, (a.count << (a.log_n + 1)) * 32, a.polys, (a.count << a.log_n) * 32)) return "kzg_cells: the output overlaps the input (there is no in-place form)";
  return nullptr;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
// the tiled transposition of `vecs` matrices of rows x cols scalars: one workgroup of tile x tile lanes per tile, tiles of a matrix
// row-major, matrices one after the other
struct KzgTranspose {
  unsigned tile = 0, block = 0, grid = 0;
  uint64_t tiles_r = 0, tiles_c = 0;   // tiles along the SOURCE rows / columns
  size_t lds = 0;                      // static in the kernel: 2 x tile x (tile + 1) words of 16 bytes
};
inline KzgTranspose kzg_transpose_plan(uint64_t vecs, int log_rows, int log_cols, unsigned tile = KZG_TILE) {
  KzgTranspose p;
  p.tile = tile; p.block = tile * tile;
  p.tiles_r = (((uint64_t)1 << log_rows) + tile - 1) / tile;
  p.tiles_c = (((uint64_t)1 << log_cols) + tile - 1) / tile;
  p.grid = (unsigned)(vecs * p.tiles_r * p.tiles_c);
  p.lds = (size_t)2 * tile * (tile + 1) * 16;
  return p;
}
inline unsigned kzg_grid(uint64_t items) { return (unsigned)((items + KZG_BLOCK - 1) / KZG_BLOCK); }

struct KzgPlan {
  int ok = 0;
  int log_n = 0, log_l = 0, log_c = 0;
  uint64_t count = 0, n = 0, l = 0, c = 0;
  uint64_t scalars = 0;                // count * 2n: the rows c^_t, the segment-order copy, the terms of the MSM
  uint64_t points = 0;                 // count * 2c: the segments, the proofs
  uint64_t vectors = 0;                // count * l: the Fr transforms of size 2c
  bool msm = false;                    // c > 1: with c = 1 every proof is the identity and nothing but the fill runs
  // scratch of the context, in bytes
  size_t coeff_bytes = 0;              // the coefficients of an evaluation-form input (count * n scalars), else 0
  size_t rows_bytes = 0, seg_bytes = 0;                      // the rows c^_t / the segment-order copy, count * 2n scalars each
  size_t point_bytes = 0;              // count * 2c projective wire points
  size_t offset_bytes = 0, base_first_bytes = 0;             // (points + 1) / points u32
  // launches
  unsigned copy_grid = 0;              // evaluation form: a lane per scalar of the copy
  unsigned rows_grid = 0;              // a lane per scalar of the rows
  KzgTranspose transpose;              // [v][t][m] -> [v][m][t]: count matrices of l rows x 2c columns
  unsigned seg_grid = 0;               // a lane per segment (+ the closing offset)
  unsigned fill_grid = 0;              // a lane per identity record: count * c (c = 1: count * 2)
  unsigned permute_grid = 0;           // a lane per proof
};
inline KzgPlan kzg_plan_proofs(int log_n, int log_l, uint64_t count, int form, unsigned tile = KZG_TILE) {
  KzgPlan p;
  KzgProofsArgs a;                                             // the ranges alone: count = 0 stops the check before the pointers
  a.handle_given = true; a.log_n = log_n; a.log_l = log_l; a.form = form;
  if (kzg_check_proofs(a) || !kzg_fits(count, log_n + 1, KZG_MAX_LOG_TERMS) || !kzg_fits(count, log_n - log_l + 1, KZG_MAX_LOG_POINTS) || tile < 1 || tile > 32) return p;
  p.log_n = log_n; p.log_l = log_l; p.log_c = log_n - log_l; p.count = count;
  p.n = (uint64_t)1 << log_n; p.l = (uint64_t)1 << log_l; p.c = (uint64_t)1 << p.log_c;
  p.scalars = count << (log_n + 1); p.points = count << (p.log_c + 1); p.vectors = count << log_l;
  p.msm = p.c > 1 && count > 0;
  p.ok = 1;
  p.fill_grid = kzg_grid(p.msm ? count << p.log_c : p.points);
  if (!p.msm) return p;
  p.coeff_bytes = form == KZG_FORM_EVALS ? (size_t)(count << log_n) * 32 : 0;
  p.rows_bytes = p.seg_bytes = (size_t)p.scalars * 32;
  p.point_bytes = (size_t)p.points * 144;
  p.offset_bytes = (size_t)(p.points + 1) * 4; p.base_first_bytes = (size_t)p.points * 4;
  p.copy_grid = form == KZG_FORM_EVALS ? kzg_grid(count << log_n) : 0;
  p.rows_grid = kzg_grid(p.scalars);
  p.transpose = kzg_transpose_plan(count, log_l, p.log_c + 1, tile);
  p.seg_grid = kzg_grid(p.points + 1);
  p.permute_grid = kzg_grid(p.points);
  return p;
}

// create: S^ (2n points) gathered, transformed, transposed to [m][t], normalised, imported as bases
struct KzgCreatePlan {
  int ok = 0;
  int log_c = 0; uint64_t n = 0, l = 0, c = 0;
  bool msm = false;                    // c > 1: else the handle keeps no bases
  uint64_t points = 0;                 // 2n
  size_t xy_bytes = 0, inf_bytes = 0;  // the SRS prefix in wire form (n points), then X^ in affine wire form (2n points)
  size_t point_bytes = 0;              // two arrays of 2n projective wire points: S^ [t][j] and its transform in [m][t]
  unsigned gather_grid = 0, permute_grid = 0;
};
inline KzgCreatePlan kzg_plan_create(int log_n, int log_l) {
  KzgCreatePlan p;
  if (kzg_check_shape(log_n, log_l)) return p;
  p.log_c = log_n - log_l; p.n = (uint64_t)1 << log_n; p.l = (uint64_t)1 << log_l; p.c = (uint64_t)1 << p.log_c;
  p.msm = p.c > 1;
  p.ok = 1;
  if (!p.msm) return p;
  p.points = 2 * p.n;
  p.xy_bytes = (size_t)p.points * 96; p.inf_bytes = (size_t)p.points;
  p.point_bytes = (size_t)p.points * 144;
  p.gather_grid = p.permute_grid = kzg_grid(p.points);
  return p;
}

// cells: [evals only: copy + inverse transform]  ->  zero-extended copy  ->  fr_ntt_many (log_n + 1, count)  ->  the tiled map E -> cells
struct KzgCellsPlan {
  int ok = 0;
  int log_c = 0; uint64_t count = 0, n = 0;
  uint64_t scalars = 0;                // count * 2n
  size_t coeff_bytes = 0;              // evaluation form: count * n scalars
  size_t ext_bytes = 0;                // the zero-extended rows and their transform: count * 2n scalars
  unsigned copy_grid = 0, extend_grid = 0;
  KzgTranspose map;                    // count matrices of l rows x 2c columns (E[t 2c + i] -> cells[i][t]), source indices bit-reversed for ORDER_BITREV
};
inline KzgCellsPlan kzg_plan_cells(int log_n, int log_l, uint64_t count, int form, unsigned tile = KZG_TILE) {
  KzgCellsPlan p;
  KzgCellsArgs a;                                              // the ranges alone: count = 0 stops the check before the pointers
  a.log_n = log_n; a.log_l = log_l; a.form = form;
  if (kzg_check_cells(a) || !kzg_fits(count, log_n + 1, KZG_CELLS_MAX_LOG_TOTAL) || tile < 1 || tile > 32) return p;
  p.log_c = log_n - log_l; p.count = count; p.n = (uint64_t)1 << log_n;
  p.scalars = count << (log_n + 1);
  p.ok = 1;
  if (!count) return p;
  p.coeff_bytes = form == KZG_FORM_EVALS ? (size_t)(count << log_n) * 32 : 0;
  p.ext_bytes = (size_t)p.scalars * 32;
  p.copy_grid = form == KZG_FORM_EVALS ? kzg_grid(count << log_n) : 0;
  p.extend_grid = kzg_grid(p.scalars);
  p.map = kzg_transpose_plan(count, log_l, p.log_c + 1, tile);
  return p;
}

}  // namespace bls
