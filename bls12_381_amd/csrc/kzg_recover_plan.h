// kzg_recover_plan.h -- KZG cell recovery (blsgpu_kzg_recover[_device]: a polynomial rebuilt from any c of its 2c cells) as plain host
// code: the limits and every argument check, the index maps, the scratch layout and the launch shapes.  No HIP calls here: api_fr.hip
// launches from the plan, kzg_recover.hip.h reads the maps through the KZGR_HD functions below, tests/simt/emu_kzg_recover.cpp walks
// the same plan on the host and tests/cpp/kzg_recover_plan_main.cpp sweeps it under sanitizers.  The header compiles on its own.
//
// Notation (that of kzg_plan.h): n = 2^log_n, l = 2^log_l, c = n / l, w the root of order 2n, cell i < 2c the coset h_i <w^(2c)> with
// h_i = w^e_i, e_i = i (NATURAL) or bitrev(i, log_c + 1) (BITREV); g = 7, the reference's GENERATOR.  Entry t of cell i sits at natural
// index kzg_cell_src(i, t) of the size-2n transform, and that index is congruent to e_i mod 2c: e_i is the RESIDUE of the cell.
// With M the missing cells of one polynomial, |M| <= c, and a_i = h_i^l = (w^l)^e_i:
//   Zs(Y) = prod_{i in M} (Y - a_i)        Z(X) = Zs(X^l): zero exactly on the missing cosets, degree l |M| <= n
//   Zd[rho] = Zs((w^l)^rho)                Z(w^j)   = Zd[j mod 2c], 0 exactly at the missing residues
//   Zc[rho] = Zs(g^l (w^l)^rho)            Z(g w^j) = Zc[j mod 2c], never 0 (g^(2n) != 1)
//   EZ[j]   = the received value at w^j times Zd[j mod 2c], 0 elsewhere   = (P Z)(w^j) on the whole domain, deg(P Z) < 2n
// The stages of blsgpu_kzg_recover_device, in order (each a launch sequence that depends on (log_n, log_l, count, m) alone):
//   effective offsets -> slots -> roots (kept per (log_c, log_l)) -> vanish (Zd, Zc) -> ONE batch inversion of Zc -> scatter (EZ) -> inverse fr_ntt_many (log_n + 1)
//   -> forward fr_ntt_many on the coset g -> scale by Zc^-1 -> inverse fr_ntt_many on the coset g (2n coefficients Q) -> check (the OR of
//   Q[n..2n)) -> finish (ok, Q[0..n) or zeros) -> [out_cells: blsgpu_kzg_cells_device on the coefficients].
//
// The offsets the kernels walk are never the caller's: off(v) = eff[v], the running maximum of the caller's offsets clamped to m, with
// eff[0] = 0 and eff[count] = m (the rule of kzg_verify_plan.h).  A polynomial one of whose two ends differs from the caller's is BROKEN.
// Status word of polynomial v: 0 when it is recovered from its cells, else the OR of the KZGR_ST_* bits; every bit gives ok[v] = 0,
// zero rows and the context's sticky flag.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KZGR_HD __host__ __device__ inline
#else
#define KZGR_HD inline
#endif

// side of the square LDS tile of the scatter, in scalars (-D overrides; the host emulation also runs a tile of 4)
#ifndef KZGR_TILE
#define KZGR_TILE 16
#endif

namespace bls {

constexpr int KZGR_ORDER_NATURAL = 0, KZGR_ORDER_BITREV = 1;   // BLSGPU_FR_ORDER_*
constexpr int KZGR_MAX_LOG_N = 27;                             // the size-2n Fr transform (log <= 28)
constexpr int KZGR_MAX_LOG_L = 12;                             // as blsgpu_kzg_cells
constexpr int KZGR_MAX_LOG_CELLS = 12;                         // log_n - log_l + 1: 2c <= 4096, the tables are direct products, O(c^2) per polynomial
constexpr int KZGR_MAX_LOG_TOTAL = 28;                         // count * 2n
constexpr int KZGR_MAX_LOG_M = 24;                             // m
constexpr int KZGR_MAX_LOG_SCALARS = 28;                       // m * l
constexpr unsigned KZGR_BLOCK = 256;                           // lanes per workgroup of every kernel but the scatter
constexpr unsigned KZGR_ROOT_TILE = 64;                        // missing roots staged through LDS at a time by the vanish kernel (the host emulation also runs 3)
constexpr uint32_t KZGR_STATUS_BAD = (uint32_t)1 << 7;         // d_status bit 7: a malformed polynomial (device form)
constexpr uint32_t KZGR_ST_OFFSETS = 1, KZGR_ST_COL = 2, KZGR_ST_DUP = 4, KZGR_ST_FEW = 8;       // the status word of a polynomial
constexpr uint64_t KZGR_GEN_MONT[4] = {0x0000000efffffff1ull, 0x17e363d300189c0full, 0xff9c57876f8457b0ull, 0x351332208fc5a8c4ull};      // g = 7, Montgomery limbs

// ---- the maps, as the kernels read them --------------------------------------------------------------------------------------------
KZGR_HD uint64_t kzgr_bitrev(uint64_t i, int bits) {
  uint64_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}
// the residue of cell i: e_i with h_i = w^e_i, and every entry of the cell sits at a natural index congruent to it mod 2c
KZGR_HD uint64_t kzgr_residue(uint64_t i, int log_c, int order) { return order == KZGR_ORDER_BITREV ? kzgr_bitrev(i, log_c + 1) : i; }
// the cell whose residue is rho (the map above is an involution)
KZGR_HD uint64_t kzgr_cell_of_residue(uint64_t rho, int log_c, int order) { return kzgr_residue(rho, log_c, order); }
// natural index j < 2n of the size-2n transform -> (cell number, entry): the inverse of kzg_cell_src
KZGR_HD uint64_t kzgr_cell_of(uint64_t j, int log_c, int order) { return kzgr_cell_of_residue(j & (((uint64_t)2 << log_c) - 1), log_c, order); }
KZGR_HD uint64_t kzgr_entry_of(uint64_t j, int log_c, int log_l, int order) {
  const uint64_t row = j >> (log_c + 1);
  return order == KZGR_ORDER_BITREV ? kzgr_bitrev(row, log_l) : row;
}
// ... and kzg_cell_src itself: the natural index of entry t of cell i
KZGR_HD uint64_t kzgr_index_of(uint64_t i, uint64_t t, int log_c, int log_l, int order) {
  return ((order == KZGR_ORDER_BITREV ? kzgr_bitrev(t, log_l) : t) << (log_c + 1)) + kzgr_residue(i, log_c, order);
}

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal -------------------------------------------------
inline bool kzgr_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
// count * 2^log_unit <= 2^log_max without overflow
inline bool kzgr_fits(uint64_t count, int log_unit, int log_max) { return log_unit <= log_max && count <= ((uint64_t)1 << (log_max - log_unit)); }

inline const char* kzgr_check_shape(int log_n, int log_l) {
  if (log_n < 0 || log_n > KZGR_MAX_LOG_N) return "kzg_recover: log_n must be in [0, 27]";
  if (log_l < 0 || log_l > log_n || log_l > KZGR_MAX_LOG_L) return "kzg_recover: log_l must be in [0, min(log_n, 12)]";
  if (log_n - log_l + 1 > KZGR_MAX_LOG_CELLS) return "kzg_recover: 2c = 2^(log_n - log_l + 1) must not exceed 4096";
  return nullptr;
}
struct KzgrArgs {
  const void* col = nullptr; const void* offsets = nullptr; uint64_t count = 0, m = 0; const void* cells = nullptr;
  int log_n = 0, log_l = 0, order = 0;
  const void* polys = nullptr; const void* out_cells = nullptr; const void* ok = nullptr;
  bool device = false;
};
inline const char* kzgr_check(const KzgrArgs& a) {
  if (const char* why = kzgr_check_shape(a.log_n, a.log_l)) return why;
  if (a.order != KZGR_ORDER_NATURAL && a.order != KZGR_ORDER_BITREV) return "kzg_recover: unknown order";
  if (!kzgr_fits(a.count, a.log_n + 1, KZGR_MAX_LOG_TOTAL)) return "kzg_recover: count * 2n must not exceed 2^28";
  if (a.m > ((uint64_t)1 << KZGR_MAX_LOG_M)) return "kzg_recover: m must not exceed 2^24";
  if (!kzgr_fits(a.m, a.log_l, KZGR_MAX_LOG_SCALARS)) return "kzg_recover: m * l must not exceed 2^28";
  if (!a.count) return a.m ? "kzg_recover: cells but no polynomial" : nullptr;
  if (!a.offsets || !a.ok) return "kzg_recover: NULL offsets or ok with polynomials to recover";
  if (a.m && (!a.col || !a.cells)) return "kzg_recover: NULL col or cells with cells received";
  if (!a.polys && !a.out_cells) return "kzg_recover: both outputs are NULL (polys or out_cells must be given)";
  if (a.device) {
    if (((uintptr_t)a.cells | (uintptr_t)a.polys | (uintptr_t)a.out_cells) & 15) return "kzg_recover_device: scalar arrays must be 16-byte aligned";
    if (((uintptr_t)a.col | (uintptr_t)a.offsets) & 3) return "kzg_recover_device: col and offsets must be 4-byte aligned";
  }
  const uint64_t n = (uint64_t)1 << a.log_n;
  const struct { const void* p; uint64_t bytes; } in[3] = {{a.col, a.m * 4}, {a.offsets, (a.count + 1) * 4}, {a.cells, (a.m << a.log_l) * 32}};
  const struct { const void* p; uint64_t bytes; } out[3] = {{a.polys, a.count * n * 32}, {a.out_cells, a.count * n * 64}, {a.ok, a.count}};
  for (int o = 0; o < 3; o++) {
    for (int i = 0; i < 3; i++) if (kzgr_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return "kzg_recover: an output overlaps an input";
    for (int q = o + 1; q < 3; q++) if (kzgr_overlap(out[o].p, out[o].bytes, out[q].p, out[q].bytes)) return "kzg_recover: two outputs overlap";
  }
  return nullptr;
}
// what only the host form can see: the offsets as the interface states them, every cell number in range, no cell twice, c cells at least
inline const char* kzgr_check_host(const uint32_t* offsets, uint64_t count, const uint32_t* col, int log_n, int log_l) {
  if (!count) return nullptr;
  if (offsets[0] != 0) return "kzg_recover: offsets[0] must be 0";
  for (uint64_t v = 0; v < count; v++) if (offsets[v] > offsets[v + 1]) return "kzg_recover: offsets must be non-decreasing";
  const uint64_t cells = (uint64_t)2 << (log_n - log_l);
  for (uint64_t v = 0; v < count; v++) {
    uint64_t seen[(1 << KZGR_MAX_LOG_CELLS) / 64] = {};
    for (uint64_t k = offsets[v]; k < offsets[v + 1]; k++) {
      if (col[k] >= cells) return "kzg_recover: a cell number is not below 2c";
      if (seen[col[k] >> 6] >> (col[k] & 63) & 1) return "kzg_recover: a cell is listed twice for one polynomial";
      seen[col[k] >> 6] |= (uint64_t)1 << (col[k] & 63);
    }
    if ((uint64_t)(offsets[v + 1] - offsets[v]) * 2 < cells) return "kzg_recover: fewer than c cells for a polynomial";
  }
  return nullptr;
}
// the effective offsets of the header comment, as the kernel computes them (the host model of tests and emulation)
inline void kzgr_effective(const uint32_t* offsets, uint64_t count, uint32_t m, uint32_t* eff, uint8_t* mis) {
  uint32_t run = 0;
  for (uint64_t i = 0; i <= count; i++) {
    const uint32_t o = offsets[i], v = i == 0 ? 0u : i == count ? m : (o < m ? o : m);
    run = v > run ? v : run;
    eff[i] = run; mis[i] = o != run ? 1 : 0;
  }
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
inline unsigned kzgr_grid(uint64_t items) { return (unsigned)((items + KZGR_BLOCK - 1) / KZGR_BLOCK); }

struct KzgrPlan {
  int ok = 0;
  int log_n = 0, log_l = 0, log_c = 0;
  uint64_t count = 0, m = 0, n = 0, l = 0, cells = 0;      // cells: 2c
  uint64_t scalars = 0;                            // count * 2n: the working vector
  uint64_t tables = 0;                             // count * 2c: Zd, Zc, the slot table
  // launches
  unsigned offsets_grid = 0;                       // 1: the ONE workgroup that scans the offsets
  unsigned slots_grid = 0;                         // a workgroup per polynomial
  unsigned roots_grid = 0;                         // a lane per residue
  unsigned vanish_per_poly = 0, vanish_grid = 0;   // a lane per table entry, 4c per polynomial: workgroups per polynomial, and in all
  unsigned tile = 0, scatter_block = 0, scatter_grid = 0;      // the scatter: tile x tile lanes per tile of the l x 2c matrix of a polynomial
  uint64_t tiles_r = 0, tiles_c = 0;               // tiles along the entries / along the residues
  unsigned scale_grid = 0;                         // a lane per scalar of the working vector
  unsigned finish_per_poly = 0, finish_grid = 0;   // check and finish: a lane per coefficient of a half, workgroups per polynomial, and in all
  // scratch of the context: byte offsets into ONE block, each a multiple of 256
  size_t eff = 0;                                  // (count + 1) u32: the effective offsets
  size_t mis = 0;                                  // (count + 1) bytes: the caller's offset differs from the effective one
  size_t slot = 0;                                 // count * 2c i32: the index of the received cell, -1 for a missing one
  size_t status = 0;                               // count u32: the status word of every polynomial
  size_t upper = 0;                                // count u32: the OR of the words of Q[n..2n)
  size_t zd = 0, zc = 0;                           // count * 2c scalars each (zc: inverted in place)
  size_t work = 0;                                 // count * 2n scalars
  size_t coef = 0;                                 // count * n scalars: the coefficients when the caller takes only out_cells (else 0 bytes)
  size_t bytes = 0;
  // the root tables, kept by the context for the last (log_c, log_l): byte offsets into a block of their own, of the largest size
  size_t rootd = 0, rootc = 0;                     // 2c scalars each: (w^l)^rho and g^l (w^l)^rho
  size_t roots_bytes = 0;                          // 2 x 4096 scalars whatever the shape: the block never moves
};
// coef_scratch: the caller takes no polys, the coefficients go to scratch; tile: the scatter's, 0 for KZGR_TILE
inline KzgrPlan kzgr_plan(int log_n, int log_l, uint64_t count, uint64_t m, bool coef_scratch, unsigned tile = 0) {
  KzgrPlan p;
  if (!tile) tile = KZGR_TILE;
  if (kzgr_check_shape(log_n, log_l) || !kzgr_fits(count, log_n + 1, KZGR_MAX_LOG_TOTAL) || m > ((uint64_t)1 << KZGR_MAX_LOG_M) || !kzgr_fits(m, log_l, KZGR_MAX_LOG_SCALARS) ||
      (m && !count) || tile > 16) return p;
  p.log_n = log_n; p.log_l = log_l; p.log_c = log_n - log_l;
  p.count = count; p.m = m; p.n = (uint64_t)1 << log_n; p.l = (uint64_t)1 << log_l; p.cells = (uint64_t)2 << p.log_c;
  p.scalars = count << (log_n + 1); p.tables = count << (p.log_c + 1);
  p.ok = 1;
  if (!count) return p;
  p.offsets_grid = 1;
  p.slots_grid = (unsigned)count;
  p.roots_grid = kzgr_grid(p.cells);
  p.vanish_per_poly = kzgr_grid(2 * p.cells); p.vanish_grid = (unsigned)(count * p.vanish_per_poly);
  p.tile = tile; p.scatter_block = tile * tile;
  p.tiles_r = (p.l + tile - 1) / tile; p.tiles_c = (p.cells + tile - 1) / tile;
  p.scatter_grid = (unsigned)(count * p.tiles_r * p.tiles_c);
  p.scale_grid = kzgr_grid(p.scalars);
  p.finish_per_poly = kzgr_grid(p.n); p.finish_grid = (unsigned)(count * p.finish_per_poly);
  size_t o = 0;
  auto take = [&o](uint64_t bytes) { const size_t at = o; o += (size_t)((bytes + 255) / 256 * 256); return at; };
  p.eff = take((count + 1) * 4);
  p.mis = take(count + 1);
  p.slot = take(p.tables * 4);
  p.status = take(count * 4);
  p.upper = take(count * 4);
  p.zd = take(p.tables * 32);
  p.zc = take(p.tables * 32);
  p.work = take(p.scalars * 32);
  p.coef = take(coef_scratch ? (count << log_n) * 32 : 0);
  p.bytes = o;
  p.rootd = 0; p.rootc = (size_t)32 << KZGR_MAX_LOG_CELLS; p.roots_bytes = (size_t)64 << KZGR_MAX_LOG_CELLS;
  return p;
}

}  // namespace bls
