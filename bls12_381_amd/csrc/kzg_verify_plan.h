// kzg_verify_plan.h -- batched KZG cell-proof verification (blsgpu_kzg_cell_verifier_*, blsgpu_kzg_verify_cells[_device]) as plain host
// code: the limits and every argument check, the exponent maps, the cut of the cell list into the chunks of the fold, the scratch
// layout and the launch shapes.  No HIP calls here: api_msm.hip launches from the plan, kzg_verify.hip.h reads the maps through the
// KZGV_HD functions below, tests/simt/emu_kzg_verify.cpp walks the same plan on the host and tests/cpp/kzg_verify_plan_main.cpp sweeps
// it under sanitizers.  The header compiles on its own.
//
// Notation (that of kzg_plan.h): n = 2^log_n, l = 2^log_l, c = n / l, w the root of order 2n, cell j < 2c the coset h_j <w^(2c)>.  With
// m cells in nseg batches, batch s owning the cells [off(s), off(s + 1)), rho_k = r_s^(k - off(s)), a_k = h_col[k]^l and I_k the
// polynomial of degree < l through cell k:
//   A_s = sum_k rho_k proof_k      B_s = sum_k rho_k commit[row_k] + sum_k rho_k a_k proof_k - sum_u agg[s][u] S[u]
//   agg[s][u] = sum_k rho_k I_k[u],   I_k[u] = h^(-u) INTT_l(v_k)[u],   v_k the cell in natural coset order
// Every power of w is a product of entries of ONE table of log_n + 1 scalars, winv^(2^b): h^(-u) = winv^(e u mod 2n) and
// a = w^(e l) = winv^(2n - e l mod 2n), e = kzgv_shift_exponent(col).
//
// The offsets the kernels walk are never the caller's: off(s) = eff[s], the running maximum of the caller's offsets clamped to m, with
// eff[0] = 0 and eff[nseg] = m.  It is a valid CSR array whatever the caller wrote, and equals the caller's wherever that one is valid;
// a batch one of whose two ends differs from the caller's is BROKEN (verdict 0, an identity pair), every other batch owns exactly the
// cells its caller meant.
//
// The fold.  The m cells form ONE list, cut into chunks of `chunk` cells whatever the batches are (the shape of gsum_plan.h).  Pass 1,
// lane (chunk q, column u), walks the chunk's cells in order and closes a batch where it ends: a batch inside the chunk is final, of a
// batch that crosses the chunk's border the chunk keeps a partial in record 2 q (HEAD: the batch holds the chunk's first cell) or
// 2 q + 1 (TAIL).  Pass 2, lane (batch s, column u), adds the partials of a batch that spans several chunks and writes 0 for an empty
// one.  Field sums are exact, so the limbs do not depend on the order.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KZGV_HD __host__ __device__ inline
#else
#define KZGV_HD inline
#endif

namespace bls {

constexpr int KZGV_ORDER_NATURAL = 0, KZGV_ORDER_BITREV = 1;   // BLSGPU_FR_ORDER_*
constexpr int KZGV_MAX_LOG_N = 23;                             // the shapes of blsgpu_kzg_multiproof_create
constexpr int KZGV_MAX_LOG_L = 12;                             // l <= BLSGPU_SEG_LEN_MAX: a segment of the MSM over S[0..l)
constexpr int KZGV_MAX_LOG_CELLS = 24;                         // m
constexpr int KZGV_MAX_LOG_SEGS = 24;                          // nseg
constexpr int KZGV_MAX_LOG_SCALARS = 27;                       // m * l and nseg * l (the total of msm_segments)
constexpr unsigned KZGV_BLOCK = 256;                           // lanes per workgroup of every kernel (one item per lane; the ONE workgroup that scans the offsets)
constexpr uint32_t KZGV_CHUNK_MAX = 256;                       // cells per chunk of the fold, a power of two
constexpr uint64_t KZGV_FOLD_LANES = (uint64_t)1 << 16;        // the fold's chunks are cut so that about this many lanes run
constexpr uint32_t KZGV_STATUS_BAD = (uint32_t)1 << 6;         // d_status bit 6 (the five below it are other calls'): a row / col out of range or a broken batch (device form)

// ---- the maps, as the kernels read them --------------------------------------------------------------------------------------------
KZGV_HD uint64_t kzgv_bitrev(uint64_t i, int bits) {
  uint64_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}
// e with h_col = w^e
KZGV_HD uint64_t kzgv_shift_exponent(uint64_t col, int log_n, int log_l, int order) { return order == KZGV_ORDER_BITREV ? kzgv_bitrev(col, log_n + 1 - log_l) : col; }
// the exponent of winv = w^-1 that gives h^(-u): e u mod 2n
KZGV_HD uint64_t kzgv_inv_power_exponent(uint64_t e, uint64_t u, int log_n) { return (e * u) & (((uint64_t)2 << log_n) - 1); }
// the exponent of winv that gives a = h^l = w^(e l): (2n - e l mod 2n) mod 2n
KZGV_HD uint64_t kzgv_a_exponent(uint64_t e, int log_n, int log_l) {
  const uint64_t mask = ((uint64_t)2 << log_n) - 1;
  return (((uint64_t)2 << log_n) - ((e << log_l) & mask)) & mask;
}
// the batch of cell k < m over the effective offsets: the LAST s < nseg with eff[s] <= k (the empty batches that begin where k's does come before it)
KZGV_HD uint32_t kzgv_seg_of(const uint32_t* eff, uint32_t nseg, uint32_t k) {
  uint32_t lo = 0, hi = nseg;                                  // eff[lo] <= k < eff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (eff[mid] <= k) lo = mid; else hi = mid;
  }
  return lo;
}
// a batch [so, se) that the chunk beginning at cb holds whole: final in pass 1
KZGV_HD bool kzgv_inside(uint32_t so, uint32_t se, uint32_t cb, uint32_t chunk) { return so >= cb && se - cb <= chunk; }
// where chunk q keeps its partial of a batch [so, ..) it does not hold whole: record 2 q (HEAD) or 2 q + 1 (TAIL)
KZGV_HD size_t kzgv_record(size_t q, uint32_t so, uint32_t cb) { return 2 * q + (so <= cb ? 0 : 1); }

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal -------------------------------------------------
inline bool kzgv_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
// count * 2^log_unit <= 2^log_max without overflow
inline bool kzgv_fits(uint64_t count, int log_unit, int log_max) { return log_unit <= log_max && count <= ((uint64_t)1 << (log_max - log_unit)); }

struct KzgvCreateArgs {
  bool srs_given = false; int srs_group = 0; uint64_t srs_len = 0; int srs_subgroup = 0;
  int log_n = 0, log_l = 0; bool q_given = false, out_given = false;
};
inline const char* kzgv_check_shape(int log_n, int log_l) {
  if (log_n < 0 || log_n > KZGV_MAX_LOG_N) return "kzg_cell_verifier: log_n must be in [0, 23]";
  if (log_l < 0 || log_l > log_n || log_l > KZGV_MAX_LOG_L) return "kzg_cell_verifier: log_l must be in [0, min(log_n, 12)]";
  return nullptr;
}
inline const char* kzgv_check_create(const KzgvCreateArgs& a) {
  if (!a.srs_given || !a.q_given || !a.out_given) return "kzg_cell_verifier_create: NULL argument";
  if (const char* why = kzgv_check_shape(a.log_n, a.log_l)) return why;
  if (a.srs_group != 1) return "kzg_cell_verifier_create: the SRS must be a G1 base set";
  if (a.srs_len < ((uint64_t)1 << a.log_l)) return "kzg_cell_verifier_create: the SRS holds fewer than 2^log_l points";
  if (a.srs_subgroup == 0) return "kzg_cell_verifier_create: the SRS holds a point outside the prime-order subgroup";
  return nullptr;
}

struct KzgvArgs {
  bool handle_given = false; int log_n = 0, log_l = 0;
  const void* commit_xy = nullptr; const void* commit_inf = nullptr; uint64_t ncommit = 0;
  const void* row = nullptr; const void* col = nullptr; const void* cells = nullptr;
  const void* proof_xy = nullptr; const void* proof_inf = nullptr;
  const void* offsets = nullptr; uint64_t nseg = 0, m = 0;
  const void* r = nullptr; int order = 0;
  const void* verdict = nullptr; const void* out_ab = nullptr;
  bool device = false;
};
inline const char* kzgv_check(const KzgvArgs& a) {
  if (!a.handle_given) return "kzg_verify_cells: NULL handle";
  if (const char* why = kzgv_check_shape(a.log_n, a.log_l)) return why;
  if (a.order != KZGV_ORDER_NATURAL && a.order != KZGV_ORDER_BITREV) return "kzg_verify_cells: unknown order";
  if (a.m > ((uint64_t)1 << KZGV_MAX_LOG_CELLS)) return "kzg_verify_cells: m must not exceed 2^24";
  if (a.nseg > ((uint64_t)1 << KZGV_MAX_LOG_SEGS)) return "kzg_verify_cells: nseg must not exceed 2^24";
  if (a.ncommit >= ((uint64_t)1 << 32)) return "kzg_verify_cells: ncommit must be below 2^32";
  if (!kzgv_fits(a.m, a.log_l, KZGV_MAX_LOG_SCALARS)) return "kzg_verify_cells: m * l must not exceed 2^27";
  if (!kzgv_fits(a.nseg, a.log_l, KZGV_MAX_LOG_SCALARS)) return "kzg_verify_cells: nseg * l must not exceed 2^27";
  if (!a.nseg) return a.m ? "kzg_verify_cells: cells but no batch" : nullptr;
  if (!a.offsets || !a.r || !a.verdict) return "kzg_verify_cells: NULL offsets, challenges or verdicts with batches to check";
  if (a.m && (!a.row || !a.col || !a.cells || !a.proof_xy || !a.proof_inf)) return "kzg_verify_cells: NULL argument with cells to check";
  if (a.m && a.ncommit && (!a.commit_xy || !a.commit_inf)) return "kzg_verify_cells: NULL commitments with cells to check";
  if (a.device) {
    if (((uintptr_t)a.cells | (uintptr_t)a.r) & 15) return "kzg_verify_cells_device: scalar arrays must be 16-byte aligned";
    if (((uintptr_t)a.commit_xy | (uintptr_t)a.proof_xy | (uintptr_t)a.out_ab) & 7) return "kzg_verify_cells_device: point arrays must be 8-byte aligned";
    if (((uintptr_t)a.row | (uintptr_t)a.col | (uintptr_t)a.offsets) & 3) return "kzg_verify_cells_device: row, col and offsets must be 4-byte aligned";
  }
  const uint64_t l = (uint64_t)1 << a.log_l;
  const struct { const void* p; uint64_t bytes; } in[9] = {{a.commit_xy, a.ncommit * 96}, {a.commit_inf, a.ncommit}, {a.row, a.m * 4}, {a.col, a.m * 4}, {a.cells, a.m * l * 32},
                                                           {a.proof_xy, a.m * 96}, {a.proof_inf, a.m}, {a.offsets, (a.nseg + 1) * 4}, {a.r, a.nseg * 32}};
  for (int i = 0; i < 9; i++) {
    if (kzgv_overlap(a.verdict, a.nseg, in[i].p, in[i].bytes)) return "kzg_verify_cells: the verdicts overlap an input";
    if (kzgv_overlap(a.out_ab, a.nseg * 288, in[i].p, in[i].bytes)) return "kzg_verify_cells: out_ab overlaps an input";
  }
  if (kzgv_overlap(a.verdict, a.nseg, a.out_ab, a.nseg * 288)) return "kzg_verify_cells: the two outputs overlap";
  return nullptr;
}
// what only the host form can see: the offsets as the interface states them, every index in range
inline const char* kzgv_check_host(const uint32_t* offsets, uint64_t nseg, uint64_t m, const uint32_t* row, const uint32_t* col, uint64_t ncommit, int log_n, int log_l) {
  if (!nseg) return nullptr;
  if (offsets[0] != 0) return "kzg_verify_cells: offsets[0] must be 0";
  for (uint64_t s = 0; s < nseg; s++) if (offsets[s] > offsets[s + 1]) return "kzg_verify_cells: offsets must be non-decreasing";
  if (offsets[nseg] != m) return "kzg_verify_cells: m must be offsets[nseg]";
  const uint64_t cells = (uint64_t)2 << (log_n - log_l);
  for (uint64_t k = 0; k < m; k++) {
    if (row[k] >= ncommit) return "kzg_verify_cells: a row index is outside the commitments";
    if (col[k] >= cells) return "kzg_verify_cells: a cell number is not below 2c";
  }
  return nullptr;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
inline unsigned kzgv_grid(uint64_t items) { return (unsigned)((items + KZGV_BLOCK - 1) / KZGV_BLOCK); }
// cells per chunk of the fold: the largest power of two <= KZGV_CHUNK_MAX that still leaves about KZGV_FOLD_LANES lanes
inline uint32_t kzgv_chunk(uint64_t m, int log_l) {
  uint32_t chunk = 1;
  while (chunk < KZGV_CHUNK_MAX && ((m << log_l) / (2 * chunk)) >= KZGV_FOLD_LANES) chunk *= 2;
  return chunk;
}

struct KzgvPlan {
  int ok = 0;
  int log_n = 0, log_l = 0, log_c = 0;
  uint64_t m = 0, nseg = 0, l = 0, cells = 0;      // cells: 2c
  uint32_t chunk = 0; uint64_t nchunks = 0;        // the fold's cut
  uint64_t products = 0;                           // 3 m: the (point, scalar) pairs of ONE mul_batch, thirds (proof, rho), (proof, rho a), (commit[row], rho)
  uint64_t sums = 0;                               // 3 nseg: the segment sums of the thirds
  uint64_t terms = 0;                              // 2 nseg: the pairing terms (A_s, q), (B_s, -G2)
  // launches
  unsigned scan_grid = 0;                          // 1 (0: no launch): the ONE workgroup that scans the offsets
  unsigned weights_grid = 0;                       // a lane per cell
  unsigned copy_grid = 0;                          // a lane per scalar of the cells
  unsigned fold_grid = 0;                          // a lane per (chunk, column)
  unsigned combine_grid = 0;                       // a lane per (batch, column)
  unsigned finish_grid = 0;                        // a lane per batch
  // scratch of the context: byte offsets into ONE block, each a multiple of 256
  size_t eff = 0;                                  // (nseg + 1) u32: the effective offsets
  size_t mis = 0;                                  // (nseg + 1) bytes: the caller's offset differs from the effective one
  size_t badidx = 0;                               // nseg bytes: a row / col of the batch was out of range
  size_t bad = 0;                                  // nseg bytes: the batch's verdict is 0 whatever the pairing says
  size_t isone = 0;                                // nseg bytes: gt_is_identity
  size_t off64 = 0;                                // (3 nseg + 1) u64: the offsets of the segment sums over the thirds
  size_t msm_off = 0, base_first = 0;              // (nseg + 1) u32: s l;  nseg u32: 0
  size_t scal = 0;                                 // 3 m scalars
  size_t pxy = 0, pinf = 0;                        // 3 m affine wire points + flags: the gathered points, then the normalised products
  size_t prod = 0;                                 // 3 m projective wire points
  size_t sum = 0;                                  // 3 nseg projective wire points
  size_t cellc = 0;                                // m l scalars: the cells in natural coset order, then their inverse transforms
  size_t part = 0;                                 // 2 nchunks records of l scalars
  size_t agg = 0;                                  // nseg l scalars
  size_t msm = 0;                                  // nseg projective wire points
  size_t ab = 0;                                   // 2 nseg projective wire points: A_s, B_s
  size_t abxy = 0, abinf = 0;                      // 2 nseg affine wire points + flags
  size_t qidx = 0, poff = 0;                       // 2 nseg u32;  (nseg + 1) u64
  size_t gt = 0;                                   // nseg x 576 bytes
  size_t bytes = 0;
};
// chunk: the cells per chunk of the fold, 0 for the automatic cut (the host emulation also runs chunks of a few cells)
inline KzgvPlan kzgv_plan(int log_n, int log_l, uint64_t m, uint64_t nseg, uint32_t chunk = 0) {
  KzgvPlan p;
  if (kzgv_check_shape(log_n, log_l) || m > ((uint64_t)1 << KZGV_MAX_LOG_CELLS) || nseg > ((uint64_t)1 << KZGV_MAX_LOG_SEGS)) return p;
  if (!kzgv_fits(m, log_l, KZGV_MAX_LOG_SCALARS) || !kzgv_fits(nseg, log_l, KZGV_MAX_LOG_SCALARS) || (m && !nseg) || chunk > KZGV_CHUNK_MAX) return p;
  p.log_n = log_n; p.log_l = log_l; p.log_c = log_n - log_l;
  p.m = m; p.nseg = nseg; p.l = (uint64_t)1 << log_l; p.cells = (uint64_t)2 << p.log_c;
  p.ok = 1;
  if (!nseg) return p;
  p.chunk = chunk ? chunk : kzgv_chunk(m, log_l);
  p.nchunks = (m + p.chunk - 1) / p.chunk;
  p.products = 3 * m; p.sums = 3 * nseg; p.terms = 2 * nseg;
  p.scan_grid = 1;
  p.weights_grid = kzgv_grid(m);
  p.copy_grid = kzgv_grid(m << log_l);
  p.fold_grid = kzgv_grid(p.nchunks << log_l);
  p.combine_grid = kzgv_grid(nseg << log_l);
  p.finish_grid = kzgv_grid(nseg);
  size_t o = 0;
  auto take = [&o](uint64_t bytes) { const size_t at = o; o += (size_t)((bytes + 255) / 256 * 256); return at; };
  p.eff = take((nseg + 1) * 4);
  p.mis = take(nseg + 1);
  p.badidx = take(nseg);
  p.bad = take(nseg);
  p.isone = take(nseg);
  p.off64 = take((3 * nseg + 1) * 8);
  p.msm_off = take((nseg + 1) * 4);
  p.base_first = take(nseg * 4);
  p.scal = take(p.products * 32);
  p.pxy = take(p.products * 96);
  p.pinf = take(p.products);
  p.prod = take(p.products * 144);
  p.sum = take(p.sums * 144);
  p.cellc = take((m << log_l) * 32);
  p.part = take((2 * p.nchunks << log_l) * 32);
  p.agg = take((nseg << log_l) * 32);
  p.msm = take(nseg * 144);
  p.ab = take(p.terms * 144);
  p.abxy = take(p.terms * 96);
  p.abinf = take(p.terms);
  p.qidx = take(p.terms * 4);
  p.poff = take((nseg + 1) * 8);
  p.gt = take(nseg * 576);
  p.bytes = o;
  return p;
}

}  // namespace bls
