// fr_mle_plan.h -- the launch plans of the multilinear operations over Fr (blsgpu_fr_mle_fold*, blsgpu_fr_eq_table*, blsgpu_fr_mle_eval*,
// blsgpu_fr_sumcheck_round_device) as plain host code: which kernels of fr_mle.hip.h run, in which order, with which grid / block /
// dynamic LDS, on which buffers, and how large the scratch is.  No HIP calls here: api_fr.hip walks a plan and launches,
// tests/simt/emu_fr_mle.cpp walks the same plan on the host -- with a small shape, so that the multi-workgroup paths are reached at a few
// hundred elements.  The term program of a sumcheck is validated here as well (host data in, the kernels' FrmProg out).
//
// A table is 2^m scalars; table j of k starts j * pitch scalars after the base.  h = 2^(m-1).  Every step is a launch of its own on the
// stream (no workgroup waits for another one):
//
//   fold    FOLD                       one output i < h of one table per lane-step, grid-stride: out[i] = in[i] + r (in[i+h] - in[i])
//   eq      EQ                         one workgroup per tile of 2^lo outputs, lo = min(m, log2(block * chunk) rounded down)
//   eval    m == 0: COPY               out[j] = table j's only entry
//           FOLD (into SCRATCH, pitch 2^(m-1)), FOLD in place ..., the LAST fold writes `out` with pitch 1; fold s = 0 .. m-1 binds
//           x_(m-1-s) and reads its challenge from point[m-1-s] (step.var)
//   round   ROUND | ROUND_FUSED        one workgroup per tile of block * chunk positions, one RECORD of D + 1 scalars each;
//           FINISH                     one workgroup adds the records in a fixed order.  A single tile writes `evals` itself: no FINISH.
//           positions: i < h (plain) or i < q = 2^(m-2) (fused: the four quarter entries i, i + q, i + 2q, i + 3q)
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bls {

constexpr int FRM_BLOCK = 256;                    // lanes per workgroup (a multiple of 64: the sums use whole wavefronts)
constexpr int FRM_CHUNK = 4;                      // positions a lane of the round kernel takes, `block` apart (consecutive lanes on consecutive positions)
constexpr int FRM_MAX_M = 28;
constexpr int FRM_MAX_K = 8;                      // tables
constexpr int FRM_MAX_TERMS = 8;
constexpr int FRM_MAX_FACTORS = 6;                // factors of one term = the largest degree D
constexpr int FRM_MAX_EVALS = FRM_MAX_FACTORS + 1;
constexpr size_t FRM_MAX_TOTAL = (size_t)1 << 28;
constexpr unsigned FRM_FOLD_GRID_MAX = 1u << 14;  // workgroups of a fold: beyond that a lane takes several outputs

enum FrMleKernel { FRM_K_FOLD = 0, FRM_K_EQ = 1, FRM_K_ROUND = 2, FRM_K_ROUND_FUSED = 3, FRM_K_FINISH = 4, FRM_K_COPY = 5 };
enum FrMleBuf { FRM_BUF_NONE = -1, FRM_BUF_IN = 0, FRM_BUF_OUT = 1, FRM_BUF_SCRATCH = 2, FRM_BUF_REC = 3 };

struct FrMleShape { int block = FRM_BLOCK, chunk = FRM_CHUNK; };

// The term program as the kernels read it (a kernel argument, passed by value: it is a parameter, not data).
//   coef[t] = coef_t * 2^(5 n_t) mod r, canonical, n_t = the number of factors of term t: frl_mul divides by 2^261 and not by 2^256, the
//   n_t - 1 products between the factors and the one with the coefficient are n_t lazy products, each short by 2^5 (fr_mle.hip.h).
struct FrmProg {
  uint32_t n_terms, deg;                          // deg = D, the longest term
  uint32_t ptr[FRM_MAX_TERMS + 1];
  uint8_t tab[FRM_MAX_TERMS * FRM_MAX_FACTORS];
  uint32_t coef[FRM_MAX_TERMS][8];
};

// dynamic LDS of the round kernels: per lane 2 k packed values (f_j(t) and delta_j, eight words each, stored as two planes of 16-byte
// halves so that consecutive lanes sit on consecutive 16-byte words), then one scalar per wavefront and evaluation point for the sums.
// Sized from k: the shipped shape takes 64 KB + 896 bytes for k = 4 (two workgroups in a CU's 160 KB) and 128 KB + 896 bytes for k = 8.
constexpr size_t frm_sum_lds_words(FrMleShape s) { return (size_t)(s.block / 64) * FRM_MAX_EVALS * 8; }
constexpr size_t frm_round_lds_bytes(FrMleShape s, size_t k) { return ((size_t)s.block * 2 * k * 8 + frm_sum_lds_words(s)) * 4; }
static_assert(2 * frm_round_lds_bytes(FrMleShape(), 4) <= 160 * 1024, "two workgroups of the shipped shape with k <= 4 must fit a CU's LDS");
static_assert(frm_round_lds_bytes(FrMleShape(), FRM_MAX_K) <= 160 * 1024, "a workgroup of the shipped shape with k = 8 must fit a CU's LDS");
constexpr int frm_log2_floor(size_t v) { int l = 0; while (v >> (l + 1)) l++; return l; }
// eq: the low bits a workgroup builds in LDS (eight words per output)
constexpr int frm_eq_lo(int m, FrMleShape s) { return m < frm_log2_floor((size_t)s.block * s.chunk) ? m : frm_log2_floor((size_t)s.block * s.chunk); }
constexpr size_t frm_eq_lds_bytes(int lo) { return ((size_t)8 << lo) * 4; }

struct FrMleStep {
  int kernel;                  // FrMleKernel
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS
  size_t items;                // FOLD: outputs (k * h); EQ: outputs; ROUND*: positions per table; FINISH: records; COPY: tables
  int src, dst;                // FrMleBuf
  size_t pitch_in, pitch_out;  // FOLD / COPY: scalars between tables (0: the caller's pitch of that buffer)
  int m;                       // variables of the tables the step reads
  int var;                     // FOLD of an eval: index into `point` of its challenge; -1: the call's own challenge
};
struct FrMlePlan {
  int n_steps = 0;             // -1: refused
  FrMleStep step[FRM_MAX_M + 1];
  size_t tile = 0;             // positions (ROUND) / outputs (EQ) per workgroup
  size_t recs = 0;             // records of deg + 1 scalars FRM_BUF_REC must hold
  size_t scratch = 0;          // scalars FRM_BUF_SCRATCH must hold
};

inline unsigned frm_fold_grid(size_t items, FrMleShape s) {
  const size_t g = (items + s.block - 1) / s.block;
  return (unsigned)(g < FRM_FOLD_GRID_MAX ? g : FRM_FOLD_GRID_MAX);
}

// fold(f, r) of k tables of m >= 1 variables: IN -> OUT (which may be the same buffer)
inline FrMlePlan fr_mle_fold_plan(int m, size_t k, FrMleShape s = FrMleShape()) {
  FrMlePlan p;
  if (m < 1 || m > FRM_MAX_M) { p.n_steps = -1; return p; }
  if (!k) return p;
  const size_t items = k << (m - 1);
  p.step[p.n_steps++] = FrMleStep{FRM_K_FOLD, frm_fold_grid(items, s), (unsigned)s.block, 0, items, FRM_BUF_IN, FRM_BUF_OUT, 0, 0, m, -1};
  return p;
}

inline FrMlePlan fr_eq_table_plan(int m, FrMleShape s = FrMleShape()) {
  FrMlePlan p;
  if (m < 0 || m > FRM_MAX_M) { p.n_steps = -1; return p; }
  const int lo = frm_eq_lo(m, s);
  p.tile = (size_t)1 << lo;
  p.step[p.n_steps++] = FrMleStep{FRM_K_EQ, (unsigned)((size_t)1 << (m - lo)), (unsigned)s.block, frm_eq_lds_bytes(lo), (size_t)1 << m, FRM_BUF_NONE, FRM_BUF_OUT, 0, 0, m, -1};
  return p;
}

// f_j(point) for k tables: a chain of folds, the first one out of place into SCRATCH, the last one into OUT with pitch 1
inline FrMlePlan fr_mle_eval_plan(int m, size_t k, FrMleShape s = FrMleShape()) {
  FrMlePlan p;
  if (m < 0 || m > FRM_MAX_M) { p.n_steps = -1; return p; }
  if (!k) return p;
  if (m == 0) { p.step[p.n_steps++] = FrMleStep{FRM_K_COPY, 0, 0, 0, k, FRM_BUF_IN, FRM_BUF_OUT, 0, 1, 0, -1}; return p; }
  const size_t sp = (size_t)1 << (m - 1);           // pitch of the scratch copy
  if (m > 1) p.scratch = k * sp;
  for (int f = 0; f < m; f++) {
    const int mm = m - f;                           // variables before this fold
    const size_t items = k << (mm - 1);
    const bool first = f == 0, last = f == m - 1;
    p.step[p.n_steps++] = FrMleStep{FRM_K_FOLD, frm_fold_grid(items, s), (unsigned)s.block, 0, items, first ? FRM_BUF_IN : FRM_BUF_SCRATCH, last ? FRM_BUF_OUT : FRM_BUF_SCRATCH,
                                    first ? 0 : sp, last ? 1 : sp, mm, m - 1 - f};
  }
  return p;
}

// one round polynomial of k tables of m variables (fused: the tables are folded first and then have m - 1)
inline FrMlePlan fr_sumcheck_round_plan(int m, size_t k, int deg, bool fused, FrMleShape s = FrMleShape()) {
  FrMlePlan p;
  if (m < (fused ? 2 : 1) || m > FRM_MAX_M || !k || k > FRM_MAX_K || deg < 1 || deg > FRM_MAX_FACTORS) { p.n_steps = -1; return p; }
  const size_t npos = (size_t)1 << (m - (fused ? 2 : 1));
  p.tile = (size_t)s.block * s.chunk;
  const size_t tiles = (npos + p.tile - 1) / p.tile;
  const bool one = tiles == 1;
  if (!one) p.recs = tiles;
  p.step[p.n_steps++] = FrMleStep{fused ? FRM_K_ROUND_FUSED : FRM_K_ROUND, (unsigned)tiles, (unsigned)s.block, frm_round_lds_bytes(s, k), npos, FRM_BUF_IN,
                                  one ? FRM_BUF_OUT : FRM_BUF_REC, 0, 0, m, -1};
  if (!one) p.step[p.n_steps++] = FrMleStep{FRM_K_FINISH, 1, (unsigned)s.block, frm_sum_lds_words(s) * 4, tiles, FRM_BUF_REC, FRM_BUF_OUT, 0, 0, m, -1};
  return p;
}

// ---- the term program ----------------------------------------------------------------------------------------------------------------
// r as four 64-bit words and 2^k x mod r on canonical words: the 2^5 bookkeeping of the coefficients is host work, done once per program
constexpr uint64_t FRM_R64[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
inline bool frm_below_r(const uint64_t* a) {
  for (int i = 3; i >= 0; i--) { if (a[i] < FRM_R64[i]) return true; if (a[i] > FRM_R64[i]) return false; }
  return false;
}
inline void frm_double_mod_r(uint64_t* a) {         // a < r < 2^255: 2a fits four words
  uint64_t c = 0;
  for (int i = 0; i < 4; i++) { const uint64_t v = a[i]; a[i] = (v << 1) | c; c = v >> 63; }
  if (!frm_below_r(a)) {
    uint64_t b = 0;
    for (int i = 0; i < 4; i++) { const uint64_t v = a[i], s = v - FRM_R64[i] - b; b = (v < FRM_R64[i] || (v == FRM_R64[i] && b)) ? 1 : 0; a[i] = s; }
  }
}

// Checks a term program against the rules of include/bls12_381_hip.h and builds the kernels' form.  Returns NULL when it is valid, or the
// text that names what is wrong.
inline const char* frm_prog_build(size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef, FrmProg* out) {
  if (!k || k > (size_t)FRM_MAX_K) return "fr_sumcheck: k must be in [1, 8]";
  if (!n_terms || n_terms > (size_t)FRM_MAX_TERMS) return "fr_sumcheck: n_terms must be in [1, 8]";
  if (!term_ptr || !term_tab || !coef) return "fr_sumcheck: NULL term_ptr / term_tab / coef";
  if (term_ptr[0] != 0) return "fr_sumcheck: term_ptr[0] must be 0";
  FrmProg p;
  p.n_terms = (uint32_t)n_terms; p.deg = 0;
  for (int i = 0; i <= FRM_MAX_TERMS; i++) p.ptr[i] = 0;
  for (int i = 0; i < FRM_MAX_TERMS * FRM_MAX_FACTORS; i++) p.tab[i] = 0;
  for (int t = 0; t < FRM_MAX_TERMS; t++) for (int w = 0; w < 8; w++) p.coef[t][w] = 0;
  for (size_t t = 0; t < n_terms; t++) {
    if (term_ptr[t + 1] <= term_ptr[t] || term_ptr[t + 1] - term_ptr[t] > (uint32_t)FRM_MAX_FACTORS) return "fr_sumcheck: term_ptr must increase strictly, by 1 to 6 factors per term";
    const uint32_t n = term_ptr[t + 1] - term_ptr[t];
    if (n > p.deg) p.deg = n;
    p.ptr[t + 1] = term_ptr[t + 1];
    for (uint32_t e = term_ptr[t]; e < term_ptr[t + 1]; e++) {
      if (term_tab[e] >= k) return "fr_sumcheck: a term_tab entry is not below k";
      p.tab[e] = term_tab[e];
    }
    uint64_t c[4] = {coef[4 * t], coef[4 * t + 1], coef[4 * t + 2], coef[4 * t + 3]};
    if (!frm_below_r(c)) return "fr_sumcheck: a coefficient is not a canonical Scalar (limbs >= r)";
    for (uint32_t d = 0; d < 5 * n; d++) frm_double_mod_r(c);
    for (int w = 0; w < 4; w++) { p.coef[t][2 * w] = (uint32_t)c[w]; p.coef[t][2 * w + 1] = (uint32_t)(c[w] >> 32); }
  }
  *out = p;
  return nullptr;
}

}  // namespace bls
