// fr_mle.hip.h -- multilinear polynomials over Fr as tables of 2^m values on the hypercube: binding the top variable (blsgpu_fr_mle_fold*),
// the table of eq(p, .) (blsgpu_fr_eq_table*), evaluation at a point (blsgpu_fr_mle_eval*: a chain of folds, no kernel of its own) and the
// round polynomial of a sumcheck over a sum of products of tables (blsgpu_fr_sumcheck_round_device, the blsgpu_fr_sumcheck handle).
// fr_mle_plan.h decides the launches, sizes the LDS and the records and validates the term program.
//
// Conventions (include/bls12_381_hip.h).  Entry i of a table is the value at the point whose coordinate x_b is bit b of i; h = 2^(m-1);
// a fold binds the TOP variable: fold(f, r)[i] = f[i] + r (f[i+h] - f[i]).  The round polynomial of P = sum_t coef_t prod_e f_tab[e] is
//     evals[t] = sum_{i<h} sum_t' coef_t' prod_e ((1 - t) f_e[i] + t f_e[i+h]),   t = 0 .. D,  D = the longest term.
//
// The schedule of a round.  The h positions are cut into tiles of blockDim.x lanes x `chunk` positions (consecutive lanes on consecutive
// positions: every table is read in 32-byte pieces next to each other).  For a position the lane loads the pair (f_j[i], f_j[i+h]) of
// every table -- fused: the four quarter entries i, i + q, i + 2q, i + 3q (q = h / 2), folds (i, i + 2q) and (i + q, i + 3q) at the
// previous challenge and writes both results back canonical at i and i + q: the table of the next round, in place, pitch kept -- and
// keeps f_j(0) and delta_j = f_j[i+h] - f_j[i] in ITS slots of LDS: the term program is indexed at run time, and a register array
// indexed by term_tab[e] would live in scratch memory, while in LDS the index is an address.  No lane touches another lane's slots, so
// the hot loop has no barrier.  Then t walks 0 .. D: every term multiplies its factors and its coefficient, the products add into the
// lane's accumulator of t, and every table steps on, f_j(t + 1) = f_j(t) + delta_j.  At the end the lanes' D + 1 sums go through the
// wavefront shuffles (frs_shfl) and LDS and become ONE record of D + 1 scalars per workgroup; k_frm_round_finish adds the records in a
// fixed order.  No atomics, no workgroup waits for another one: the same sums in the same order from run to run.
//
// Arithmetic: the lazy 9 x 29-bit limbs of fr.hip.h, bounds in that file's notation ("A": limbs < A 2^29, "V": value < V r).  frl_mul
// divides by 2^261, not by 2^256, so every lazy product is short by 2^5 against the reference's Montgomery product; the factor is folded
// into the constant operand each time:
//   fold      r' = 2^5 r mod r (five doublings, once per lane and launch)                                                 canonical
//             d = hi + 4r - lo                                              (canonical lo, hi)                            A3 V5
//             frl_mul(d, r') = r (hi - lo) / 2^256                          (A3 x A1 <= 6, V5 x V1 <= 70)                 A1 V2
//             lo + that                                                                                                   A2 V3
//             -> frl_reduce (needs A <= 4, V <= 8)                                                                        A1 V2  -> frl_canon to store
//   round     f(0) = lo (canonical, or a fold's A1 V2), delta = hi + 4r - lo                                              A3 V6
//             -> frl_reduce                                                                                               A1 V2  (what LDS holds: packed, < 2r < 2^256)
//             f(t + 1) = f(t) + delta                                                                                     A2 V4  -> frl_reduce -> A1 V2
//             a term of n factors: n - 1 products of A1 V2 values (A1 x A1, V2 x V2 = 4 <= 70), each A1 V2, in all short by 2^(5 (n - 1));
//             one more product with coef' = 2^(5 n) coef (canonical, folded on the host when the program is validated)     A1 V2  = coef prod f / 2^(256 n)
//             the sum over the terms of one position takes FRM_LAZY products between reductions                        <= A3 V6
//             accumulator (A1 V2) + that                                                                               <= A4 V8 -> frl_reduce -> A1 V2
// Where the coefficient goes.  Accumulators per (t, term) with the coefficients applied by the finish kernel would take the coefficient
// product out of the hot loop, but they are up to 7 x 8 accumulators of nine registers each; the kernel keeps ONE accumulator per t (63
// registers) and pays one product per term, position and t.
// Sums ACROSS lanes and workgroups are canonical fr_add (scalar.hip.h).
#pragma once
#include "fr.hip.h"
#include "fr_scan.hip.h"
#include "fr_mle_plan.h"

namespace bls {

constexpr int FRM_LAZY = 3;                          // products added to a term sum before the next frl_reduce
static_assert(1 + FRM_LAZY <= 4 && 2 + 2 * FRM_LAZY <= 8, "a reduced term sum (A1 V2) + FRM_LAZY products (A1 V2 each) must stay within frl_reduce's A <= 4, V <= 8");
static_assert(1 + FRM_LAZY <= 4 && 2 + 2 * FRM_LAZY <= 8, "accumulator (A1 V2) + a term sum that left the loop (reduced + FRM_LAZY - 1 products at most: A3 V6) likewise");
static_assert(3 * 1 <= 6 && 5 * 1 <= 70, "the fold's product: d (A3 V5) x r' (A1 V1) within frl_mul's column bound A <= 6 and value bound V <= 70");
static_assert(1 * 1 <= 6 && 2 * 2 <= 70, "a term's products: A1 V2 x A1 V2 within frl_mul's bounds");
static_assert(FRM_BLOCK % 64 == 0, "the sums work on whole wavefronts");
static_assert(FRM_MAX_EVALS == 7, "k_frm_round keeps one accumulator per evaluation point in registers");

DEV FrL frm_zero() { FrL r; for (int i = 0; i < 9; i++) r.l[i] = 0; return r; }
// 2^5 r for the challenge at p (canonical in, canonical out), as lazy limbs
DEV FrL frm_challenge(const u32* p) {
  Fr v = fr_load(p);
  for (int s = 0; s < 5; s++) v = fr_add(v, v);
  return frl_unpack(v);
}
// lo + r (hi - lo) for canonical lo, hi and r5 = 2^5 r: A1 V2
DEV FrL frm_fold(const FrL& lo, const FrL& hi, const FrL& r5) {
  return frl_reduce(frl_add(lo, frl_mul(frl_sub<1>(hi, lo), r5)));
}

// ---- fold ---------------------------------------------------------------------------------------------------------------------------
// out[j][i] = in[j][i] + r (in[j][i + h] - in[j][i]) for i < h = 2^log_h and every table j: `items` = k h outputs, one per lane-step.
// out == in with equal pitches is the in-place form: a lane reads i and i + h and writes i, which no other lane reads.
__global__ void __launch_bounds__(FRM_BLOCK) k_frm_fold(const u32* in, size_t pitch_in, u32* out, size_t pitch_out, int log_h, size_t items, const u32* __restrict__ r) {
  const FrL r5 = frm_challenge(r);
  const size_t h = (size_t)1 << log_h;
#pragma unroll 1
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < items; g += (size_t)gridDim.x * blockDim.x) {
    const size_t j = g >> log_h, i = g & (h - 1);
    const u32* src = in + (j * pitch_in + i) * 8;
    const FrL lo = frl_load(src), hi = frl_load(src + h * 8);
    fr_store(out + (j * pitch_out + i) * 8, frl_canon(frm_fold(lo, hi, r5)));
  }
}

// ---- eq -----------------------------------------------------------------------------------------------------------------------------
// out[i] = prod_{b<m} (bit b of i ? p_b : 1 - p_b).  Workgroup w owns the 2^lo outputs whose high bits are w.  It starts from
// T[0] = the product over the HIGH bits (the lanes of the first wavefront hold one factor each and multiply across the wavefront) and
// doubles the table in LDS once per low bit b: T[i + 2^b] = T[i] p_b, T[i] = T[i] - T[i + 2^b] -- one product per output.  Canonical
// arithmetic (scalar.hip.h) throughout: the table is built once per sumcheck, not once per round.
__global__ void __launch_bounds__(FRM_BLOCK) k_frm_eq(const u32* __restrict__ point, int m, int lo, u32* __restrict__ out) {
  BLS_DYN_LDS(lds);
  if (threadIdx.x < 64) {
    const int b = lo + (int)threadIdx.x;
    Fr f = fr_one();
    if (b < m) {
      f = fr_load(point + (size_t)b * 8);
      if (!((blockIdx.x >> threadIdx.x) & 1u)) f = fr_sub(fr_one(), f);
    }
#pragma unroll 1
    for (unsigned d = 32; d; d >>= 1) f = frs_mul(f, frs_shfl(f, d, true));      // lane 0 ends with the product of all 64 (m - lo <= 28 of them are not one)
    if (threadIdx.x == 0) fr_store(lds, f);
  }
  __syncthreads();
#pragma unroll 1
  for (int b = 0; b < lo; b++) {
    const unsigned half = 1u << b;
    const Fr p = fr_load(point + (size_t)b * 8);
#pragma unroll 1
    for (unsigned i = threadIdx.x; i < half; i += blockDim.x) {
      const Fr x = fr_load(lds + i * 8);
      const Fr y = frs_mul(x, p);
      fr_store(lds + (i + half) * 8, y);
      fr_store(lds + i * 8, fr_sub(x, y));
    }
    __syncthreads();
  }
  const unsigned words = 2u << lo;                                 // 16-byte words of the tile
  uint4* dst = reinterpret_cast<uint4*>(out) + (size_t)blockIdx.x * words;
  for (unsigned i = threadIdx.x; i < words; i += blockDim.x) dst[i] = *reinterpret_cast<const uint4*>(lds + i * 4);
}

// ---- the sums of a workgroup --------------------------------------------------------------------------------------------------------
// Every lane holds `nd` <= 7 canonical values v[0 .. nd); dst[t] = the sum of v[t] over the workgroup, t < nd, in a fixed order: down the
// wavefront by shuffles, then the wavefronts in turn.  wrec: frm_sum_lds_words of LDS.  All lanes of the workgroup call this.
DEV void frm_block_sums(const Fr* v, unsigned nd, u32* wrec, u32* dst) {
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (unsigned t = 0; t < (unsigned)FRM_MAX_EVALS; t++) {
    if (t < nd) {
      Fr s = v[t];
#pragma unroll 1
      for (unsigned d = 32; d; d >>= 1) s = fr_add(s, frs_shfl(s, d, true));     // lane 0 ends with the sum of all 64 (the others' values are unused)
      if (lane == 0) fr_store(wrec + (w * FRM_MAX_EVALS + t) * 8, s);
    }
  }
  __syncthreads();
  if (threadIdx.x < nd) {
    Fr s = fr_zero();
#pragma unroll 1
    for (unsigned i = 0; i < nw; i++) s = fr_add(s, fr_load(wrec + (i * FRM_MAX_EVALS + threadIdx.x) * 8));
    fr_store(dst + threadIdx.x * 8, s);
  }
}

// ---- a tile of positions, all tables, all evaluation points -------------------------------------------------------------------------
// word offset in LDS of half `hf` of this lane's slot s (slot 2 j: f_j(t), slot 2 j + 1: delta_j)
DEV unsigned frm_slot(unsigned s, unsigned hf) { return ((s * 2 + hf) * blockDim.x + threadIdx.x) * 4; }
DEV FrL frm_slot_load(const u32* vals, unsigned s) {
  const uint4 a = *reinterpret_cast<const uint4*>(vals + frm_slot(s, 0)), b = *reinterpret_cast<const uint4*>(vals + frm_slot(s, 1));
  Fr v;
  v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w; v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
  return frl_unpack(v);
}
DEV void frm_slot_store(u32* vals, unsigned s, const FrL& x) {      // x: A1, value < 2r < 2^256
  const Fr v = frl_pack(x);
  *reinterpret_cast<uint4*>(vals + frm_slot(s, 0)) = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  *reinterpret_cast<uint4*>(vals + frm_slot(s, 1)) = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
DEV FrL frm_coef(const FrmProg& prog, unsigned t) {
  Fr v;
  for (int i = 0; i < 8; i++) v.l[i] = prog.coef[t][i];
  return frl_unpack(v);
}

// tables: k tables `pitch` scalars apart; npos: positions per table -- h = 2^(m-1), or FUSED q = 2^(m-2): the tables are first folded at
// *r_prev in place (results at i and i + q of every table, the upper half is left as it is) and the evaluations are those of the folded
// tables.  rec: this workgroup's record of prog.deg + 1 scalars at rec + blockIdx.x * (prog.deg + 1) * 8.
template <bool FUSED>
__global__ void __launch_bounds__(FRM_BLOCK, 2) k_frm_round(u32* tables, size_t pitch, size_t npos, unsigned k, unsigned chunk, FrmProg prog, const u32* __restrict__ r_prev,
                                                             u32* __restrict__ rec) {
  BLS_DYN_LDS(lds);
  u32* vals = lds;
  u32* wrec = lds + (size_t)blockDim.x * 2 * k * 8;
  const unsigned nd = prog.deg + 1;
  FrL acc[FRM_MAX_EVALS];
#pragma unroll
  for (int t = 0; t < FRM_MAX_EVALS; t++) acc[t] = frm_zero();
  FrL r5 = frm_zero();
  if (FUSED) r5 = frm_challenge(r_prev);
  const size_t base = (size_t)blockIdx.x * blockDim.x * chunk;
#pragma unroll 1
  for (unsigned c = 0; c < chunk; c++) {
    const size_t i = base + (size_t)c * blockDim.x + threadIdx.x;
    if (i >= npos) break;                                          // the last tile may be ragged; the sums below are reached by every lane
#pragma unroll 1
    for (unsigned j = 0; j < k; j++) {
      u32* row = tables + (j * pitch + i) * 8;
      FrL lo, hi;
      if (FUSED) {
        const FrL a0 = frl_load(row), a1 = frl_load(row + npos * 8), a2 = frl_load(row + 2 * npos * 8), a3 = frl_load(row + 3 * npos * 8);
        lo = frm_fold(a0, a2, r5);                                 // A1 V2
        hi = frm_fold(a1, a3, r5);
        fr_store(row, frl_canon(lo));
        fr_store(row + npos * 8, frl_canon(hi));
      } else {
        lo = frl_load(row);
        hi = frl_load(row + npos * 8);
      }
      frm_slot_store(vals, 2 * j, lo);
      frm_slot_store(vals, 2 * j + 1, frl_reduce(frl_sub<1>(hi, lo)));      // A3 V6 -> A1 V2
    }
#pragma unroll 1
    for (unsigned t = 0; t < nd; t++) {
      FrL s = frm_zero();
      int lazy = 0;
#pragma unroll 1
      for (unsigned term = 0; term < prog.n_terms; term++) {
        const unsigned e0 = prog.ptr[term], e1 = prog.ptr[term + 1];
        FrL p = frm_slot_load(vals, 2u * prog.tab[e0]);
#pragma unroll 1
        for (unsigned e = e0 + 1; e <= e1; e++)                    // the factors, then the coefficient: ONE call site of the product
          p = frl_mul(p, e < e1 ? frm_slot_load(vals, 2u * prog.tab[e]) : frm_coef(prog, term));
        s = frl_add(s, p);
        if (++lazy == FRM_LAZY) { s = frl_reduce(s); lazy = 0; }   // <= A3 V6 -> A1 V2
      }
#pragma unroll
      for (unsigned u = 0; u < (unsigned)FRM_MAX_EVALS; u++)
        if (u == t) acc[u] = frl_reduce(frl_add(acc[u], s));       // <= A4 V8 -> A1 V2
      if (t + 1 < nd) {
#pragma unroll 1
        for (unsigned j = 0; j < k; j++)
          frm_slot_store(vals, 2 * j, frl_reduce(frl_add(frm_slot_load(vals, 2 * j), frm_slot_load(vals, 2 * j + 1))));      // A2 V4 -> A1 V2
      }
    }
  }
  Fr v[FRM_MAX_EVALS];
#pragma unroll
  for (int t = 0; t < FRM_MAX_EVALS; t++) v[t] = frl_canon(acc[t]);
  frm_block_sums(v, nd, wrec, rec + (size_t)blockIdx.x * nd * 8);
}

// evals[t] = the sum of the n_rec records' scalar t, t < nd: ONE workgroup, lane l takes records l, l + blockDim.x, ...
__global__ void __launch_bounds__(FRM_BLOCK) k_frm_round_finish(const u32* __restrict__ rec, size_t n_rec, unsigned nd, u32* __restrict__ evals) {
  BLS_DYN_LDS(lds);
  Fr v[FRM_MAX_EVALS];
#pragma unroll
  for (unsigned t = 0; t < (unsigned)FRM_MAX_EVALS; t++) {
    v[t] = fr_zero();
    if (t < nd) {
#pragma unroll 1
      for (size_t i = threadIdx.x; i < n_rec; i += blockDim.x) v[t] = fr_add(v[t], fr_load(rec + (i * nd + t) * 8));
    }
  }
  frm_block_sums(v, nd, lds, evals);
}

}  // namespace bls
