// fr_frac.hip.h -- the fused front of the Fr fraction scans: the accumulator column of a permutation argument
// (blsgpu_fr_grand_product*) and of a log-derivative lookup argument (blsgpu_fr_frac_sum*) from their column sets in ONE pass.
//
//     grand product   f[i] = prod_j (na_j[i] + beta nb_j[i] + gamma)  *  inv0( prod_j (da_j[i] + beta db_j[i] + gamma) )      PRODUCT scan of f
//     fraction sum    f[i] = sum_j  m_j[i] * inv0( gamma + da_j[i] + beta db_j[i] )                                           SUM scan of f
//
// The arithmetic is scalar.hip.h's (fr_add / fr_mul: scalar.rs:435-503) and fr_scan.hip.h's inversion (frs_inv, the same canonical
// element as Scalar::invert, scalar.rs:505-580); the scan behind the front is fr_scan.hip.h's, unchanged: k_frf_front ends in
// frs_tile_body, so it leaves what k_frs_tile's REDUCE mode leaves (or, in SINGLE mode, the finished call), and k_frs_agg and
// k_frs_tile<PRODUCT | SUM> in SCAN mode run on `out` in place (fr_frac_plan.h).
//
// One pass, one inversion per tile whatever c is.  Both operations carry a PAIR per element through the columns:
//     grand product   N <- N n_j            D <- D d_j
//     fraction sum    S <- S d_j + m_j P    P <- P d_j          (S / P = sum_j m_j / d_j: three products per column, none of them an inversion)
// and divide once at the end, by Montgomery's trick over the tile's `block x chunk` denominators exactly as k_frs_invert does: chunk
// prefix products in registers, the lane totals scanned forward and backward, one frs_inv by one wavefront, a backward sweep.  A zero
// denominator factor is replaced by 1 and remembered (per element, a bit per chunk slot): the grand product's f[i] is then 0, the
// fraction sum drops that one term (m_j taken as 0) and keeps the others -- inv0's convention, so the results are limb-identical to the
// composition fr_op / fr_batch_invert / fr_scan_many (field elements are canonical: equal values are equal limbs).
//
// Data movement.  The tables pass ONE AT A TIME through the tile's LDS buffer (frs_tile_load: 16-byte words, consecutive lanes on
// consecutive words), each lane then picks its own chunk into registers, so LDS is the scan's 36 KB tile whatever c is and a lane's
// state is three elements per chunk slot (N / S, D / P, the factor being built).  Two barriers per table.  The challenges are read
// from device memory by every lane (a uniform address: scalar loads), so a transcript on the device feeds them without a host round trip.
// Aliased input sets (num_a == den_a in the permutation argument) are simply read twice: the second read of a tile comes from L2, and
// sharing it would need a second factor per slot in registers.
#pragma once
#include "fr_scan.hip.h"
#include "fr_frac_plan.h"

namespace bls {

// t[e] = a[e] + beta * b[e] + gamma for the lane's chunk of the tile (b == NULL: a[e] + gamma); a, b: the tables' base pointers
DEV void frf_factor(Fr* t, const u32* a, const u32* b, const u32* __restrict__ chal, size_t base, unsigned cnt, unsigned chunk, unsigned s0, unsigned mine, u32* lds) {
  const Fr gamma = fr_load(chal + 8);
  if (b) {
    const Fr beta = fr_load(chal);
    __syncthreads();                                    // the lanes are done with the table before
    frs_tile_load<false>(b, base, cnt, 0, chunk, lds);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < FRF_CHUNK_MAX; e++)
      if ((unsigned)e < mine) t[e] = fr_add(frs_mul(beta, fr_load(lds + frs_lds_addr(s0 + e, chunk))), gamma);
  } else {
#pragma unroll
    for (int e = 0; e < FRF_CHUNK_MAX; e++) t[e] = gamma;
  }
  __syncthreads();
  frs_tile_load<false>(a, base, cnt, 0, chunk, lds);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < FRF_CHUNK_MAX; e++)
    if ((unsigned)e < mine) t[e] = fr_add(fr_load(lds + frs_lds_addr(s0 + e, chunk)), t[e]);
}

// One tile of blockDim.x * chunk elements per workgroup, chunk <= FRF_CHUNK_MAX.  mode FRS_K_SINGLE: the whole call; FRS_K_REDUCE: f to
// out, the tile's aggregate to agg_out[blockIdx.x], the lanes' prefixes to lane_rec, as k_frs_tile.
// OP = FRF_GRAND_PRODUCT: xa / xb = num_a / num_b; FRF_FRAC_SUM: xa = mult (NULL: every multiplicity is 1), xb unused.  xb, db may be NULL.
// Table j of a set is at + j * pitch scalars.  chal: beta, gamma.  flags: k * len bytes or NULL.  out and flags overlap no input.
template <int OP>
__global__ void __launch_bounds__(FRS_BLOCK, 2) k_frf_front(int mode, int exclusive, int c, const u32* xa, const u32* xb, const u32* da, const u32* db, size_t pitch,
                                                            const u32* __restrict__ chal, size_t len, size_t k, unsigned chunk, u32* __restrict__ out,
                                                            uint8_t* __restrict__ flags, u32* __restrict__ agg_out, u32* lane_rec) {
  BLS_DYN_LDS(lds);
  const size_t total = len * k;
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= total) return;
  const unsigned cnt = total - base < (size_t)tile ? (unsigned)(total - base) : tile;
  u32* wrec = lds + blockDim.x * (chunk * 8 + 4);
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;
  Fr X[FRF_CHUNK_MAX], P[FRF_CHUNK_MAX], t[FRF_CHUNK_MAX];      // numerator (N / S), denominator product, the factor in hand
  u32 zmask = 0;                                                // bit e: a denominator factor of slot e was zero
#pragma unroll 1
  for (int j = 0; j < c; j++) {
    const size_t off = (size_t)j * pitch * 8;
    if (OP == FRF_GRAND_PRODUCT) {
      frf_factor(t, xa + off, xb ? xb + off : nullptr, chal, base, cnt, chunk, s0, mine, lds);
#pragma unroll
      for (int e = 0; e < FRF_CHUNK_MAX; e++)
        if ((unsigned)e < mine) X[e] = j ? frs_mul(X[e], t[e]) : t[e];
      frf_factor(t, da + off, db ? db + off : nullptr, chal, base, cnt, chunk, s0, mine, lds);
#pragma unroll
      for (int e = 0; e < FRF_CHUNK_MAX; e++)
        if ((unsigned)e < mine) {
          if (fr_is_zero(t[e])) { zmask |= 1u << e; t[e] = fr_one(); }
          P[e] = j ? frs_mul(P[e], t[e]) : t[e];
        }
    } else {
      frf_factor(t, da + off, db ? db + off : nullptr, chal, base, cnt, chunk, s0, mine, lds);
      if (xa) {
        __syncthreads();
        frs_tile_load<false>(xa + off, base, cnt, 0, chunk, lds);
        __syncthreads();
      }
#pragma unroll
      for (int e = 0; e < FRF_CHUNK_MAX; e++)
        if ((unsigned)e < mine) {
          const bool zero = fr_is_zero(t[e]);
          if (zero) { zmask |= 1u << e; t[e] = fr_one(); }
          const Fr m = zero ? fr_zero() : (xa ? fr_load(lds + frs_lds_addr(s0 + e, chunk)) : fr_one());
          if (j) {
            const Fr mp = (xa && !zero) ? frs_mul(m, P[e]) : (zero ? m : P[e]);
            X[e] = fr_add(frs_mul(X[e], t[e]), mp);
            P[e] = frs_mul(P[e], t[e]);
          } else { X[e] = m; P[e] = t[e]; }
        }
    }
  }
  // 1 / P for the whole tile (k_frs_invert's schedule; the denominators hold no zero any more).  The lane parks its denominators in its
  // own slots -- nobody else reads them -- and keeps their prefix products.
  Fr prod = fr_one();
#pragma unroll
  for (int e = 0; e < FRF_CHUNK_MAX; e++)
    if ((unsigned)e < mine) {
      fr_store(lds + frs_lds_addr(s0 + e, chunk), P[e]);
      prod = e ? frs_mul(prod, P[e]) : P[e];
      P[e] = prod;
    }
  const Fr before = frs_block_prod_excl<false>(prod, wrec);
  const Fr after = frs_block_prod_excl<true>(prod, wrec);
  if (threadIdx.x < 64) {                              // one wavefront inverts the tile's total (every lane holds the same total)
    const Fr inv = frs_inv(frs_mul(frs_mul(before, prod), after));
    if (threadIdx.x == 0) fr_store(wrec, inv);
  }
  __syncthreads();
  Fr r = frs_mul(frs_mul(fr_load(wrec), before), after);      // 1 / (the lane's chunk total)
#pragma unroll
  for (int e = FRF_CHUNK_MAX - 1; e >= 0; e--)
    if ((unsigned)e < mine) {
      u32* slot = lds + frs_lds_addr(s0 + e, chunk);
      const Fr x = fr_load(slot);
      const Fr o = e ? frs_mul(P[e ? e - 1 : 0], r) : r;
      r = frs_mul(r, x);
      const bool zero = (zmask >> e) & 1u;
      fr_store(slot, (OP == FRF_GRAND_PRODUCT && zero) ? fr_zero() : frs_mul(X[e], o));
      if (flags) flags[base + s0 + e] = zero ? 0 : 1;
    }
  __syncthreads();                                     // wrec is free again, f is in LDS
  frs_tile_body<frf_scan_op(OP)>(mode, exclusive, lds, wrec, nullptr, len, k, chunk, base, cnt, agg_out, nullptr, lane_rec);
  __syncthreads();
  frs_tile_store<false>(out, base, cnt, total, chunk, lds);
}

}  // namespace bls
