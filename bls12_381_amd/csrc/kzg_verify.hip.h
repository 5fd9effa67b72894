// kzg_verify.hip.h -- the kernels of batched KZG cell-proof verification (blsgpu_kzg_verify_cells[_device]) that no other call has:
// the offsets the chain walks, the per-cell weights with the gather of the points, the fold of m interpolation polynomials into one
// per batch, and the finish that forms (A_s, B_s) and lays out the pairing terms.  kzg_verify_plan.h holds the maps, the cut and the
// scratch layout; api_msm.hip launches from it and runs the stages between these kernels through the entry points that exist
// (mul_batch, batch_normalize, sum_segments, fr_ntt_many, msm_segments, multi_miller_loop_prepared_many, gt_is_identity).
//
// The Fr arithmetic is scalar.hip.h's (fr_mul / fr_add: scalar.rs:435-503): canonical results, so every limb is the definition's.
// A power of w is a product over the set bits of its exponent of the handle's table tab[b] = winv^(2^b), b <= log_n: at most log_n + 1
// products, no table proportional to n.  The fold is the Fr hot path: about m l (log_n + 3) products.
// -DKZGV_FAULT=n seeds one fault for tests/test_simt_kzg_verify.py (1: rho's exponent is k where k - off(s) belongs, 2: h^(+u) in place
// of h^(-u), 3: the fold drops the last cell of a chunk).
#pragma once
#include "msm.hip.h"
#include "generators.hip.h"
#include "kzg_verify_plan.h"

#ifndef KZGV_FAULT
#define KZGV_FAULT 0
#endif

namespace bls {

DEV Fr kzgv_root() {                                          // ROOT_OF_UNITY (scalar.rs:200-205), of order 2^32
  constexpr FrWords k = {BLS_FR_ROOT_W};
  Fr r;
  for (int i = 0; i < 8; i++) r.l[i] = k.w[i];
  return r;
}
// winv^x for x < 2n from the table of winv^(2^b)
DEV Fr kzgv_tab_pow(const u32* __restrict__ tab, uint64_t x, int log_n) {
  Fr acc = fr_one();
  bool first = true;
#pragma unroll 1
  for (int b = 0; b <= log_n; b++) {
    if (!((x >> b) & 1)) continue;
    const Fr t = fr_load(tab + (size_t)b * 8);
    acc = first ? t : fr_mul(acc, t);
    first = false;
  }
  return acc;
}
// a^e by squaring: e = 0 gives 1 whatever a is
DEV Fr kzgv_pow_u32(const Fr& a, u32 e) {
  Fr acc = fr_one(), sq = a;
#pragma unroll 1
  for (; e; e >>= 1) {
    if (e & 1) acc = fr_mul(acc, sq);
    if (e > 1) sq = fr_sqr(sq);
  }
  return acc;
}

// create: tab[b] = winv^(2^b) for b <= log_n, winv the inverse of the root blsgpu_fr_ntt uses for log_n + 1; one lane
__global__ void k_kzgv_roots(u32* __restrict__ tab, int log_n) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Fr w = kzgv_root();
  for (int i = 0; i < 31 - log_n; i++) w = fr_sqr(w);          // of order 2n
  Fr winv = w, p = w;                                          // w^(2n - 1): the product of w^(2^b), b <= log_n
  for (int b = 1; b <= log_n; b++) { p = fr_sqr(p); winv = fr_mul(winv, p); }
  for (int b = 0; b <= log_n; b++) { fr_store(tab + (size_t)b * 8, winv); winv = fr_sqr(winv); }
}

// create: slot 1 of the two points the handle's `G2Prepared` table is made of = -G2 (g2.rs:103-140 negated), and both flags; slot 0 is
// the caller's q, copied in before
__global__ void k_kzgv_table_points(u32* __restrict__ xy, uint8_t* __restrict__ inf, int q_inf) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Aff<Fp2Policy> h = generator<Fp2Policy>();
  Wire<Fp2Policy>::save(h.x, xy + 48); Wire<Fp2Policy>::save(neg(h.y), xy + 72);
  inf[0] = q_inf ? 1 : 0; inf[1] = 0;
}

// The offsets every later stage walks, by ONE workgroup: eff[i] = the running maximum of v_j, j <= i, with v_0 = 0, v_nseg = m and
// v_j = min(offsets[j], m) between; mis[i] = the caller's offsets[i] is another value.  Lane t owns the entries [t S, (t + 1) S): it
// takes their maximum, reads the maxima of the lanes before it, and walks its entries again.  Also the arrays that depend on the
// offsets alone: the u64 offsets of the segment sums over the three thirds of the products, the offsets s l and the base_first 0 of
// the MSM over S[0..l).  Nothing here is indexed by a value the caller wrote.
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_offsets(const u32* __restrict__ offsets, u32 nseg, u32 m, int log_l, u32* __restrict__ eff, uint8_t* __restrict__ mis,
                                                             unsigned long long* __restrict__ off64, u32* __restrict__ msm_off, u32* __restrict__ base_first,
                                                             u32* __restrict__ status) {
  __shared__ u32 mx[KZGV_BLOCK];
  const u32 t = threadIdx.x, B = blockDim.x;
  const u32 S = (nseg + 1 + B - 1) / B;
  const size_t lo = (size_t)t * S, hi = lo + S < (size_t)nseg + 1 ? lo + S : (size_t)nseg + 1;
  u32 run = 0;
  for (size_t i = lo; i < hi; i++) {
    const u32 o = offsets[i];
    const u32 v = i == 0 ? 0u : i == nseg ? m : (o < m ? o : m);
    run = v > run ? v : run;
  }
  mx[t] = run;
  __syncthreads();
  run = 0;
  for (u32 j = 0; j < t; j++) run = mx[j] > run ? mx[j] : run;
  bool any = false;
  for (size_t i = lo; i < hi; i++) {
    const u32 o = offsets[i];
    const u32 v = i == 0 ? 0u : i == nseg ? m : (o < m ? o : m);
    run = v > run ? v : run;
    eff[i] = run;
    mis[i] = o != run ? 1 : 0;
    any = any || o != run;
    msm_off[i] = (u32)(i << log_l);
    if (i < nseg) {
      base_first[i] = 0;
      for (u32 th = 0; th < 3; th++) off64[(size_t)th * nseg + i] = (unsigned long long)th * m + run;
    } else {
      off64[(size_t)3 * nseg] = (unsigned long long)3 * m;
    }
  }
  if (any) atomicOr(status, KZGV_STATUS_BAD);
}

// A lane per cell k: rho_k and rho_k a_k, and the 3 m (point, scalar) pairs of ONE mul_batch -- (proof_k, rho_k) at k, (proof_k,
// rho_k a_k) at m + k, (commit[row_k], rho_k) at 2 m + k.  A row or col out of range is never used as an index: the cell is multiplied
// by 0, its commitment slot is an identity, the batch's flag and the status bit are raised.
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_weights(const u32* __restrict__ eff, u32 nseg, u32 m, const u32* __restrict__ row, const u32* __restrict__ col, u32 ncommit,
                                                             const u32* __restrict__ r, const u32* __restrict__ tab, const uint2* __restrict__ commit_xy,
                                                             const uint8_t* __restrict__ commit_inf, const uint2* __restrict__ proof_xy, const uint8_t* __restrict__ proof_inf,
                                                             int log_n, int log_l, int order, u32* __restrict__ scal, uint2* __restrict__ pxy, uint8_t* __restrict__ pinf,
                                                             uint8_t* __restrict__ badidx, u32* __restrict__ status) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const u32 s = kzgv_seg_of(eff, nseg, (u32)k);
#if KZGV_FAULT == 1
  const u32 e = (u32)k;
#else
  const u32 e = (u32)k - eff[s];
#endif
  u32 j = col[k], rw = row[k];
  const bool ok = j < ((u32)2 << (log_n - log_l)) && rw < ncommit;
  Fr rho = kzgv_pow_u32(fr_load(r + (size_t)s * 8), e);
  if (!ok) {
    rho = fr_zero(); j = 0; rw = 0;
    badidx[s] = 1;
    atomicOr(status, KZGV_STATUS_BAD);
  }
  const Fr a = kzgv_tab_pow(tab, kzgv_a_exponent(kzgv_shift_exponent(j, log_n, log_l, order), log_n, log_l), log_n);
  fr_store(scal + k * 8, rho);
  fr_store(scal + ((size_t)m + k) * 8, fr_mul(rho, a));
  fr_store(scal + ((size_t)2 * m + k) * 8, rho);
  const uint2* p = proof_xy + k * 12;                          // (the caller's point arrays are 8-byte aligned: 8-byte words)
  const uint2* cm = commit_xy + (size_t)rw * 12;
#pragma unroll
  for (int q = 0; q < 12; q++) {
    const uint2 v = p[q];
    pxy[k * 12 + q] = v; pxy[((size_t)m + k) * 12 + q] = v;
    pxy[((size_t)2 * m + k) * 12 + q] = ok ? cm[q] : make_uint2(0, 0);
  }
  const uint8_t pi = proof_inf[k] ? 1 : 0;
  pinf[k] = pi; pinf[(size_t)m + k] = pi;
  pinf[(size_t)2 * m + k] = ok ? (commit_inf[rw] ? 1 : 0) : 1;
}

// The fold, pass 1: lane (chunk q, column u) adds rho_k h_k^(-u) c_k[u] over the chunk's cells in order, c_k the inverse transform of
// cell k in natural coset order, and closes a batch where it ends (kzg_verify_plan.h: final in agg, or a HEAD / TAIL partial).
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_fold_chunks(const u32* __restrict__ eff, u32 nseg, u32 m, const u32* __restrict__ col, const u32* __restrict__ rho,
                                                                 const u32* __restrict__ cellc, const u32* __restrict__ tab, int log_n, int log_l, int order, u32 chunk,
                                                                 u32 nchunks, u32* __restrict__ agg, u32* __restrict__ part) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nchunks << log_l)) return;
  const size_t q = g >> log_l, u = g & (((size_t)1 << log_l) - 1);
  const u32 cb = (u32)(q * chunk), ce = m - cb < chunk ? m : cb + chunk;
  u32 s = kzgv_seg_of(eff, nseg, cb), so = eff[s], se = eff[s + 1];
  Fr acc = fr_zero();
  auto close = [&]() {
    if (se <= so) return;
    u32* o = kzgv_inside(so, se, cb, chunk) ? agg + (((size_t)s << log_l) + u) * 8 : part + ((kzgv_record(q, so, cb) << log_l) + u) * 8;
    fr_store(o, acc);
  };
#if KZGV_FAULT == 3
  const u32 stop = ce - 1;
#else
  const u32 stop = ce;
#endif
#pragma unroll 1
  for (u32 k = cb; k < stop; k++) {
    while (k >= se) { close(); s++; so = se; se = eff[s + 1]; acc = fr_zero(); }
    const uint64_t e = kzgv_shift_exponent(col[k], log_n, log_l, order);
#if KZGV_FAULT == 2
    const uint64_t x = kzgv_inv_power_exponent(((uint64_t)2 << log_n) - (e & (((uint64_t)2 << log_n) - 1)), u, log_n);
#else
    const uint64_t x = kzgv_inv_power_exponent(e, u, log_n);
#endif
    const Fr w = fr_mul(fr_load(rho + (size_t)k * 8), kzgv_tab_pow(tab, x, log_n));
    acc = fr_add(acc, fr_mul(w, fr_load(cellc + (((size_t)k << log_l) + u) * 8)));
  }
  close();
}
// pass 2: lane (batch s, column u) writes 0 for an empty batch and the sum of the partials for one that spans several chunks
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_fold_combine(const u32* __restrict__ eff, u32 nseg, int log_l, u32 chunk, const u32* __restrict__ part, u32* __restrict__ agg) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)nseg << log_l)) return;
  const size_t s = g >> log_l, u = g & (((size_t)1 << log_l) - 1);
  const u32 so = eff[s], se = eff[s + 1];
  if (se <= so) { fr_store(agg + g * 8, fr_zero()); return; }
  const size_t q0 = so / chunk, q1 = (se - 1) / chunk;
  if (q0 == q1) return;                                        // inside one chunk: final since pass 1
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t q = q0; q <= q1; q++) acc = fr_add(acc, fr_load(part + ((kzgv_record(q, so, (u32)(q * chunk)) << log_l) + u) * 8));
  fr_store(agg + g * 8, acc);
}

// A lane per batch: A_s = T1, B_s = T3 + T2 - M from the segment sums of the three thirds (sum[t nseg + s]) and the MSM over S[0..l),
// by the complete formulas (identities, equal and opposite operands need no case); an identity pair for a batch that is broken or
// holds a bad index.  The pair goes to the chain's scratch and, if asked, to the caller; the two pairing terms of the batch are
// (A_s, table[0] = q) and (B_s, table[1] = -G2).
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_finish(const u32* __restrict__ sum, const u32* __restrict__ msm, const uint8_t* __restrict__ mis,
                                                            const uint8_t* __restrict__ badidx, u32 nseg, u32* __restrict__ ab, u32* __restrict__ out_ab, u32* __restrict__ qidx,
                                                            unsigned long long* __restrict__ poff, uint8_t* __restrict__ bad) {
  typedef FpPolicy F;
  constexpr int WW = Wire<F>::WORDS;
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  auto load = [](const u32* w) {
    Proj<F> p;
    p.x = F::st(Wire<F>::load(w)); p.y = F::st(Wire<F>::load(w + WW)); p.z = F::st(Wire<F>::load(w + 2 * WW));
    return p;
  };
  auto save = [](const Proj<F>& p, u32* o) { Wire<F>::save(p.x, o); Wire<F>::save(p.y, o + WW); Wire<F>::save(p.z, o + 2 * WW); };
  const bool b = mis[s] || mis[s + 1] || badidx[s];
  Proj<F> A = pt_identity<F>(), Bp = pt_identity<F>();
  if (!b) {
    A = load(sum + s * 3 * WW);
    Bp = pt_add<F>(pt_add<F>(load(sum + ((size_t)2 * nseg + s) * 3 * WW), load(sum + ((size_t)nseg + s) * 3 * WW)), pt_neg<F>(load(msm + s * 3 * WW)));
  }
  save(A, ab + (2 * s) * 3 * WW); save(Bp, ab + (2 * s + 1) * 3 * WW);
  if (out_ab) { save(A, out_ab + (2 * s) * 3 * WW); save(Bp, out_ab + (2 * s + 1) * 3 * WW); }
  qidx[2 * s] = 0; qidx[2 * s + 1] = 1;
  poff[s] = 2 * s;
  if (s + 1 == nseg) poff[nseg] = (unsigned long long)2 * nseg;
  bad[s] = b ? 1 : 0;
}

// verdict = the pairing product is the identity and the batch is neither broken nor holds a bad index
__global__ void __launch_bounds__(KZGV_BLOCK) k_kzgv_verdict(const uint8_t* __restrict__ isone, const uint8_t* __restrict__ bad, u32 nseg, uint8_t* __restrict__ verdict) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  verdict[s] = isone[s] && !bad[s] ? 1 : 0;
}

}  // namespace bls
