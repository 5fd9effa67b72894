// kzg_recover.hip.h -- the kernels of KZG cell recovery (blsgpu_kzg_recover[_device]): everything around the three Fr transforms and the
// batch inversion that rebuild a polynomial from c of its 2c cells.  kzg_recover_plan.h holds the mathematics, the index maps, the
// scratch layout, the order of the stages and the launch shapes; api_fr.hip launches from it.  The Fr arithmetic is fr.hip.h's: every
// scalar is eight u32 words of canonical Montgomery limbs.
//
// Nothing here is indexed by a value the caller wrote: the offsets walked are the effective ones, a cell number is compared with 2c
// before it selects a slot, and the slot table the later stages gather through is this file's own.
// -DKZG_REC_FAULT=n seeds one fault for tests/test_simt_kzg_recover.py (1: the scatter ignores the bit reversal of the entry number,
// 2: the vanish kernel skips the last root of every LDS tile's list, 3: the check ORs only the first half of Q[n..2n)).
#pragma once
#include "fr.hip.h"
#include "kzg_recover_plan.h"

#ifndef KZG_REC_FAULT
#define KZG_REC_FAULT 0
#endif

namespace bls {

// The offsets every later stage walks, by ONE workgroup (the scan of k_kzgv_offsets): eff[i] = the running maximum of v_j, j <= i, with
// v_0 = 0, v_count = m and v_j = min(offsets[j], m) between; mis[i] = the caller's offsets[i] is another value.
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_offsets(const u32* __restrict__ offsets, u32 count, u32 m, u32* __restrict__ eff, uint8_t* __restrict__ mis) {
  __shared__ u32 mx[KZGR_BLOCK];
  const u32 t = threadIdx.x, B = blockDim.x;
  const u32 S = (count + 1 + B - 1) / B;
  const size_t lo = (size_t)t * S, hi = lo + S < (size_t)count + 1 ? lo + S : (size_t)count + 1;
  u32 run = 0;
  for (size_t i = lo; i < hi; i++) {
    const u32 o = offsets[i];
    const u32 v = i == 0 ? 0u : i == count ? m : (o < m ? o : m);
    run = v > run ? v : run;
  }
  mx[t] = run;
  __syncthreads();
  run = 0;
  for (u32 j = 0; j < t; j++) run = mx[j] > run ? mx[j] : run;
  for (size_t i = lo; i < hi; i++) {
    const u32 o = offsets[i];
    const u32 v = i == 0 ? 0u : i == count ? m : (o < m ? o : m);
    run = v > run ? v : run;
    eff[i] = run;
    mis[i] = o != run ? 1 : 0;
  }
}

// A workgroup per polynomial v: slot[v][i] = the index k of the received cell with col[k] = i, or -1.  The 2c slots live in LDS; the
// lanes walk the cells [eff[v], eff[v + 1]) and claim slot[col] with a compare-and-swap, so a second claim of one slot is a duplicate.
// status[v] = the KZGR_ST_* bits (0: good); a polynomial with any bit gets an all -1 table (nothing of it is gathered) and raises the
// context's sticky word.  Also clears upper[v], the word the check kernel ORs into.
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_slots(const u32* __restrict__ eff, const uint8_t* __restrict__ mis, const u32* __restrict__ col, int log_c,
                                                              int* __restrict__ slot, u32* __restrict__ status, u32* __restrict__ upper, u32* __restrict__ sticky) {
  __shared__ int s_slot[1 << KZGR_MAX_LOG_CELLS];
  __shared__ u32 s_bad, s_got;
  const u32 v = blockIdx.x, t = threadIdx.x, B = blockDim.x;
  const u32 cells = 2u << log_c;
  for (u32 i = t; i < cells; i += B) s_slot[i] = -1;
  if (t == 0) { s_bad = (mis[v] | mis[v + 1]) ? KZGR_ST_OFFSETS : 0; s_got = 0; }
  __syncthreads();
  const bool broken = s_bad != 0;                  // uniform: read before any lane ORs into it
  __syncthreads();
  if (!broken) {
    const u32 lo = eff[v], hi = eff[v + 1];
    for (u32 k = lo + t; k < hi; k += B) {
      const u32 i = col[k];
      if (i >= cells) { atomicOr(&s_bad, KZGR_ST_COL); continue; }
      if (atomicCAS(&s_slot[i], -1, (int)k) != -1) atomicOr(&s_bad, KZGR_ST_DUP);
      else atomicAdd(&s_got, 1u);
    }
  }
  __syncthreads();
  u32 st = s_bad;
  if (s_got * 2 < cells) st |= KZGR_ST_FEW;
  for (u32 i = t; i < cells; i += B) slot[(size_t)v * cells + i] = st ? -1 : s_slot[i];
  if (t == 0) {
    status[v] = st; upper[v] = 0;
    if (st) atomicOr(sticky, KZGR_STATUS_BAD);
  }
}

// rootd[rho] = (w^l)^rho and rootc[rho] = g^l (w^l)^rho for rho < 2c; a lane per residue.  w^l is the root of unity of order 2c.
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_roots(u32* __restrict__ rootd, u32* __restrict__ rootc, FrArg g, int log_c, int log_l) {
  const u32 rho = blockIdx.x * blockDim.x + threadIdx.x;
  if (rho >= (2u << log_c)) return;
  Fr gen;
  for (int i = 0; i < 8; i++) gen.l[i] = g.w[i];
  Fr b = fr_pow2k(fr_root_of_unity(), 32 - (log_c + 1)), d = fr_one();      // w^l, and its power rho from the low bit up (inline: no call, no scratch)
  for (int bit = 0; bit <= log_c; bit++) {
    if ((rho >> bit) & 1u) d = fr_mul(d, b);
    b = fr_sqr(b);
  }
  fr_store(rootd + (size_t)rho * 8, d);
  fr_store(rootc + (size_t)rho * 8, fr_mul(fr_pow2k(gen, log_l), d));
}

// Zd and Zc of every polynomial; a lane per table entry, 4c per polynomial: entry q < 2c is Zd[q] = Zs(rootd[q]), entry 2c + q is
// Zc[q] = Zs(rootc[q]).  The workgroup walks the 2c cells in tiles of `tile` <= KZGR_ROOT_TILE: lane u < tile looks at cell base + u
// and, when it is missing, appends its root a_i = rootd[residue(i)] to the tile's list in LDS (the place comes from an LDS counter: the
// product does not depend on the order, field arithmetic being exact); then every lane multiplies its y - a_i over the list, in two
// independent chains that are joined at the end.  A polynomial with a bad status gets tables of ones.
DEV Fr kzgr_lds_scalar(const uint4* lo, const uint4* hi, u32 u) {
  const uint4 a0 = lo[u], a1 = hi[u];
  Fr a;
  a.l[0] = a0.x; a.l[1] = a0.y; a.l[2] = a0.z; a.l[3] = a0.w; a.l[4] = a1.x; a.l[5] = a1.y; a.l[6] = a1.z; a.l[7] = a1.w;
  return a;
}
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_vanish(const int* __restrict__ slot, const u32* __restrict__ status, const u32* __restrict__ rootd,
                                                               const u32* __restrict__ rootc, int log_c, int order, u32 per_poly, u32 tile, u32* __restrict__ zd,
                                                               u32* __restrict__ zc) {
  __shared__ uint4 s_root[2][KZGR_ROOT_TILE];
  __shared__ u32 s_cnt;
  const u32 cells = 2u << log_c;
  const u32 v = blockIdx.x / per_poly, q = (blockIdx.x % per_poly) * blockDim.x + threadIdx.x, t = threadIdx.x;
  const bool live = q < 2 * cells;
  const bool good = status[v] == 0;
  Fr y = fr_one(), acc0 = fr_one(), acc1 = fr_one();
  if (live) y = fr_load(q < cells ? rootd + (size_t)q * 8 : rootc + (size_t)(q - cells) * 8);
  if (good) {
    for (u32 base = 0; base < cells; base += tile) {
      __syncthreads();
      if (t == 0) s_cnt = 0;
      __syncthreads();
      if (t < tile && base + t < cells) {
        const u32 i = base + t;
        if (slot[(size_t)v * cells + i] < 0) {
          const u32 at = atomicAdd(&s_cnt, 1u);
          const uint4* a = (const uint4*)(rootd + (size_t)kzgr_residue(i, log_c, order) * 8);
          s_root[0][at] = a[0]; s_root[1][at] = a[1];
        }
      }
      __syncthreads();
      u32 lim = s_cnt;
#if KZG_REC_FAULT == 2
      if (lim) lim--;
#endif
      u32 u = 0;
      for (; u + 1 < lim; u += 2) {
        acc0 = fr_mul(acc0, fr_sub(y, kzgr_lds_scalar(s_root[0], s_root[1], u)));
        acc1 = fr_mul(acc1, fr_sub(y, kzgr_lds_scalar(s_root[0], s_root[1], u + 1)));
      }
      if (u < lim) acc0 = fr_mul(acc0, fr_sub(y, kzgr_lds_scalar(s_root[0], s_root[1], u)));
    }
  }
  if (live) fr_store((q < cells ? zd + ((size_t)v * cells + q) * 8 : zc + ((size_t)v * cells + (q - cells)) * 8), fr_mul(acc0, acc1));
}

// EZ[v][j] = the received value at w^j times Zd[v][j mod 2c], or 0: per polynomial the transposition of an l x 2c matrix whose row of
// residue rho is gathered through the slot table.  A workgroup of T x T lanes owns one tile.  Lane (y, x) reads entry e0 + x of the cell
// of residue r0 + y -- consecutive lanes, consecutive scalars of one cell -- and writes residue r0 + x of row e0 + y -- consecutive
// lanes, consecutive scalars of EZ; the row of entry t is t itself, or bitrev(t, log_l) for ORDER_BITREV: the bit reversal moves whole
// rows of the target and costs neither side its coalescing.  Entries and residues past the matrix edge are skipped.
template <int T>
__global__ void __launch_bounds__(T * T) k_kzg_rec_scatter(const int* __restrict__ slot, const uint4* __restrict__ cells, const u32* __restrict__ zd, size_t count, int log_c,
                                                           int log_l, int order, uint4* __restrict__ ez) {
  __shared__ uint4 tile[2][T][T + 1];
  const size_t R = (size_t)1 << log_l, C = (size_t)2 << log_c;
  const size_t tiles_r = (R + T - 1) / T, tiles_c = (C + T - 1) / T;
  size_t b = blockIdx.x;
  const size_t tc = b % tiles_c; b /= tiles_c;
  const size_t tr = b % tiles_r; b /= tiles_r;
  const size_t v = b;
  const unsigned y = threadIdx.x / T, x = threadIdx.x % T;
  if (v < count) {
    const size_t rho = tc * T + y, e = tr * T + x;
    if (rho < C && e < R) {
      const int s = slot[v * C + (size_t)kzgr_cell_of_residue(rho, log_c, order)];
      uint4 a = make_uint4(0, 0, 0, 0), c2 = a;
      if (s >= 0) { const uint4* p = cells + (((size_t)s << log_l) + e) * 2; a = p[0]; c2 = p[1]; }
      tile[0][y][x] = a; tile[1][y][x] = c2;
    }
  }
  __syncthreads();
  if (v < count) {
    const size_t e = tr * T + y, rho = tc * T + x;
    if (rho < C && e < R) {
#if KZG_REC_FAULT == 1
      const size_t row = e;
#else
      const size_t row = order == KZGR_ORDER_BITREV ? (size_t)kzgr_bitrev(e, log_l) : e;
#endif
      const Fr a = kzgr_lds_scalar(tile[0][x], tile[1][x], y);
      const Fr r = fr_mul(a, fr_load(zd + (v * C + rho) * 8));
      fr_store((u32*)(ez + ((v << (log_c + 1 + log_l)) + (row << (log_c + 1)) + rho) * 2), r);
    }
  }
}

// x[v][j] *= zcinv[v][j mod 2c] over count * 2n scalars, in place; a lane per scalar
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_scale(u32* __restrict__ x, const u32* __restrict__ zcinv, size_t total, int log_n, int log_c) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t v = g >> (log_n + 1), rho = g & (((size_t)2 << log_c) - 1);
  fr_store(x + g * 8, fr_mul(fr_load(x + g * 8), fr_load(zcinv + ((v << (log_c + 1)) + rho) * 8)));
}

// upper[v] |= the OR of the words of Q[v][n .. 2n); a lane per coefficient, per_poly workgroups per polynomial, one atomic per workgroup
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_check(const u32* __restrict__ q, int log_n, u32 per_poly, u32* __restrict__ upper) {
  __shared__ u32 s_any;
  const size_t v = blockIdx.x / per_poly, j = (size_t)(blockIdx.x % per_poly) * blockDim.x + threadIdx.x;
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  size_t n_checked = (size_t)1 << log_n;
#if KZG_REC_FAULT == 3
  if (log_n > 0) n_checked >>= 1;
#endif
  if (j < n_checked) {
    const Fr a = fr_load(q + ((v << (log_n + 1)) + ((size_t)1 << log_n) + j) * 8);
    if (!fr_is_zero(a)) atomicOr(&s_any, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_any) atomicOr(upper + v, 1u);
}

// ok[v] = status[v] == 0 && upper[v] == 0; out[v][j] = ok[v] ? Q[v][j] : 0 for j < n; a lane per coefficient, per_poly workgroups per
// polynomial
__global__ void __launch_bounds__(KZGR_BLOCK) k_kzg_rec_finish(const uint4* __restrict__ q, const u32* __restrict__ status, const u32* __restrict__ upper, int log_n, u32 per_poly,
                                                               uint4* __restrict__ out, uint8_t* __restrict__ ok) {
  const size_t v = blockIdx.x / per_poly, j = (size_t)(blockIdx.x % per_poly) * blockDim.x + threadIdx.x;
  if (j >= ((size_t)1 << log_n)) return;
  const bool good = status[v] == 0 && upper[v] == 0;
  if (j == 0) ok[v] = good ? 1 : 0;
  uint4 a = make_uint4(0, 0, 0, 0), b = a;
  if (good) { const uint4* p = q + ((v << (log_n + 1)) + j) * 2; a = p[0]; b = p[1]; }
  uint4* o = out + ((v << log_n) + j) * 2;
  o[0] = a; o[1] = b;
}

}  // namespace bls
