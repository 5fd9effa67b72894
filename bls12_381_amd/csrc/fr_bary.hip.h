// fr_bary.hip.h -- polynomials over Fr held in EVALUATION form: the value at a point outside (or inside) the domain and the quotient
// of the KZG opening, without leaving the Lagrange basis (blsgpu_fr_bary_eval_many* / blsgpu_fr_bary_open_many*).
//
// Row v holds f[i] = p(D[i]) on the domain D of the n-th roots of unity (D[i] = w^i, or w^bitrev(i)), p of degree < n, and has its own
// point z.  With d[i] = z - D[i] and the two sums over the row
//     A = sum f[i] / d[i]        F = sum f[i]
// the barycentric formula  y = (z^n - 1) / n * sum f[i] D[i] / d[i]  becomes, since D / (z - D) = z / (z - D) - 1,
//     y = (z^n - 1) / n * (z A - F)                                  one product per element instead of two
//     q[i] = (y - f[i]) / d[i]
// and for z = D[j] (the "hit"; the sums then leave element j out):  y = f[j],  q[i] as above for i != j, and
//     q[j] = sum_{i != j} (f[i] - y) D[i] / (z d[i]) = sum_{i != j} (f[i] - y) (1 / d[i] - 1 / z) = A - y I - (F - n y) / z
// with I = sum_{i != j} 1 / (D[j] - D[i]) = P''(D[j]) / (2 P'(D[j])) = (n - 1) / (2 z) for P = X^n - 1 (and F - f[j] - (n - 1) y = F - n y):
//     q[j] = A - (F - (n + 1) / 2 * y) / z
// so the hit element needs nothing but the sums the evaluation reduces anyway: no second pass over the row, no second reduction.
// 1 / z = z^(n - 1).  Field addition is exact, so the order of a sum cannot change a limb; it is fixed anyway.
//
// D[i] comes from the forward twiddle table of the transform (fr.hip.h: level log_n - 1 holds 2^5 w^j, j < n / 2; w^(j + n / 2) = -w^j;
// no level at log_n = 0, where D = {1}).  The 2^5 is not divided out per element: d' = 2^5 z - table = 2^5 d, and the ONE inverse a tile
// takes (below) is multiplied by 2^5, which makes every element's inverse 1 / d.
// d' is formed twice per element, in the forward and in the backward sweep of the inversion: two 32-byte table reads (unit stride in
// natural order, a gather in bit-reversed order; the table has n / 2 entries and stays in the caches) instead of eight more registers or
// a second copy of the tile in LDS, which would halve the workgroups per CU.
//
// Schedule (fr_bary_plan.h).  Tiles, LDS layout and the inversion are fr_scan.hip.h's k_frs_invert: a lane keeps the prefix products of
// the d' of its chunk in registers, the lane totals are scanned forward and backward (frs_block_prod_excl), one wavefront inverts the
// tile's total (frs_inv), and the backward sweep leaves 1 / d[i] in the registers while it adds up A and F.  A zero d' is taken as 1
// and remembered as the row's hit.  Then
//   ROWS (n <= tile)  a row is a lane's segment (n <= chunk) or n / chunk whole lanes; the lanes' sums meet in the row's first lane
//                     (shuffles inside a wavefront, LDS across), which writes y and, for a hit row, q[j]; the others turn their
//                     registers into q.  Rows of one workgroup share nothing but the tile's inverse, where a hit contributes a 1.
//   TILE (n > tile)   the workgroup's sums go to the tile's record, 1 / d[i] to q (open); k_frb_row sums a row's records, writes y,
//                     the row record and q[j]; k_frb_quot rewrites q in place and leaves q[j] alone.
// Per element: four products for eval, five for open.  No workgroup waits for another, no atomics.
#pragma once
#include "fr.hip.h"
#include "fr_scan.hip.h"
#include "fr_bary_plan.h"

namespace bls {

static_assert(FRB_CHUNK <= FRS_CHUNK_MAX, "a lane keeps its chunk's inverses in FRS_CHUNK_MAX registers");

struct FrbAgg { Fr a, f; u32 hit; };

DEV Fr frb_x32(Fr a) { for (int k = 0; k < 5; k++) a = fr_add(a, a); return a; }
// a / 2: (a + r) / 2 for an odd a (a + r < 2^256)
DEV Fr frb_half(const Fr& a) {
  const u32 m = 0u - (a.l[0] & 1u);
  Fr t; u64 c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { u64 x = (u64)a.l[i] + (FR_MOD[i] & m) + c; t.l[i] = (u32)x; c = x >> 32; }
#pragma unroll
  for (int i = 0; i < 7; i++) t.l[i] = (t.l[i] >> 1) | (t.l[i + 1] << 31);
  t.l[7] >>= 1;
  return t;
}
// the exponent e of D[i] = w^e
DEV u32 frb_exp(u32 i, int log_n, int order) { return order == FRB_BITREV && log_n ? (u32)(__brevll((unsigned long long)i) >> (64 - log_n)) : i; }
// 2^5 w^e from the forward twiddle table of log_n
DEV Fr frb_dom32(const u32* __restrict__ tw, int log_n, u32 e) {
  if (log_n == 0) return frb_x32(fr_one());
  const u32 half = 1u << (log_n - 1);
  const Fr t = fr_load(tw + (fr_tw_off(log_n - 1) + (e & (half - 1))) * 8);
  return (e & half) ? fr_neg(t) : t;
}
// y of a row whose point is outside the domain
DEVNI Fr frb_y(Fr z, int log_n, Fr a, Fr f) {
  Fr s = z;
#pragma unroll 1
  for (int i = 0; i < log_n; i++) s = frs_mul(s, s);
  s = fr_sub(s, fr_one());
#pragma unroll 1
  for (int i = 0; i < log_n; i++) s = frb_half(s);
  return frs_mul(s, fr_sub(frs_mul(z, a), f));
}
// q[j] of a row whose point is D[j] (y = f[j]; the sums leave j out): A - (F - (n + 1) / 2 * y) / z
DEVNI Fr frb_qhit(Fr z, int log_n, Fr y, Fr a, Fr f) {
  Fr zi = fr_one(), p = z, ny = y;                       // z^(n - 1) = z^(1 + 2 + ... + n / 2)
#pragma unroll 1
  for (int i = 0; i < log_n; i++) { zi = frs_mul(zi, p); p = frs_mul(p, p); ny = fr_add(ny, ny); }
  return fr_sub(a, frs_mul(zi, fr_sub(f, frb_half(fr_add(ny, y)))));
}

DEV FrbAgg frb_wrec_load(const u32* p) { FrbAgg g; g.a = fr_load(p); g.f = fr_load(p + 8); g.hit = p[16]; return g; }
DEV void frb_wrec_store(u32* p, const FrbAgg& g) { fr_store(p, g.a); fr_store(p + 8, g.f); p[16] = g.hit; }
DEV FrbAgg frb_join(const FrbAgg& x, const FrbAgg& y) {
  FrbAgg g;
  g.a = fr_add(x.a, y.a); g.f = fr_add(x.f, y.f);
  g.hit = x.hit > y.hit ? x.hit : y.hit;                 // at most one element of a row is hit
  return g;
}
// The sums of the `lanes` consecutive lanes (a power of two; the group starts at a multiple of it) the caller belongs to; the result is
// valid in the group's FIRST lane only.  Every lane of the workgroup calls it.  wrec: FRB_WREC_WORDS per wavefront, free again on return.
DEV FrbAgg frb_group_sum(FrbAgg g, unsigned lanes, u32* wrec) {
#pragma unroll 1
  for (unsigned d = 1; d < lanes && d < 64; d <<= 1) {
    FrbAgg o;
    o.a = frs_shfl(g.a, d, true); o.f = frs_shfl(g.f, d, true);
    o.hit = (u32)__shfl_down((int)g.hit, d);
    g = frb_join(g, o);
  }
  if (lanes > 64) {
    const unsigned w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) frb_wrec_store(wrec + w * FRB_WREC_WORDS, g);
    __syncthreads();
    if (threadIdx.x % lanes == 0)
#pragma unroll 1
      for (unsigned i = 1; i < lanes / 64; i++) g = frb_join(g, frb_wrec_load(wrec + (w + i) * FRB_WREC_WORDS));
    __syncthreads();
  }
  return g;
}

// ---- a tile of evaluations ----------------------------------------------------------------------------------------------------------
// mode FRB_K_ROWS (n <= tile): the tile holds whole rows; y (and q) are final.  mode FRB_K_TILE (n > tile): the tile is a piece of one
// row; its sums go to rec[blockIdx.x] and, for OPEN, 1 / d[i] to q.  q overlaps neither evals nor points nor y (the entry points refuse).
template <bool OPEN>
__global__ void __launch_bounds__(FRB_BLOCK, 2) k_frb_tile(int mode, const u32* __restrict__ evals, const u32* __restrict__ points, const u32* __restrict__ tw, int log_n,
                                                           size_t k, int order, unsigned chunk, u32* y, u32* __restrict__ q, u32* __restrict__ rec) {
  BLS_DYN_LDS(lds);
  const size_t n = (size_t)1 << log_n, total = k << log_n;
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= total) return;
  const unsigned cnt = total - base < (size_t)tile ? (unsigned)(total - base) : tile;
  u32* ybuf = lds + blockDim.x * (chunk * 8 + 4);
  u32* wrec = ybuf + blockDim.x * 8;
  frs_tile_load<false>(evals, base, cnt, total, chunk, lds);
  __syncthreads();
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;      // 0 or whole segments: cnt is a multiple of min(n, chunk)
  const unsigned seg = n < chunk ? (unsigned)n : chunk;                             // elements of one row in a lane's chunk
  const unsigned lanes = n <= chunk ? 1u : mode == FRB_K_TILE ? blockDim.x : (unsigned)(n / chunk);      // lanes whose sums meet
  const size_t g0 = base + s0;
  // forward: prefix products of d' = 2^5 (z - D[i]), a zero taken as 1
  Fr c[FRS_CHUNK_MAX];
  Fr prod = fr_one(), z32 = fr_zero();
  u32 hitmask = 0;
#pragma unroll
  for (int j = 0; j < FRS_CHUNK_MAX; j++) {
    if ((unsigned)j < mine) {
      const size_t g = g0 + j;
      if (((unsigned)j & (seg - 1)) == 0) z32 = frb_x32(fr_load(points + (g >> log_n) * 8));
      Fr d = fr_sub(z32, frb_dom32(tw, log_n, frb_exp((u32)(g & (n - 1)), log_n, order)));
      if (fr_is_zero(d)) { d = fr_one(); hitmask |= 1u << j; }
      prod = j ? frs_mul(prod, d) : d;
    }
    c[j] = prod;
  }
  const Fr before = frs_block_prod_excl<false>(prod, wrec);
  const Fr after = frs_block_prod_excl<true>(prod, wrec);
  if (threadIdx.x < 64) {                              // one wavefront inverts the tile's total; times 2^5: every element's inverse is 1 / d
    const Fr inv = frb_x32(frs_inv(frs_mul(frs_mul(before, prod), after)));
    if (threadIdx.x == 0) fr_store(wrec, inv);
  }
  __syncthreads();
  Fr r = frs_mul(frs_mul(fr_load(wrec), before), after);
  __syncthreads();                                     // wrec is written again below
  // backward: c[j] = 1 / d[j]; the sums of a segment are complete at its first element
  FrbAgg g;
  g.a = g.f = fr_zero(); g.hit = 0;
#pragma unroll
  for (int j = FRS_CHUNK_MAX - 1; j >= 0; j--) {
    if ((unsigned)j < mine) {
      const size_t gi = g0 + j, row = gi >> log_n;
      const u32 i = (u32)(gi & (n - 1));
      if ((((unsigned)j + 1) & (seg - 1)) == 0) z32 = frb_x32(fr_load(points + row * 8));
      const bool hit = (hitmask >> j) & 1u;
      const Fr d = hit ? fr_one() : fr_sub(z32, frb_dom32(tw, log_n, frb_exp(i, log_n, order)));
      const Fr o = j ? frs_mul(c[j ? j - 1 : 0], r) : r;
      r = frs_mul(r, d);
      c[j] = o;
      const Fr f = fr_load(lds + frs_lds_addr(s0 + j, chunk));
      g.f = fr_add(g.f, f);
      if (hit) g.hit = i + 1;
      else g.a = fr_add(g.a, frs_mul(f, o));
      if (lanes == 1 && ((unsigned)j & (seg - 1)) == 0) {          // a row inside this lane: finished here
        const Fr z = fr_load(points + row * 8);
        const Fr yv = g.hit ? fr_load(lds + frs_lds_addr(s0 + j + g.hit - 1, chunk)) : frb_y(z, log_n, g.a, g.f);
        fr_store(y + row * 8, yv);
        // the lane owns the slot, and f[j] has been read: the pass below skips it
        if (OPEN && g.hit) fr_store(lds + frs_lds_addr(s0 + j + g.hit - 1, chunk), frb_qhit(z, log_n, yv, g.a, g.f));
        g.a = g.f = fr_zero(); g.hit = 0;
      }
    }
  }
  Fr yv = fr_zero();
  if (lanes > 1) {
    g = frb_group_sum(g, lanes, wrec);
    const bool lead = threadIdx.x % lanes == 0 && mine;
    // the slot of the hit element: the leader's first element is element (g0 & (n - 1)) of the row
    const unsigned hslot = g.hit ? s0 + (g.hit - 1) - (u32)(g0 & (n - 1)) : 0u;
    if (mode == FRB_K_TILE) {
      if (lead) {
        u32* p = rec + (size_t)blockIdx.x * FRB_REC_WORDS;
        fr_store(p, g.a); fr_store(p + 8, g.f);
        fr_store(p + 16, g.hit ? fr_load(lds + frs_lds_addr(hslot, chunk)) : fr_zero());
        *reinterpret_cast<uint4*>(p + 24) = make_uint4(g.hit, 0, 0, 0);
      }
      if (!OPEN) return;
      __syncthreads();                                 // the leader has read f[j]
#pragma unroll
      for (int j = 0; j < FRS_CHUNK_MAX; j++)
        if ((unsigned)j < mine) fr_store(lds + frs_lds_addr(s0 + j, chunk), c[j]);
      __syncthreads();
      frs_tile_store<false>(q, base, cnt, total, chunk, lds);
      return;
    }
    Fr qj = fr_zero();
    if (lead) {
      const Fr z = fr_load(points + (g0 >> log_n) * 8);
      yv = g.hit ? fr_load(lds + frs_lds_addr(hslot, chunk)) : frb_y(z, log_n, g.a, g.f);
      fr_store(y + (g0 >> log_n) * 8, yv);
      fr_store(ybuf + threadIdx.x * 8, yv);
      if (OPEN && g.hit) qj = frb_qhit(z, log_n, yv, g.a, g.f);
    }
    if (!OPEN) return;
    __syncthreads();                                   // y is in ybuf, f[j] has been read
    yv = fr_load(ybuf + (threadIdx.x - threadIdx.x % lanes) * 8);
    if (lead && g.hit) fr_store(lds + frs_lds_addr(hslot, chunk), qj);      // its owner skips the slot below
  }
  if (!OPEN) return;
  // q[i] = (y - f[i]) / d[i] in place of f[i]; a hit element already holds its q
#pragma unroll
  for (int j = 0; j < FRS_CHUNK_MAX; j++) {
    if ((unsigned)j < mine && lanes == 1 && ((unsigned)j & (seg - 1)) == 0) yv = fr_load(y + ((g0 + j) >> log_n) * 8);      // this lane's own store above
    if ((unsigned)j < mine && !((hitmask >> j) & 1u)) {
      u32* slot = lds + frs_lds_addr(s0 + j, chunk);
      fr_store(slot, frs_mul(fr_sub(yv, fr_load(slot)), c[j]));
    }
  }
  __syncthreads();
  frs_tile_store<false>(q, base, cnt, total, chunk, lds);
}

// ---- a row of tile records (n > tile) -------------------------------------------------------------------------------------------------
// One workgroup per row: sums the row's `tpr` records, writes y[row], the row record and, for OPEN, q[j] of a hit row.
template <bool OPEN>
__global__ void __launch_bounds__(FRB_BLOCK) k_frb_row(const u32* __restrict__ rec, size_t tpr, unsigned tile, const u32* __restrict__ points, int log_n, size_t k,
                                                        u32* __restrict__ y, u32* __restrict__ q, u32* __restrict__ rowrec) {
  BLS_DYN_LDS(wrec);
  const size_t row = blockIdx.x;
  if (row >= k) return;
  const u32* mine = rec + row * tpr * FRB_REC_WORDS;
  FrbAgg g;
  g.a = g.f = fr_zero(); g.hit = 0;
#pragma unroll 1
  for (size_t t = threadIdx.x; t < tpr; t += blockDim.x) {
    FrbAgg o = frb_wrec_load(mine + t * FRB_REC_WORDS);
    o.hit = mine[t * FRB_REC_WORDS + 24];
    g = frb_join(g, o);
  }
  g = frb_group_sum(g, blockDim.x, wrec);
  if (threadIdx.x) return;
  const Fr z = fr_load(points + row * 8);
  const Fr yv = g.hit ? fr_load(mine + (size_t)((g.hit - 1) / tile) * FRB_REC_WORDS + 16) : frb_y(z, log_n, g.a, g.f);
  fr_store(y + row * 8, yv);
  fr_store(rowrec + row * FRB_ROWREC_WORDS, yv);
  *reinterpret_cast<uint4*>(rowrec + row * FRB_ROWREC_WORDS + 8) = make_uint4(g.hit, 0, 0, 0);
  if (OPEN && g.hit) fr_store(q + ((row << log_n) + (g.hit - 1)) * 8, frb_qhit(z, log_n, yv, g.a, g.f));
}

// ---- the quotient of a row over tiles: q[i] = (y - f[i]) * q[i], where k_frb_tile left 1 / d[i]; q[j] of a hit row is k_frb_row's ----------
__global__ void __launch_bounds__(FRB_BLOCK) k_frb_quot(const u32* __restrict__ evals, const u32* __restrict__ rowrec, int log_n, size_t k, unsigned chunk, u32* __restrict__ q) {
  const size_t n = (size_t)1 << log_n, total = k << log_n;
  const size_t base = (size_t)blockIdx.x * blockDim.x * chunk;
  if (base >= total) return;
  const u32* rr = rowrec + (base >> log_n) * FRB_ROWREC_WORDS;      // uniform: a tile lies in one row
  const Fr yv = fr_load(rr);
  const u32 hit = rr[8];
#pragma unroll 1
  for (unsigned m = 0; m < chunk; m++) {
    const size_t g = base + (size_t)m * blockDim.x + threadIdx.x;
    if (g >= total || (u32)(g & (n - 1)) + 1 == hit) continue;
    fr_store(q + g * 8, frs_mul(fr_sub(yv, fr_load(evals + g * 8)), fr_load(q + g * 8)));
  }
}

}  // namespace bls
