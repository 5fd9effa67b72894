// fr_scan.hip.h -- recurrences ALONG a vector of Fr elements: segmented prefix sums, prefix products and Horner rows
// (blsgpu_fr_scan_many*), and the inversion of a whole vector by Montgomery's trick (blsgpu_fr_batch_invert*).
//
// The arithmetic is scalar.hip.h's (fr_add / fr_mul: scalar.rs:435-503, restated there); what is here is the schedule.  The k x len
// array is one flat sequence with segment heads at the multiples of len, cut into tiles of blockDim.x lanes x `chunk` consecutive
// elements, and scanned reduce-then-scan in separate launches (fr_scan_plan.h): per-tile aggregates, a scan of the aggregates by one
// workgroup (through a second level of aggregates when there are more than a tile of them), a pass that rescans each lane's chunk from
// the tile's carry-in and the lane's own prefix inside the tile, which the first pass left behind.  No workgroup ever waits for another
// one: no look-back, no flag polling, no grid barrier -- the stream orders the passes.
//
// The monoid.  A piece of the sequence is (value, multiplier, crossed-a-head flag).  `l` followed by `r` is `r` alone when r holds a
// head, and otherwise
//     SUM      l.v + r.v                 PRODUCT  l.v * r.v                 HORNER  (r.p * l.p,  r.v + r.p * l.v)
// HORNER runs from the top of each row downward, so its kernels see the flat sequence REVERSED (logical index g = total - 1 - physical
// index; heads are again the multiples of len) and element c of a row with point z is the affine map h -> c + z h.  The multiplier
// p = z^(elements of the piece) is carried as the generic affine pair rather than read from per-row tables of z^(chunk 2^s), z^tile:
//   * in the cross-lane steps both cost the same two products (p * p and p * v against squaring the table power and power * v);
//   * the inclusive scan of lane t covers t + 1 chunks, not a power of two, so applying a carry to it needs z^(chunk (t + 1)) anyway --
//     the pair has it, a table would need a per-lane exponentiation;
//   * rows may be one element long: tables for 2^28 rows would be several times the data, while the pair only widens the records --
//     "twice the traffic" applies to the aggregates (80-byte records instead of 48-byte ones, one per tile and one per lane chunk), never to the elements;
//   * the flag makes whatever p a piece with a head carries irrelevant, so nothing is special-cased at a row boundary.
// A carry (what precedes a tile in its row) is a value alone: applying it never needs the left piece's multiplier.
//
// Data movement.  A tile is loaded with 16-byte words, consecutive lanes on consecutive words, into LDS; a lane then walks ITS chunk
// there.  LDS layout: eight words per element and FOUR words of padding per lane chunk (frs_lds_addr), not the nine-word pitch of
// k_fr_tile: that pitch is right when consecutive lanes take consecutive elements, but here lane t starts at element t * chunk, and with
// chunk = 8 a nine-word pitch puts lanes t and t + 8 on the same bank (72 t mod 64).  Padding by 4 keeps every element 16-byte aligned
// (one ds_read_b128 / ds_write_b128 per half element) and makes the lane stride 68 words: 16 consecutive lanes cover the 64 banks once.
// 2048 elements: 68 KB + the wavefront records, two workgroups per CU (__launch_bounds__(256, 2): two wavefronts per SIMD).
//
// Per lane: a serial pass over its chunk, a Hillis-Steele scan of the 64 lane aggregates with __shfl_up, the wavefront totals through
// LDS.  Products on these paths go through ONE out-of-line copy of fr_mul (frs_mul): the kernels are a few dozen call sites, and the
// inlined product is ~500 instructions.
//
// Batch inversion (k_frs_invert), same tiles, ONE launch: zeros are replaced by 1, a lane keeps the prefix products of its chunk in
// registers, the lane totals are scanned forward and backward, ONE inversion per tile gives 1 / (tile total), every lane derives the
// inverse of its own chunk total (inv_total * before * after) and sweeps its chunk backward: out_j = prefix_(j-1) * r, r *= x_j.  Three
// products per element plus the two scans.  The tile's inversion is on every workgroup's critical path with one wavefront busy, so it is
// NOT fr_inv (a^(r-2): 380 dependent products, several times the rest of the tile's work) but Kaliski's almost-inverse (frs_inv: at most
// 510 steps of 8-word shifts, additions and subtractions, then ten products); it returns the same canonical element, so the outputs are
// limb-identical to blsgpu_fr_op op 4.
#pragma once
#include "scalar.hip.h"
#include "fr_scan_plan.h"

namespace bls {

struct FrsAgg { Fr v, p; u32 f; };

DEVNI Fr frs_mul(Fr a, Fr b) { return fr_mul(a, b); }

template <int OP> DEV FrsAgg frs_identity() {
  FrsAgg a;
  a.v = OP == FRS_PRODUCT ? fr_one() : fr_zero();
  a.p = fr_one();
  a.f = 0;
  return a;
}
// one element x after the running value acc (same row); z: the row's point (HORNER)
template <int OP> DEV Fr frs_step(const Fr& acc, const Fr& x, const Fr& z) {
  if (OP == FRS_SUM) return fr_add(acc, x);
  if (OP == FRS_PRODUCT) return frs_mul(acc, x);
  return fr_add(x, frs_mul(z, acc));
}
// the value after the piece r, given the value lv before it (r holds no head)
template <int OP> DEV Fr frs_apply(const Fr& lv, const FrsAgg& r) {
  if (OP == FRS_SUM) return fr_add(lv, r.v);
  if (OP == FRS_PRODUCT) return frs_mul(lv, r.v);
  return fr_add(r.v, frs_mul(r.p, lv));
}
template <int OP> DEV Fr frs_carry(const Fr& lv, const FrsAgg& r) { return r.f ? r.v : frs_apply<OP>(lv, r); }
// l followed by r
template <int OP> DEV FrsAgg frs_combine(const FrsAgg& l, const FrsAgg& r) {
  if (r.f) return r;
  FrsAgg o;
  o.v = frs_apply<OP>(l.v, r);
  o.p = OP == FRS_HORNER ? frs_mul(r.p, l.p) : r.p;
  o.f = l.f;
  return o;
}
template <int OP> DEV FrsAgg frs_shfl_up(const FrsAgg& a, unsigned d) {
  FrsAgg o;
#pragma unroll
  for (int i = 0; i < 8; i++) o.v.l[i] = (u32)__shfl_up((int)a.v.l[i], d);
  if (OP == FRS_HORNER) {
#pragma unroll
    for (int i = 0; i < 8; i++) o.p.l[i] = (u32)__shfl_up((int)a.p.l[i], d);
  } else o.p = a.p;
  o.f = (u32)__shfl_up((int)a.f, d);
  return o;
}
// a record of frs_rec_words(OP) words: the multiplier is stored for HORNER only (nothing else reads it)
template <int OP> DEV FrsAgg frs_rec_load(const u32* p) {
  FrsAgg a;
  a.v = fr_load(p);
  if (OP == FRS_HORNER) { a.p = fr_load(p + 8); a.f = p[16]; }
  else { a.p = fr_one(); a.f = p[8]; }
  return a;
}
template <int OP> DEV void frs_rec_store(u32* p, const FrsAgg& a) {
  fr_store(p, a.v);
  if (OP == FRS_HORNER) fr_store(p + 8, a.p);
  *reinterpret_cast<uint4*>(p + (OP == FRS_HORNER ? 16 : 8)) = make_uint4(a.f, 0, 0, 0);
}

// The lanes of a workgroup (whole wavefronts) each hold the aggregate `a` of their chunk, in lane order.  Returns the aggregate of
// everything BEFORE the lane's chunk (the identity for lane 0); followed by `a` it is the aggregate up to and including the chunk.
// wrec: one record per wavefront in LDS, free again on return.
template <int OP> DEV FrsAgg frs_block_scan(FrsAgg a, u32* wrec) {
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll 1
  for (unsigned d = 1; d < 64; d <<= 1) {
    const FrsAgg o = frs_shfl_up<OP>(a, d);
    if (lane >= d) a = frs_combine<OP>(o, a);
  }
  if (lane == 63) frs_rec_store<OP>(wrec + w * FRS_REC_WORDS, a);
  __syncthreads();
  FrsAgg before = frs_identity<OP>();                 // the wavefronts before this one
#pragma unroll 1
  for (unsigned i = 0; i < w; i++) before = frs_combine<OP>(before, frs_rec_load<OP>(wrec + i * FRS_REC_WORDS));
  const FrsAgg prev = frs_shfl_up<OP>(a, 1);
  const FrsAgg r = lane ? frs_combine<OP>(before, prev) : before;
  __syncthreads();
  return r;
}

// word offset in LDS of slot s of a tile: eight words per element, four words of padding per lane chunk
DEV unsigned frs_lds_addr(unsigned s, unsigned chunk) { return s * 8 + (s / chunk) * 4; }
// slots [0, cnt) of the tile = logical elements [base, base + cnt) of the flat sequence of `total` elements; REV: logical g is physical
// total - 1 - g.  16-byte words, consecutive lanes on consecutive words of the (contiguous) physical range.
template <bool REV> DEV void frs_tile_load(const u32* in, size_t base, unsigned cnt, size_t total, unsigned chunk, u32* lds) {
  const uint4* src = reinterpret_cast<const uint4*>(in) + 2 * (REV ? total - base - cnt : base);
  for (unsigned i = threadIdx.x; i < 2 * cnt; i += blockDim.x) {
    const unsigned e = i >> 1, s = REV ? cnt - 1 - e : e;
    *reinterpret_cast<uint4*>(lds + frs_lds_addr(s, chunk) + (i & 1u) * 4) = src[i];
  }
}
template <bool REV> DEV void frs_tile_store(u32* out, size_t base, unsigned cnt, size_t total, unsigned chunk, const u32* lds) {
  uint4* dst = reinterpret_cast<uint4*>(out) + 2 * (REV ? total - base - cnt : base);
  for (unsigned i = threadIdx.x; i < 2 * cnt; i += blockDim.x) {
    const unsigned e = i >> 1, s = REV ? cnt - 1 - e : e;
    dst[i] = *reinterpret_cast<const uint4*>(lds + frs_lds_addr(s, chunk) + (i & 1u) * 4);
  }
}

// ---- a tile of elements -----------------------------------------------------------------------------------------------------------
// mode FRS_K_SINGLE: the whole call is this tile (carry-in = the identity); FRS_K_REDUCE: write the tile's aggregate record to
// agg_out[blockIdx.x] AND, for every lane, the aggregate of what precedes its chunk inside the tile to lane_rec[global lane]; FRS_K_SCAN:
// read that record back, put carry_in[blockIdx.x] (eight words: the value that precedes the tile in its row) in front of it and rescan
// the chunk.  The lane records are what keeps the scan pass at one product per element: without them it would repeat the reduce pass's
// serial pass and cross-lane scan -- they cost 48 bytes (HORNER: 80) per `chunk` elements of traffic each way, which these kernels,
// bound by their products and not by HBM, have to spare.
// `in` and `out` may be the same buffer: a workgroup has its whole tile in LDS before its first store and touches no other tile.
// points: k scalars, the point of physical row v at points + 8 v (HORNER only).
// The tile's elements are in LDS (frs_lds_addr; every lane sees its own chunk): the part of k_frs_tile between its load and its store,
// shared with the fused front of fr_frac.hip.h, whose tile is built in LDS instead of loaded.  SINGLE and SCAN leave the scanned tile in
// LDS (the caller stores it after a barrier), REDUCE leaves the elements as they were and writes the records.
template <int OP>
DEV void frs_tile_body(int mode, int exclusive, u32* lds, u32* wrec, const u32* __restrict__ points, size_t len, size_t k, unsigned chunk, size_t base, unsigned cnt,
                       u32* __restrict__ agg_out, const u32* __restrict__ carry_in, u32* lane_rec) {
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;
  const size_t row0 = mine ? (base + s0) / len : 0;                // logical row of the lane's first element, and its position in it
  const size_t pos0 = mine ? (base + s0) - row0 * len : 0;
  Fr z = fr_zero();
  u32* my_rec = mode == FRS_K_SINGLE ? nullptr : lane_rec + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * frs_rec_words(OP);
  // the lane's aggregate
  FrsAgg a = frs_identity<OP>();
  if (mode != FRS_K_SCAN) {
    size_t q = pos0, row = row0;
    if (OP == FRS_HORNER && mine) z = fr_load(points + (k - 1 - row) * 8);
#pragma unroll 1
    for (unsigned j = 0; j < mine; j++) {
      const Fr x = fr_load(lds + frs_lds_addr(s0 + j, chunk));
      if (q == 0) {
        if (OP == FRS_HORNER && j) z = fr_load(points + (k - 1 - row) * 8);
        a.v = x; a.p = fr_one(); a.f = 1;
      } else {
        a.v = frs_step<OP>(a.v, x, z);
        if (OP == FRS_HORNER) a.p = frs_mul(a.p, z);
      }
      if (++q == len) { q = 0; row++; }
    }
  }
  if (mode == FRS_K_REDUCE) {
    const FrsAgg before = frs_block_scan<OP>(a, wrec);
    frs_rec_store<OP>(my_rec, before);
    if (threadIdx.x >> 6 == (blockDim.x >> 6) - 1) {             // the last wavefront: its last lane holds the tile's aggregate
      const FrsAgg t = frs_combine<OP>(before, a);
      if (threadIdx.x == blockDim.x - 1) frs_rec_store<OP>(agg_out + (size_t)blockIdx.x * frs_rec_words(OP), t);
    }
    return;
  }
  Fr acc;
  if (mode == FRS_K_SCAN) acc = frs_carry<OP>(fr_load(carry_in + (size_t)blockIdx.x * 8), frs_rec_load<OP>(my_rec));
  else acc = frs_block_scan<OP>(a, wrec).v;
  {
    size_t q = pos0, row = row0;
    if (OP == FRS_HORNER && mine) z = fr_load(points + (k - 1 - row) * 8);
#pragma unroll 1
    for (unsigned j = 0; j < mine; j++) {
      u32* slot = lds + frs_lds_addr(s0 + j, chunk);
      const Fr x = fr_load(slot);
      Fr prior = acc;
      if (q == 0) {
        if (OP == FRS_HORNER && j) z = fr_load(points + (k - 1 - row) * 8);
        prior = frs_identity<OP>().v;
        acc = x;
      } else acc = frs_step<OP>(acc, x, z);
      fr_store(slot, exclusive ? prior : acc);
      if (++q == len) { q = 0; row++; }
    }
  }
}
template <int OP>
__global__ void __launch_bounds__(FRS_BLOCK, 2) k_frs_tile(int mode, int exclusive, const u32* in, u32* out, const u32* __restrict__ points, size_t len, size_t k, unsigned chunk,
                                                           u32* __restrict__ agg_out, const u32* __restrict__ carry_in, u32* lane_rec) {
  BLS_DYN_LDS(lds);
  constexpr bool REV = OP == FRS_HORNER;
  const size_t total = len * k;
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= total) return;
  const unsigned cnt = total - base < (size_t)tile ? (unsigned)(total - base) : tile;
  u32* wrec = lds + blockDim.x * (chunk * 8 + 4);
  frs_tile_load<REV>(in, base, cnt, total, chunk, lds);
  __syncthreads();
  frs_tile_body<OP>(mode, exclusive, lds, wrec, points, len, k, chunk, base, cnt, agg_out, carry_in, lane_rec);
  if (mode == FRS_K_REDUCE) return;
  __syncthreads();
  frs_tile_store<REV>(out, base, cnt, total, chunk, lds);
}

// ---- a tile of aggregate records --------------------------------------------------------------------------------------------------
// n records at `agg`; a workgroup takes blockDim.x * chunk consecutive ones, a lane `chunk` of them.  mode FRS_K_AGG_REDUCE: the
// aggregate of the workgroup's records to agg_out[blockIdx.x]; FRS_K_AGG_SCAN: carry_out[i] (eight words) = the value that precedes
// record i in its row, starting from carry_in[blockIdx.x] (NULL: nothing precedes the workgroup's first record).
template <int OP>
__global__ void __launch_bounds__(FRS_BLOCK) k_frs_agg(int mode, const u32* __restrict__ agg, size_t n, unsigned chunk, u32* __restrict__ agg_out,
                                                        const u32* __restrict__ carry_in, u32* __restrict__ carry_out) {
  BLS_DYN_LDS(wrec);
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= n) return;
  const unsigned cnt = n - base < (size_t)tile ? (unsigned)(n - base) : tile;
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;
  const u32* my = agg + (base + s0) * frs_rec_words(OP);
  FrsAgg a = frs_identity<OP>();
#pragma unroll 1
  for (unsigned j = 0; j < mine; j++) a = frs_combine<OP>(a, frs_rec_load<OP>(my + (size_t)j * frs_rec_words(OP)));
  const FrsAgg before = frs_block_scan<OP>(a, wrec);
  if (mode == FRS_K_AGG_REDUCE) {
    if (threadIdx.x == blockDim.x - 1) frs_rec_store<OP>(agg_out + (size_t)blockIdx.x * frs_rec_words(OP), frs_combine<OP>(before, a));
    return;
  }
  Fr acc = before.v;
  if (carry_in) acc = frs_carry<OP>(fr_load(carry_in + (size_t)blockIdx.x * 8), before);
#pragma unroll 1
  for (unsigned j = 0; j < mine; j++) {
    fr_store(carry_out + (base + s0 + j) * 8, acc);
    acc = frs_carry<OP>(acc, frs_rec_load<OP>(my + (size_t)j * frs_rec_words(OP)));
  }
}

// ---- batch inversion --------------------------------------------------------------------------------------------------------------
// a^-1 for a canonical non-zero Montgomery element: Kaliski's almost-inverse on the limbs, then one product.  With a' = a R (the
// limbs as an integer), phase 1 keeps  a' r = -u 2^k,  a' s = v 2^k  (mod p; p = the modulus r of the field) while it halves and
// subtracts (u, v) = (p, a') down to v = 0, doubling r or s at every step: only 8-word shifts, additions and subtractions, r, s < 2p <
// 2^256, and at most 2 * 255 steps (every step halves u or v).  It ends with p - r = a'^-1 2^k, 255 <= k <= 510, and
//   a^-1 R = a'^-1 R^2 = (p - r) * 2^(768 - k) / R,
// one Montgomery product with 2^(768 - k) = the Montgomery form of 2^(512 - k), built by square-and-double from the top bit.  About a
// quarter of the instructions of the binary Euclid with modular halvings, a tenth of a^(p-2).  The step bound also ends the loop for an
// input that is 0 mod p (limbs >= p: unspecified result, but no endless loop).  All lanes of a wavefront call it with the same value.
DEV void frs_shr1(u32* a) { for (int i = 0; i < 7; i++) a[i] = (a[i] >> 1) | (a[i + 1] << 31); a[7] >>= 1; }
DEV void frs_shl1(u32* a) { for (int i = 7; i > 0; i--) a[i] = (a[i] << 1) | (a[i - 1] >> 31); a[0] <<= 1; }
DEV void frs_add_words(u32* a, const u32* b) { u64 c = 0; for (int i = 0; i < 8; i++) { u64 x = (u64)a[i] + b[i] + c; a[i] = (u32)x; c = x >> 32; } }
// d = a - b; returns the borrow (1 if a < b)
DEV u32 frs_sub_words(u32* d, const u32* a, const u32* b) {
  int64_t br = 0;
  for (int i = 0; i < 8; i++) { int64_t x = (int64_t)a[i] - b[i] + br; d[i] = (u32)x; br = x >> 32; }
  return (u32)br & 1u;
}
DEVNI Fr frs_inv(Fr a) {
  u32 u[8], v[8], r[8], s[8], d[8];
  for (int i = 0; i < 8; i++) { u[i] = FR_MOD[i]; v[i] = a.l[i]; r[i] = 0; s[i] = 0; }
  s[0] = 1;
  int k = 0;
#pragma unroll 1
  for (; k < 520; k++) {
    u32 nz = 0;
    for (int i = 0; i < 8; i++) nz |= v[i];
    if (!nz) break;
    if (!(u[0] & 1u)) { frs_shr1(u); frs_shl1(s); }
    else if (!(v[0] & 1u)) { frs_shr1(v); frs_shl1(r); }
    else if (!frs_sub_words(d, u, v)) {                     // u >= v (u == v only at u = v = 1: then v becomes 0 below)
      u32 dz = 0;
      for (int i = 0; i < 8; i++) dz |= d[i];
      if (dz) { for (int i = 0; i < 8; i++) u[i] = d[i]; frs_shr1(u); frs_add_words(r, s); frs_shl1(s); }
      else { for (int i = 0; i < 8; i++) v[i] = 0; frs_add_words(s, r); frs_shl1(r); }
    } else { frs_sub_words(v, v, u); frs_shr1(v); frs_add_words(s, r); frs_shl1(r); }
  }
  Fr x;                                                    // p - (r mod p) = a'^-1 2^k
  if (!frs_sub_words(d, r, FR_MOD)) for (int i = 0; i < 8; i++) r[i] = d[i];
  frs_sub_words(x.l, FR_MOD, r);
  const int e = 512 - k;                                   // in [2, 257] for a valid input
  Fr c = fr_one();                                         // the Montgomery form of 2^e
#pragma unroll 1
  for (int i = 8; i >= 0; i--) { c = frs_mul(c, c); if (e > 0 && ((e >> i) & 1)) c = fr_add(c, c); }
  return frs_mul(x, c);
}

DEV Fr frs_shfl(const Fr& a, unsigned d, bool down) {
  Fr o;
#pragma unroll
  for (int i = 0; i < 8; i++) o.l[i] = (u32)(down ? __shfl_down((int)a.l[i], d) : __shfl_up((int)a.l[i], d));
  return o;
}
// the product of the lane values `a` of all lanes before (REV: after) this one in the workgroup; wrec: 8 words per wavefront
template <bool REV> DEV Fr frs_block_prod_excl(Fr a, u32* wrec) {
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll 1
  for (unsigned d = 1; d < 64; d <<= 1) {
    const Fr o = frs_shfl(a, d, REV);
    if (REV ? lane + d < 64 : lane >= d) a = frs_mul(o, a);
  }
  if (lane == (REV ? 0u : 63u)) fr_store(wrec + w * 8, a);
  __syncthreads();
  Fr other = fr_one();
#pragma unroll 1
  for (unsigned i = REV ? w + 1 : 0; i < (REV ? nw : w); i++) other = frs_mul(other, fr_load(wrec + i * 8));
  const Fr next = frs_shfl(a, 1, REV);
  const Fr r = lane == (REV ? 63u : 0u) ? other : frs_mul(other, next);
  __syncthreads();
  return r;
}
// out[i] = in[i]^-1, 0 for a zero (flags[i] = 0 there, 1 elsewhere; flags may be NULL).  One tile of blockDim.x * chunk elements per
// workgroup, chunk <= FRS_CHUNK_MAX; in == out allowed (as k_frs_tile).
__global__ void __launch_bounds__(FRS_BLOCK, 2) k_frs_invert(const u32* in, u32* out, uint8_t* __restrict__ flags, size_t n, unsigned chunk) {
  BLS_DYN_LDS(lds);
  const unsigned tile = blockDim.x * chunk;
  const size_t base = (size_t)blockIdx.x * tile;
  if (base >= n) return;
  const unsigned cnt = n - base < (size_t)tile ? (unsigned)(n - base) : tile;
  u32* wrec = lds + blockDim.x * (chunk * 8 + 4);
  frs_tile_load<false>(in, base, cnt, n, chunk, lds);
  __syncthreads();
  const unsigned s0 = threadIdx.x * chunk;
  const unsigned mine = s0 < cnt ? (cnt - s0 < chunk ? cnt - s0 : chunk) : 0u;
  Fr c[FRS_CHUNK_MAX];                                 // c[j] = x_0 ... x_j of the lane's chunk, zeros taken as 1
  Fr prod = fr_one();
#pragma unroll
  for (int j = 0; j < FRS_CHUNK_MAX; j++) {
    if ((unsigned)j < mine) {
      Fr x = fr_load(lds + frs_lds_addr(s0 + j, chunk));
      if (fr_is_zero(x)) x = fr_one();
      prod = j ? frs_mul(prod, x) : x;
    }
    c[j] = prod;
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
  for (int j = FRS_CHUNK_MAX - 1; j >= 0; j--) {
    if ((unsigned)j < mine) {
      u32* slot = lds + frs_lds_addr(s0 + j, chunk);
      Fr x = fr_load(slot);
      const bool zero = fr_is_zero(x);
      if (zero) x = fr_one();
      const Fr o = j ? frs_mul(c[j ? j - 1 : 0], r) : r;
      r = frs_mul(r, x);
      fr_store(slot, zero ? fr_zero() : o);
      if (flags) flags[base + s0 + j] = zero ? 0 : 1;
    }
  }
  __syncthreads();
  frs_tile_store<false>(out, base, cnt, n, chunk, lds);
}

}  // namespace bls
