// fr_edwards.hip.h -- twisted Edwards groups  a x^2 + y^2 = 1 + d x^2 y^2  over Fr (blsgpu_fr_edwards_*): curve checks, batch
// normalisation, batched variable-base products, fixed-base tables and segmented fixed-base MSMs.  Jubjub and Bandersnatch are such
// curves; the constants are the caller's (fr_edwards_plan.h has the definition, the recoding, the table layout and the plans).
//
// Arithmetic: the 8 x 32-bit Montgomery product of scalar.hip.h (fr_mul), NOT the 9 x 29-bit lazy limbs of fr.hip.h.  The lazy form
// pays when long runs of products meet few additions (the Poseidon rounds, the butterflies).  A point addition is the opposite: ten
// products between a dozen additions and subtractions whose operands feed the next products on both sides, so every value would need a
// tracked bound and most differences a reduction before the next product (the column bound sum A_a A_b <= 6 leaves no room for a
// difference of sums times a sum), and the comparisons of `check`, the Z = 0 test and the limb-exact outputs want canonical values
// anyway.  With fr_mul every value is canonical between operations and the completeness of the formulas is the whole correctness
// argument.  That the lazy form would have been faster here is possible and NOT measured.
//
// Coordinates: extended (X : Y : Z : T), T = X Y / Z.  ed_add is the unified addition (Hisil, Wong, Carter, Dawson 2008, section 3.1:
// 9 products + one by a + one by d), ed_add_mixed the same against a table entry (x, y, d x y) (7 products + one by a), ed_dbl the
// dedicated doubling (4 products + 4 squarings + one by a).  No formula has an exceptional case on a complete curve, so the lanes of a
// wavefront never diverge over the values they add: a zero digit adds the identity, a negative one negates x and t with selects.
// Results leave as (X : Y : Z); T is dropped.
//
// -DFR_EDWARDS_FAULT=n builds one of four seeded WRONG-RESULT variants for the host emulation only (tests/test_simt_fr_edwards.py must
// tell each from the real kernels; none of them touches an index or a bound):
//   1 the top window's borrowed bit is dropped, 2 a negative digit's table entry is not negated, 3 the last term of a chunk is skipped,
//   4 the combine pass skips a segment's first partial.
#pragma once
#include "fr.hip.h"
#include "fr_scan.hip.h"
#include "fr_edwards_plan.h"

namespace bls {

struct EdPt { Fr x, y, z, t; };                   // extended coordinates
struct EdAff { Fr x, y, dt; };                    // a table entry: affine, dt = d x y
struct EdArgs { FrArg a, d; };                    // the curve, passed by value

DEV Fr ed_arg(const FrArg& v) { Fr r; for (int i = 0; i < 8; i++) r.l[i] = v.w[i]; return r; }
DEV Fr ed_sel(bool take, const Fr& a, const Fr& b) { Fr r; for (int i = 0; i < 8; i++) r.l[i] = take ? a.l[i] : b.l[i]; return r; }
DEV bool ed_eq(const Fr& a, const Fr& b) { u32 t = 0; for (int i = 0; i < 8; i++) t |= a.l[i] ^ b.l[i]; return t == 0; }
DEV EdPt ed_identity() { EdPt p; p.x = fr_zero(); p.y = fr_one(); p.z = fr_one(); p.t = fr_zero(); return p; }
DEV EdPt ed_from_affine(const Fr& x, const Fr& y) { EdPt p; p.x = x; p.y = y; p.z = fr_one(); p.t = fr_mul(x, y); return p; }

// P + Q, unified: A = X1 X2, B = Y1 Y2, C = d T1 T2, D = Z1 Z2, E = (X1 + Y1)(X2 + Y2) - A - B, F = D - C, G = D + C, H = B - a A
DEV EdPt ed_add(const EdPt& p, const EdPt& q, const Fr& a, const Fr& d) {
  const Fr A = fr_mul(p.x, q.x), B = fr_mul(p.y, q.y), C = fr_mul(fr_mul(p.t, q.t), d), D = fr_mul(p.z, q.z);
  const Fr E = fr_sub(fr_sub(fr_mul(fr_add(p.x, p.y), fr_add(q.x, q.y)), A), B);
  const Fr F = fr_sub(D, C), G = fr_add(D, C), H = fr_sub(B, fr_mul(a, A));
  EdPt r;
  r.x = fr_mul(E, F); r.y = fr_mul(G, H); r.t = fr_mul(E, H); r.z = fr_mul(F, G);
  return r;
}
// P + (x, y) with Z2 = 1 and d T2 = dt precomputed
DEV EdPt ed_add_mixed(const EdPt& p, const EdAff& q, const Fr& a) {
  const Fr A = fr_mul(p.x, q.x), B = fr_mul(p.y, q.y), C = fr_mul(p.t, q.dt);
  const Fr E = fr_sub(fr_sub(fr_mul(fr_add(p.x, p.y), fr_add(q.x, q.y)), A), B);
  const Fr F = fr_sub(p.z, C), G = fr_add(p.z, C), H = fr_sub(B, fr_mul(a, A));
  EdPt r;
  r.x = fr_mul(E, F); r.y = fr_mul(G, H); r.t = fr_mul(E, H); r.z = fr_mul(F, G);
  return r;
}
// 2 P: A = X^2, B = Y^2, C = 2 Z^2, D = a A, E = (X + Y)^2 - A - B, G = D + B, F = G - C, H = D - B
DEV EdPt ed_dbl(const EdPt& p, const Fr& a) {
  const Fr A = fr_sqr(p.x), B = fr_sqr(p.y), Z2 = fr_sqr(p.z), C = fr_add(Z2, Z2), D = fr_mul(a, A);
  const Fr E = fr_sub(fr_sub(fr_sqr(fr_add(p.x, p.y)), A), B);
  const Fr G = fr_add(D, B), F = fr_sub(G, C), H = fr_sub(D, B);
  EdPt r;
  r.x = fr_mul(E, F); r.y = fr_mul(G, H); r.t = fr_mul(E, H); r.z = fr_mul(F, G);
  return r;
}
DEV bool ed_on_curve(const Fr& x, const Fr& y, const Fr& a, const Fr& d) {
  const Fr x2 = fr_sqr(x), y2 = fr_sqr(y);
  return ed_eq(fr_add(fr_mul(a, x2), y2), fr_add(fr_one(), fr_mul(d, fr_mul(x2, y2))));
}
DEV void ed_store_out(u32* __restrict__ out, size_t i, const EdPt& p) {
  u32* o = out + i * FRED_OUT_WORDS;
  fr_store(o, p.x); fr_store(o + 8, p.y); fr_store(o + 16, p.z);
}
DEV void ed_store_rec(u32* rec, const EdPt& p) { fr_store(rec, p.x); fr_store(rec + 8, p.y); fr_store(rec + 16, p.z); fr_store(rec + 24, p.t); }
DEV EdPt ed_load_rec(const u32* rec) { EdPt p; p.x = fr_load(rec); p.y = fr_load(rec + 8); p.z = fr_load(rec + 16); p.t = fr_load(rec + 24); return p; }

// digit w of the scalar at k, as the plan header defines it
DEV int ed_digit(const u32* __restrict__ k, int bits, int window, int w, int W) {
#if defined(FR_EDWARDS_FAULT) && FR_EDWARDS_FAULT == 1
  if (w == W - 1 && w > 0) return (int)fred_field(k, w * window, window, bits);
#endif
  (void)W;
  return fred_digit(k, bits, window, w);
}

// ---- check: ok[i] = the point satisfies the curve equation (limbs >= r never do) --------------------------------------------------------
__global__ void __launch_bounds__(FRED_BLOCK) k_fred_check(EdArgs c, const u32* __restrict__ xy, size_t n, uint8_t* __restrict__ ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr x = fr_load(xy + i * FRED_AFF_WORDS), y = fr_load(xy + i * FRED_AFF_WORDS + 8);
  const bool canon = fr_words_below_r(x.l) && fr_words_below_r(y.l);
  ok[i] = canon && ed_on_curve(x, y, ed_arg(c.a), ed_arg(c.d)) ? 1 : 0;
}

// ---- normalize: (X : Y : Z) -> (X / Z, Y / Z), one inversion per workgroup (Montgomery's trick over the lanes: the scans and the inverse
// of fr_scan.hip.h).  A point with Z = 0 gives (0, 1) and ok = 0 and takes no part in the product.  TABLE: the records are table entries
// normalised IN PLACE (a lane reads its record before it writes it) and d x y takes the place of Z; ok is not written.
// LDS: eight words per wavefront.
template <bool TABLE>
__global__ void __launch_bounds__(FRED_BLOCK) k_fred_normalize(EdArgs c, const u32* xyz, size_t n, u32* xy, uint8_t* __restrict__ ok) {
  BLS_DYN_LDS(wrec);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  Fr X = fr_zero(), Y = fr_one(), Z = fr_one();
  if (live) { X = fr_load(xyz + i * FRED_OUT_WORDS); Y = fr_load(xyz + i * FRED_OUT_WORDS + 8); Z = fr_load(xyz + i * FRED_OUT_WORDS + 16); }
  const bool zero = fr_is_zero(Z);
  if (zero) Z = fr_one();
  const Fr before = frs_block_prod_excl<false>(Z, wrec);
  const Fr after = frs_block_prod_excl<true>(Z, wrec);
  if (threadIdx.x < 64) {                          // one wavefront inverts the workgroup's product (every lane holds the same value)
    const Fr inv = frs_inv(frs_mul(frs_mul(before, Z), after));
    if (threadIdx.x == 0) fr_store(wrec, inv);
  }
  __syncthreads();
  if (!live) return;
  const Fr zi = frs_mul(frs_mul(fr_load(wrec), before), after);
  Fr x = frs_mul(X, zi), y = frs_mul(Y, zi);
  if (zero) { x = fr_zero(); y = fr_one(); }
  if (TABLE) {
    u32* o = xy + i * FRED_ENTRY_WORDS;
    fr_store(o, x); fr_store(o + 8, y); fr_store(o + 16, frs_mul(ed_arg(c.d), frs_mul(x, y)));
  } else {
    fr_store(xy + i * FRED_AFF_WORDS, x); fr_store(xy + i * FRED_AFF_WORDS + 8, y);
    if (ok) ok[i] = zero ? 0 : 1;
  }
}

// ---- mul_batch: out[i] = s_i P_i, one pair per lane, ONE launch ---------------------------------------------------------------------------
// Signed windows of FRED_MUL_WINDOW bits from the top: W - 1 runs of `window` doublings and W additions, W = fred_windows(bits, window),
// so the work depends on `bits` alone.  A lane's multiples 1 P .. 4 P live in LDS, word-interleaved over the lanes (word v of entry e of
// lane l at (e * 32 + v) * blockDim.x + l: whatever entries the lanes pick, lane l stays on bank l), because the entry is chosen by the
// digit and a register array indexed by a lane's value would go to scratch.  The scalar is read from memory window by window for the same
// reason.  No barrier: a lane touches its own LDS words only.
__global__ void __launch_bounds__(FRED_MUL_BLOCK) k_fred_mul(EdArgs c, const u32* __restrict__ xy, const u32* __restrict__ scalars, int bits, size_t n, u32* __restrict__ out,
                                                             u32* __restrict__ status) {
  BLS_DYN_LDS(tab);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 B = blockDim.x, l = threadIdx.x;
  const Fr a = ed_arg(c.a), d = ed_arg(c.d);
  const EdPt p = ed_from_affine(fr_load(xy + i * FRED_AFF_WORDS), fr_load(xy + i * FRED_AFF_WORDS + 8));
  {
    EdPt m = p;                                    // k P by additions: P + P is the unified law's doubling
#pragma unroll 1
    for (int e = 0; e < FRED_MUL_ENTRIES; e++) {
      if (e) m = ed_add(m, p, a, d);
#pragma unroll
      for (int v = 0; v < 8; v++) {
        tab[(e * 32 + v) * B + l] = m.x.l[v]; tab[(e * 32 + 8 + v) * B + l] = m.y.l[v];
        tab[(e * 32 + 16 + v) * B + l] = m.z.l[v]; tab[(e * 32 + 24 + v) * B + l] = m.t.l[v];
      }
    }
  }
  const u32* k = scalars + i * 8;
  if (!fred_scalar_fits(k, bits)) atomicOr(status, FRED_STATUS_SCALAR);      // reported, this output is unspecified
  const int W = fred_windows(bits, FRED_MUL_WINDOW);
  EdPt acc = ed_identity();
#pragma unroll 1
  for (int w = W - 1; w >= 0; w--) {
    if (w != W - 1) {
#pragma unroll 1
      for (int j = 0; j < FRED_MUL_WINDOW; j++) acc = ed_dbl(acc, a);
    }
    const int dg = ed_digit(k, bits, FRED_MUL_WINDOW, w, W);
    const int m = dg < 0 ? -dg : dg;
    const int e = m ? m - 1 : 0;
    EdPt q;
#pragma unroll
    for (int v = 0; v < 8; v++) {
      q.x.l[v] = tab[(e * 32 + v) * B + l]; q.y.l[v] = tab[(e * 32 + 8 + v) * B + l];
      q.z.l[v] = tab[(e * 32 + 16 + v) * B + l]; q.t.l[v] = tab[(e * 32 + 24 + v) * B + l];
    }
#if !(defined(FR_EDWARDS_FAULT) && FR_EDWARDS_FAULT == 2)
    q.x = ed_sel(dg < 0, fr_neg(q.x), q.x);
    q.t = ed_sel(dg < 0, fr_neg(q.t), q.t);
#endif
    const EdPt id = ed_identity();
    q.x = ed_sel(m == 0, id.x, q.x); q.y = ed_sel(m == 0, id.y, q.y); q.z = ed_sel(m == 0, id.z, q.z); q.t = ed_sel(m == 0, id.t, q.t);
    acc = ed_add(acc, q, a, d);
  }
  ed_store_out(out, i, acc);
}

// ---- fixed-base tables ---------------------------------------------------------------------------------------------------------------
// BUILD: lane g = base * W + w computes Q = 2^(w window) B by doublings and writes Q, 2 Q .. H Q as (X : Y : Z) into the entries' own
// 24 words; the NORM launch (k_fred_normalize<true>) then makes them (x, y, d x y) in place.  A base that is not on the curve (or has
// limbs >= r) sets flag[0]: the caller reads it back and drops the table.
__global__ void __launch_bounds__(FRED_BLOCK) k_fred_table_build(EdArgs c, const u32* __restrict__ xy, size_t n, int window, int W, int H, u32* __restrict__ table,
                                                                  u32* __restrict__ flag) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n * (size_t)W) return;
  const size_t base = g / (size_t)W;
  const int w = (int)(g - base * (size_t)W);
  const Fr a = ed_arg(c.a), d = ed_arg(c.d);
  const Fr x = fr_load(xy + base * FRED_AFF_WORDS), y = fr_load(xy + base * FRED_AFF_WORDS + 8);
  if (w == 0 && !(fr_words_below_r(x.l) && fr_words_below_r(y.l) && ed_on_curve(x, y, a, d))) flag[0] = 1u;      // every writer stores the same word
  EdPt q = ed_from_affine(x, y);
#pragma unroll 1
  for (int j = 0; j < w * window; j++) q = ed_dbl(q, a);
  EdPt m = q;
#pragma unroll 1
  for (int k = 1; k <= H; k++) {
    if (k > 1) m = ed_add(m, q, a, d);
    ed_store_out(table, fred_entry(base, w, k, W, H), m);
  }
}

// ---- the segmented MSM ---------------------------------------------------------------------------------------------------------------
// PREP: lane j widens offsets[j] for the cut functions of gsum_plan.h and checks segment j: offsets[0] = 0, non-decreasing, the last one
// equal to total, the segment's bases inside the table.  A broken segment sets FRED_STATUS_BAD; the passes stay inside the caller's
// arrays whatever the offsets hold (gsum_off clamps to total, a base outside the table is skipped).
__global__ void __launch_bounds__(FRED_BLOCK) k_fred_msm_prep(const u32* __restrict__ offsets, const u32* __restrict__ base_first, size_t k, u32 total, size_t nbases,
                                                               unsigned long long* __restrict__ off64, u32* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > k) return;
  const u32 o = offsets[j];
  off64[j] = o;
  bool bad = (j == 0 && o != 0) || (j == k && o != total);
  if (j < k) {
    const u32 o1 = offsets[j + 1];
    if (o1 < o || o1 > total) bad = true;
    else if ((unsigned long long)(base_first ? base_first[j] : o) + (o1 - o) > nbases) bad = true;
  }
  if (bad) atomicOr(status, FRED_STATUS_BAD);
}

struct EdMsmArgs {
  EdArgs c;
  const u32* table; u32 nbases; int bits, window, W, H;
};
// acc + scalar(t) * base: W table additions
DEV EdPt ed_msm_term(EdPt acc, const EdMsmArgs& m, const Fr& a, u32 base, const u32* __restrict__ k) {
#pragma unroll 1
  for (int w = 0; w < m.W; w++) {
    const int dg = ed_digit(k, m.bits, m.window, w, m.W);
    const int mag = dg < 0 ? -dg : dg;
    const u32* e = m.table + fred_entry(base, w, mag ? mag : 1, m.W, m.H) * FRED_ENTRY_WORDS;
    EdAff q;
    q.x = fr_load(e); q.y = fr_load(e + 8); q.dt = fr_load(e + 16);
#if !(defined(FR_EDWARDS_FAULT) && FR_EDWARDS_FAULT == 2)
    q.x = ed_sel(dg < 0, fr_neg(q.x), q.x);
    q.dt = ed_sel(dg < 0, fr_neg(q.dt), q.dt);
#endif
    q.x = ed_sel(mag == 0, fr_zero(), q.x); q.y = ed_sel(mag == 0, fr_one(), q.y); q.dt = ed_sel(mag == 0, fr_zero(), q.dt);
    acc = ed_add_mixed(acc, q, a);
  }
  return acc;
}

// pass 1: a workgroup per chunk, the schedule of k_gsum_chunks (gsum.hip.h) with a term = one fixed-base product.
// LDS: blockDim.x records at a pitch of FRED_LDS_REC_WORDS (36 words: sixteen consecutive lanes cover the 64 banks once with 16-byte
// accesses, a pitch of 32 would put every lane on two of them), then blockDim.x keys, then blockDim.x head flags.
__global__ void __launch_bounds__(FRED_MSM_BLOCK) k_fred_msm_chunks(EdMsmArgs m, const u32* __restrict__ base_first, const u32* __restrict__ scalars,
                                                                     const unsigned long long* __restrict__ offsets, u32 nseg, u32 total, u32 terms, u32* __restrict__ out,
                                                                     u32* __restrict__ part, u32* __restrict__ meta, u32* __restrict__ status) {
  BLS_DYN_LDS(fred_lds);
  constexpr int PW = FRED_REC_WORDS, LW = FRED_LDS_REC_WORDS;
  const u32 B = blockDim.x, l = threadIdx.x;
  const size_t c = blockIdx.x;
  const u32 chunk = B * terms, cb = (u32)c * chunk, ce = total - cb < chunk ? total : cb + chunk;
  u32* recs = fred_lds;
  u32* keys = fred_lds + (size_t)B * LW;
  u32* heads = keys + B;
  const Fr a = ed_arg(m.c.a), d = ed_arg(m.c.d);
  const u32 b = (size_t)cb + (size_t)l * terms < ce ? cb + l * terms : ce, e = ce - b < terms ? ce : b + terms;
  const bool active = b < e;
  u32 s = GSUM_NONE;
  bool has_head = false;
  EdPt acc = ed_identity();
  if (active) {
    s = gsum_seg_of(offsets, nseg, total, b);
    const u32 first = s;
    u32 so = gsum_off(offsets, nseg, total, s), send = gsum_off(offsets, nseg, total, s + 1);
    u32 bf = base_first ? base_first[s] : so;
#if defined(FR_EDWARDS_FAULT) && FR_EDWARDS_FAULT == 3
    const u32 stop = e == ce ? e - 1 : e;
#else
    const u32 stop = e;
#endif
#pragma unroll 1
    for (u32 t = b; t < stop; t++) {
      if (t >= send) {
        // segment s ends inside this slice.  It began before the slice: the lane before this one holds the rest (lane 0: the chunk
        // before this one does, and this is the chunk's HEAD partial).  It began in the slice: it is whole.
        if (s == first && so < b) {
          if (l == 0) ed_store_rec(part + gsum_record(c, so, cb) * PW, acc);
          else { ed_store_rec(recs + (size_t)l * LW, acc); has_head = true; }
        } else {
          ed_store_out(out, s, acc);
        }
        acc = ed_identity();
        do { s++; send = gsum_off(offsets, nseg, total, s + 1); } while (t >= send);          // off(nseg) = total > t ends it
        so = gsum_off(offsets, nseg, total, s);
        bf = base_first ? base_first[s] : so;
      }
      const unsigned long long base = (unsigned long long)bf + (u32)(t - so);
      if (base >= m.nbases) continue;                                                          // never dereferenced; PREP has flagged the segment
      const u32* k = scalars + (size_t)t * 8;
      if (!fred_scalar_fits(k, m.bits)) atomicOr(status, FRED_STATUS_SCALAR);
      acc = ed_msm_term(acc, m, a, (u32)base, k);
    }
  }
  keys[l] = s;
  heads[l] = has_head ? 1u : 0u;
  if (active && l == 0) meta[2 * c] = gsum_seg_of(offsets, nseg, total, cb);
  if (active && e == ce) meta[2 * c + 1] = s;
  __syncthreads();
  // the head of the next lane's slice belongs to the segment this lane ends in (its term b - 1 is this lane's last)
  if (active && l + 1 < B && heads[l + 1]) acc = ed_add(acc, ed_load_rec(recs + (size_t)(l + 1) * LW), a, d);
  __syncthreads();
  if (active) ed_store_rec(recs + (size_t)l * LW, acc);
  __syncthreads();
  // segmented tree: after the step with distance dist, lane l holds the sum of the lanes l .. l + 2 dist - 1 that share its key
#pragma unroll 1
  for (u32 dist = 1; dist < B; dist <<= 1) {
    const bool take = active && l + dist < B && keys[l + dist] == s;
    EdPt o = ed_identity();
    if (take) o = ed_load_rec(recs + (size_t)(l + dist) * LW);
    __syncthreads();
    if (take) { acc = ed_add(acc, o, a, d); ed_store_rec(recs + (size_t)l * LW, acc); }
    __syncthreads();
  }
  // the first lane of every run of equal keys holds the run's sum
  if (active && (l == 0 || keys[l - 1] != s)) {
    const u32 so = gsum_off(offsets, nseg, total, s), se = gsum_off(offsets, nseg, total, s + 1);
    if (gsum_inside(so, se, cb, chunk)) ed_store_out(out, s, acc);
    else ed_store_rec(part + gsum_record(c, so, cb) * PW, acc);
  }
}

// pass 2: job blockIdx.x of gsum_plan.h, and (0 : 1 : 1) for the empty segments.  LDS: blockDim.x records.
__global__ void __launch_bounds__(FRED_MSM_BLOCK) k_fred_msm_combine(EdArgs c, const unsigned long long* __restrict__ offsets, u32 nseg, u32 total, u32 chunk, size_t nchunks,
                                                                      const u32* __restrict__ part, const u32* __restrict__ meta, u32* __restrict__ out) {
  BLS_DYN_LDS(fred_lds);
  constexpr int PW = FRED_REC_WORDS, LW = FRED_LDS_REC_WORDS;
  const u32 B = blockDim.x, l = threadIdx.x;
  const size_t j = blockIdx.x;
  const Fr a = ed_arg(c.a), d = ed_arg(c.d);
  {
    const size_t i = j * B + l;
    if (i < nseg && gsum_off(offsets, nseg, total, (u32)i) >= gsum_off(offsets, nseg, total, (u32)i + 1)) ed_store_out(out, i, ed_identity());
  }
  if (j >= 2 * nchunks) return;
  const size_t ch = j >> 1;
  u32 s = 0; size_t c_last = 0;
  if (!gsum_job(offsets, nseg, total, chunk, ch, (int)(j & 1), meta[2 * ch], meta[2 * ch + 1], &s, &c_last)) return;      // the same answer in every lane
  const size_t count = c_last - ch + 1;                      // this chunk's record, then the HEAD records of the chunks behind it
  EdPt acc = ed_identity();
#if defined(FR_EDWARDS_FAULT) && FR_EDWARDS_FAULT == 4
  for (size_t k = l ? l : B; k < count; k += B)
#else
  for (size_t k = l; k < count; k += B)
#endif
    acc = ed_add(acc, ed_load_rec(part + (k ? 2 * (ch + k) : j) * PW), a, d);
  ed_store_rec(fred_lds + (size_t)l * LW, acc);
  __syncthreads();
#pragma unroll 1
  for (u32 dist = B >> 1; dist >= 1; dist >>= 1) {
    if (dist >= count) continue;                             // the lanes from dist on hold identities
    if (l < dist) {
      acc = ed_add(acc, ed_load_rec(fred_lds + (size_t)(l + dist) * LW), a, d);
      ed_store_rec(fred_lds + (size_t)l * LW, acc);
    }
    __syncthreads();
  }
  if (l == 0) ed_store_out(out, s, acc);
}

}  // namespace bls
