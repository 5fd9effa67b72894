// fr_edwards_plan.h -- twisted Edwards groups over Fr (blsgpu_fr_edwards_*) as plain host code: the limits, every argument check, the
// `complete` test of a curve, the signed-window recoding of a 256-bit integer, the layout of a fixed-base table and the launch shapes
// and scratch bytes of every operation.  No HIP calls here: api_fr.hip launches from these plans, fr_edwards.hip.h reads the recoding
// and the table layout through the FRED_HD functions below, tests/simt/emu_fr_edwards.cpp walks the same plans on the host and
// tests/cpp/fr_edwards_plan_main.cpp sweeps this header under sanitizers.
//
// The curve is  a x^2 + y^2 = 1 + d x^2 y^2  over Fr, a and d the caller's (the library ships NO parameter set).  The group law is the
// unified addition of Hisil, Wong, Carter and Dawson in extended coordinates (X : Y : Z : T), x = X / Z, y = Y / Z, T = X Y / Z.  It is
// COMPLETE -- exact for every pair of curve points -- exactly when a is a square and d is not (Bernstein, Birkner, Joye, Lange, Peters
// 2008); fred_complete decides that with two Euler-criterion powers.  On any other curve a denominator 1 +- d x1 x2 y1 y2 can only
// vanish when P + Q or P - Q is one of the points of order 2 or 4 at infinity, so sums of points of ODD order stay exact there.
//
// ---- the recoding ------------------------------------------------------------------------------------------------------------------
// A scalar is a plain 256-bit little-endian integer of which the low `bits` bits are read (it is NOT an Fr element: the order of these
// groups is not r).  With windows of `window` bits there are W = ceil((bits + 1) / window) signed digits
//     digit_w = (bits [w window, (w + 1) window) of k) + bit (w window - 1) - 2^window bit ((w + 1) window - 1)
// each in [-2^(window-1), 2^(window-1)]: every digit reads window + 1 bits of k and nothing of its neighbours (no carry chain, so a
// lane can take the windows in any order), and  sum_w digit_w 2^(w window) = k  because the borrowed top bit of a window is the bit
// the next window adds back; the last window's top bit lies at or above `bits` and reads as 0, which is what the + 1 in W is for.
//
// ---- the fixed-base table ---------------------------------------------------------------------------------------------------------
// For base b, window w and k = 1 .. H = 2^(window-1) the entry (b W + w) H + (k - 1) holds k 2^(w window) B_b as (x, y, d x y): affine
// with the product the mixed addition wants, 24 u32 words.  A term of an MSM is then W mixed additions (a zero digit adds (0, 1, 0))
// and no doubling.
//
// ---- the segmented MSM ----------------------------------------------------------------------------------------------------------
// The term list of a call is cut exactly as the gathered point sums cut theirs (gsum_plan.h: chunks of block * terms terms, a lane a
// slice of `terms`, HEAD / TAIL records of the chunk-crossing segments, one combine job per such segment); the u32 CSR offsets of the
// call are widened to the 64-bit offsets those functions read by the PREP launch, which also checks every segment.
#pragma once
#include <cstddef>
#include <cstdint>
#include "fr_poseidon_plan.h"                      // Fr on the host (frp_*: Montgomery limbs, canonical)
#include "gsum_plan.h"

#if defined(__HIPCC__)
#define FRED_HD __host__ __device__ inline
#else
#define FRED_HD inline
#endif

// lanes per workgroup and terms per lane of pass 1 of the MSM, lanes of mul_batch; -D overrides them for a build
#ifndef FRED_MSM_BLOCK
#define FRED_MSM_BLOCK 128
#endif
#ifndef FRED_MSM_TERMS
#define FRED_MSM_TERMS 2
#endif
#ifndef FRED_MUL_BLOCK
#define FRED_MUL_BLOCK 64
#endif

namespace bls {

constexpr int FRED_BLOCK = 256;                              // check / normalize / table kernels
constexpr int FRED_MUL_WINDOW = 3;                           // mul_batch: a lane's table is 1 P .. 4 P in LDS
constexpr int FRED_MUL_ENTRIES = 1 << (FRED_MUL_WINDOW - 1);
constexpr int FRED_BITS_MAX = 256;
constexpr int FRED_WINDOW_MIN = 2, FRED_WINDOW_MAX = 8;
constexpr size_t FRED_MAX_POINTS = (size_t)1 << 26;          // points of one check / normalize / mul_batch call
constexpr size_t FRED_MAX_BASES = (size_t)1 << 24;           // bases of one table
constexpr size_t FRED_MAX_TOTAL = (size_t)1 << 26;           // terms of one msm_segments call
constexpr size_t FRED_MAX_SEGS = (size_t)1 << 26;            // segments of one msm_segments call
constexpr size_t FRED_TABLE_MAX_BYTES = (size_t)1 << 31;     // a table above 2 GiB is refused
constexpr uint32_t FRED_STATUS_SCALAR = 1u;                  // d_status bit 0, shared with every scalar-reading call: a scalar has a bit at or above `bits`
constexpr uint32_t FRED_STATUS_BAD = (uint32_t)1 << 8;       // d_status bit 8: a segment broke the offsets / base-range contract (device form)
constexpr int FRED_AFF_WORDS = 16, FRED_OUT_WORDS = 24, FRED_ENTRY_WORDS = 24, FRED_REC_WORDS = 32;      // (x, y); (X : Y : Z); (x, y, d x y); (X : Y : Z : T)
constexpr int FRED_LDS_REC_WORDS = 36;                       // pitch of a record in the LDS of the MSM passes (fr_edwards.hip.h)
constexpr size_t FRED_LDS_LIMIT = 64 * 1024;                 // what a kernel gets unasked

// ---- the recoding, as the kernels read it ----------------------------------------------------------------------------------------------
FRED_HD int fred_windows(int bits, int window) { return (bits + window) / window; }      // ceil((bits + 1) / window)
// bits [pos, pos + len) of the low `bits` bits of k (eight little-endian words), len <= 9; a position below 0 or from `bits` on reads as 0
FRED_HD uint32_t fred_field(const uint32_t* k, int pos, int len, int bits) {
  const int lo = pos < 0 ? 0 : pos;
  const int hi = pos + len < bits ? pos + len : bits;
  if (hi <= lo) return 0;
  const int idx = lo >> 5, sh = lo & 31;                     // lo < bits <= 256: idx <= 7
  uint64_t v = k[idx];
  if (idx + 1 < 8) v |= (uint64_t)k[idx + 1] << 32;
  v >>= sh;
  v &= ((uint64_t)1 << (hi - lo)) - 1;
  return (uint32_t)(v << (lo - pos));
}
// digit w < fred_windows(bits, window), in [-2^(window-1), 2^(window-1)]
FRED_HD int fred_digit(const uint32_t* k, int bits, int window, int w) {
  const uint32_t f = fred_field(k, w * window - 1, window + 1, bits);      // the bit below the window, then the window
  return (int)((f + 1) >> 1) - (int)((f >> window) << window);
}
// no bit at or above `bits` is set
FRED_HD bool fred_scalar_fits(const uint32_t* k, int bits) {
  uint32_t over = 0;
  for (int i = 0; i < 8; i++) {
    const int lo = 32 * i;
    if (bits <= lo) over |= k[i];
    else if (bits < lo + 32) over |= k[i] >> (bits - lo);
  }
  return over == 0;
}

// ---- the table layout --------------------------------------------------------------------------------------------------------------
FRED_HD int fred_table_half(int window) { return 1 << (window - 1); }       // H: multiples per window
// entry of k 2^(w window) B_base, k in [1, H]
FRED_HD size_t fred_entry(size_t base, int w, int k, int W, int H) { return (base * (size_t)W + (size_t)w) * (size_t)H + (size_t)(k - 1); }

// ---- a curve ---------------------------------------------------------------------------------------------------------------------------
struct FredCurve { FrpFe a, d; int complete = 0; };
inline bool fred_is_square(const FrpFe& x) {                  // Euler: x^((r-1)/2) = 1 (x != 0)
  uint64_t e[4];
  for (int i = 0; i < 4; i++) e[i] = FRP_R64[i];
  e[0] -= 1;                                                 // r is odd
  for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i + 1 < 4 ? e[i + 1] << 63 : 0);
  FrpFe r = frp_one();
  for (int i = 255; i >= 0; i--) { r = frp_mul(r, r); if ((e[i >> 6] >> (i & 63)) & 1) r = frp_mul(r, x); }
  return frp_eq(r, frp_one());
}
inline int fred_complete(const FrpFe& a, const FrpFe& d) { return fred_is_square(a) && !fred_is_square(d) ? 1 : 0; }
inline FrpFe fred_fe(const uint64_t* p) { return FrpFe{{p[0], p[1], p[2], p[3]}}; }
// NULL when (a, d) is a curve the library takes, or the text of the refusal
inline const char* fred_curve_check(const uint64_t* a, const uint64_t* d, FredCurve* out) {
  if (!a) return "fr_edwards_create: NULL a";
  if (!d) return "fr_edwards_create: NULL d";
  if (!frp_below_r(a)) return "fr_edwards_create: a is not a canonical Scalar (limbs >= r)";
  if (!frp_below_r(d)) return "fr_edwards_create: d is not a canonical Scalar (limbs >= r)";
  const FrpFe fa = fred_fe(a), fd = fred_fe(d);
  if (frp_is_zero(fa)) return "fr_edwards_create: a must not be 0";
  if (frp_is_zero(fd)) return "fr_edwards_create: d must not be 0";
  if (frp_eq(fa, fd)) return "fr_edwards_create: a and d must differ (the curve is singular)";
  if (out) { out->a = fa; out->d = fd; out->complete = fred_complete(fa, fd); }
  return nullptr;
}
// a x^2 + y^2 = 1 + d x^2 y^2 for canonical limbs; false for limbs >= r
inline bool fred_on_curve(const FredCurve& c, const uint64_t* xy) {
  if (!frp_below_r(xy) || !frp_below_r(xy + 4)) return false;
  const FrpFe x2 = frp_mul(fred_fe(xy), fred_fe(xy)), y2 = frp_mul(fred_fe(xy + 4), fred_fe(xy + 4));
  return frp_eq(frp_add(frp_mul(c.a, x2), y2), frp_add(frp_one(), frp_mul(c.d, frp_mul(x2, y2))));
}

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal ----------------------------------------------------
inline bool fred_overlap(const void* p, size_t pb, const void* q, size_t qb) {
  if (!p || !q || !pb || !qb) return false;
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qb && b < a + pb;
}
inline bool fred_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
// check: xy -> ok
inline const char* fred_check_args(const void* xy, size_t n, const void* ok, bool device) {
  if (n > FRED_MAX_POINTS) return "fr_edwards_check: n must not exceed 2^26";
  if (!n) return nullptr;
  if (!xy || !ok) return "fr_edwards_check: NULL pointer with points to check";
  if (device && fred_misaligned(xy)) return "fr_edwards_check: d_xy must be 16-byte aligned";
  if (fred_overlap(xy, n * 64, ok, n)) return "fr_edwards_check: ok overlaps the points";
  return nullptr;
}
// normalize: xyz -> xy, ok (ok may be NULL).  There is NO in-place form: the strides differ.
inline const char* fred_normalize_args(const void* xyz, size_t n, const void* xy, const void* ok, bool device) {
  if (n > FRED_MAX_POINTS) return "fr_edwards_normalize: n must not exceed 2^26";
  if (!n) return nullptr;
  if (!xyz || !xy) return "fr_edwards_normalize: NULL pointer with points to convert";
  if (device && (fred_misaligned(xyz) || fred_misaligned(xy))) return "fr_edwards_normalize: d_xyz and d_xy must be 16-byte aligned";
  if (fred_overlap(xyz, n * 96, xy, n * 64)) return "fr_edwards_normalize: xy overlaps xyz (there is no in-place form)";
  if (fred_overlap(xyz, n * 96, ok, n) || fred_overlap(xy, n * 64, ok, n)) return "fr_edwards_normalize: ok overlaps the points";
  return nullptr;
}
inline const char* fred_mul_args(const void* xy, const void* scalars, int bits, size_t n, const void* out, bool device) {
  if (bits < 1 || bits > FRED_BITS_MAX) return "fr_edwards_mul_batch: bits must be in [1, 256]";
  if (n > FRED_MAX_POINTS) return "fr_edwards_mul_batch: n must not exceed 2^26";
  if (!n) return nullptr;
  if (!xy || !scalars || !out) return "fr_edwards_mul_batch: NULL pointer with products to form";
  if (device && (fred_misaligned(xy) || fred_misaligned(scalars) || fred_misaligned(out))) return "fr_edwards_mul_batch: device pointers must be 16-byte aligned";
  if (fred_overlap(xy, n * 64, out, n * 96) || fred_overlap(scalars, n * 32, out, n * 96)) return "fr_edwards_mul_batch: out_xyz overlaps an input";
  return nullptr;
}

// ---- launch shapes -------------------------------------------------------------------------------------------------------------------
struct FredLaunch { unsigned grid = 0, block = 0; size_t lds = 0; };
inline FredLaunch fred_points_launch(size_t n, int block = FRED_BLOCK) {      // check / normalize: a point per lane, whole wavefronts
  FredLaunch l;
  l.grid = (unsigned)((n + block - 1) / block); l.block = (unsigned)block;
  l.lds = (size_t)(block / 64) * 8 * 4;                      // normalize: one scalar per wavefront
  return l;
}
struct FredMulPlan { int ok = 0; int W = 0, doublings = 0; FredLaunch mul; };
constexpr size_t fred_mul_lds_bytes(int block) { return (size_t)block * FRED_MUL_ENTRIES * FRED_REC_WORDS * 4; }
inline FredMulPlan fred_mul_plan(size_t n, int bits, int block = FRED_MUL_BLOCK) {
  FredMulPlan p;
  if (bits < 1 || bits > FRED_BITS_MAX || n > FRED_MAX_POINTS || block < 1 || block > 1024 || fred_mul_lds_bytes(block) > FRED_LDS_LIMIT) return p;
  p.W = fred_windows(bits, FRED_MUL_WINDOW);
  p.doublings = FRED_MUL_WINDOW * (p.W - 1);
  p.mul.grid = (unsigned)((n + block - 1) / block); p.mul.block = (unsigned)block; p.mul.lds = fred_mul_lds_bytes(block);
  p.ok = 1;
  return p;
}
static_assert(fred_mul_lds_bytes(FRED_MUL_BLOCK) <= FRED_LDS_LIMIT, "the mul_batch tables of a workgroup must fit the LDS a kernel gets unasked");

// a fixed-base table: sizes, and the two launches that build it (BUILD: a lane per (base, window) writes the H multiples projectively
// into the table's own memory; NORM: a lane per entry, one inversion per workgroup, in place)
struct FredTablePlan {
  int ok = 0; const char* why = nullptr;
  int bits = 0, window = 0, W = 0, H = 0;
  size_t n = 0, entries = 0, bytes = 0;
  FredLaunch build, norm;
};
inline FredTablePlan fred_table_plan(size_t n, int bits, int window, int block = FRED_BLOCK) {
  FredTablePlan p;
  if (bits < 1 || bits > FRED_BITS_MAX) { p.why = "fr_edwards_bases: bits must be in [1, 256]"; return p; }
  if (window < FRED_WINDOW_MIN || window > FRED_WINDOW_MAX) { p.why = "fr_edwards_bases: window must be in [2, 8]"; return p; }
  if (n < 1 || n > FRED_MAX_BASES) { p.why = "fr_edwards_bases: n must be in [1, 2^24]"; return p; }
  p.bits = bits; p.window = window; p.W = fred_windows(bits, window); p.H = fred_table_half(window); p.n = n;
  const size_t per_base = (size_t)p.W * p.H * FRED_ENTRY_WORDS * 4;        // at most 129 * 128 * 96 bytes
  if (n > FRED_TABLE_MAX_BYTES / per_base) { p.why = "fr_edwards_bases: the table would exceed 2 GiB (n * W * 2^(window-1) * 96 bytes)"; return p; }
  p.entries = n * p.W * p.H; p.bytes = n * per_base;
  p.build = fred_points_launch(n * p.W, block);
  p.norm = fred_points_launch(p.entries, block);
  p.ok = 1;
  return p;
}

// the segmented MSM: PREP (a lane per offset), pass 1 (a workgroup per chunk), pass 2 (the jobs of gsum_plan.h and the empty segments)
struct FredMsmShape { int block = FRED_MSM_BLOCK, terms = FRED_MSM_TERMS; };
struct FredMsmPlan {
  int ok = 0;
  GsumPlan cut;                        // chunk, nchunks and the grids of the two passes
  FredLaunch prep, chunks, combine;
  size_t off_bytes = 0, part_bytes = 0, meta_bytes = 0;      // the widened offsets, 2 nchunks records of FRED_REC_WORDS, 2 nchunks segment numbers
};
constexpr size_t fred_msm_lds_bytes(int block) { return (size_t)block * (FRED_LDS_REC_WORDS + 2) * 4; }
inline FredMsmPlan fred_msm_plan(size_t k, size_t total, FredMsmShape s = FredMsmShape()) {
  FredMsmPlan p;
  if (k > FRED_MAX_SEGS || total > FRED_MAX_TOTAL || fred_msm_lds_bytes(s.block) > FRED_LDS_LIMIT) return p;
  p.cut = gsum_plan(1, k, total, GsumShape{s.block, s.terms});
  if (!p.cut.ok) return p;
  p.prep = fred_points_launch(k + 1);
  p.chunks.grid = p.cut.chunks_grid; p.combine.grid = p.cut.combine_grid;
  p.chunks.block = p.combine.block = p.cut.block;
  p.chunks.lds = p.combine.lds = fred_msm_lds_bytes(s.block);
  p.off_bytes = (k + 1) * 8;
  p.part_bytes = p.cut.records * FRED_REC_WORDS * 4;
  p.meta_bytes = p.cut.meta_words * 4;
  p.ok = 1;
  return p;
}

struct FredMsmArgs {
  size_t nbases = 0;
  const void* base_first = nullptr; const void* offsets = nullptr; const void* scalars = nullptr;
  size_t k = 0, total = 0;
  const void* out = nullptr;
  bool device = false;
};
inline const char* fred_msm_args(const FredMsmArgs& a) {
  if (a.k > FRED_MAX_SEGS) return "fr_edwards_msm_segments: k must not exceed 2^26";
  if (a.total > FRED_MAX_TOTAL) return "fr_edwards_msm_segments: total must not exceed 2^26";
  if (!a.k) return a.total ? "fr_edwards_msm_segments: terms but no segment" : nullptr;
  if (!a.offsets || !a.out) return "fr_edwards_msm_segments: NULL offsets or output with segments to sum";
  if (a.total && !a.scalars) return "fr_edwards_msm_segments: NULL scalars with terms to add";
  if (a.device) {
    if (((uintptr_t)a.offsets & 3) || ((uintptr_t)a.base_first & 3)) return "fr_edwards_msm_segments: d_offsets and d_base_first must be 4-byte aligned";
    if (fred_misaligned(a.scalars) || fred_misaligned(a.out)) return "fr_edwards_msm_segments: d_scalars and d_out_xyz must be 16-byte aligned";
  }
  if (fred_overlap(a.scalars, a.total * 32, a.out, a.k * 96) || fred_overlap(a.offsets, (a.k + 1) * 4, a.out, a.k * 96) || fred_overlap(a.base_first, a.k * 4, a.out, a.k * 96))
    return "fr_edwards_msm_segments: out_xyz overlaps an input";
  return nullptr;
}
// what only the host form can see: the offsets as the interface states them and every segment's bases inside the table; *total = offsets[k]
inline const char* fred_msm_args_host(const uint32_t* offsets, const uint32_t* base_first, size_t k, size_t nbases, size_t* total) {
  *total = 0;
  if (!k) return nullptr;
  if (offsets[0] != 0) return "fr_edwards_msm_segments: offsets[0] must be 0";
  for (size_t j = 0; j < k; j++) {
    if (offsets[j] > offsets[j + 1]) return "fr_edwards_msm_segments: offsets must be non-decreasing";
    const uint64_t first = base_first ? base_first[j] : offsets[j];
    if (first + (uint64_t)(offsets[j + 1] - offsets[j]) > nbases) return "fr_edwards_msm_segments: a segment's bases lie outside the table";
  }
  if (offsets[k] > FRED_MAX_TOTAL) return "fr_edwards_msm_segments: total must not exceed 2^26";
  *total = offsets[k];
  return nullptr;
}

}  // namespace bls
