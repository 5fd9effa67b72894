// fr_poseidon_plan.h -- Poseidon over Fr (blsgpu_fr_poseidon_*) as plain host code: the validation of an instance, the derivation of the
// sparse form of its partial rounds, the constant image the kernels of fr_poseidon.hip.h read, and the launch plans of permute / hash_many /
// merkle.  No HIP calls here: api_fr.hip builds a handle and walks a plan, tests/simt/emu_fr_poseidon.cpp walks the same plan on the host
// with a small block, tests/cpp/fr_poseidon_plan_main.cpp runs the derivation against the textbook rounds on the host arithmetic below.
//
// The library ships NO standard parameter set: the caller passes round constants and matrix of the instance it uses (canonical Montgomery
// limbs), see include/bls12_381_hip.h.
//
// ---- the permutation (the definition) -------------------------------------------------------------------------------------------------
//   rounds r = 0 .. R_F + R_P - 1;  rounds R_F/2 .. R_F/2 + R_P - 1 are PARTIAL, the others FULL
//   s[i] += C[r][i];   s[i] = s[i]^5 (full: every i; partial: i = 0 only);   s'[i] = sum_j M[i][j] s[j]
//
// ---- the sparse form of the partial rounds ------------------------------------------------------------------------------------------------
// Walking the partial rounds forward with a pending matrix P = diag(1, Ph) (Ph starts as I) and a carry vector u (starts as 0), the actual
// state being P y + u:
//   c' = C[r] + u;  only k_r = c'[0] meets the S-box (P fixes element 0 and the rest of c' is linear from here on);  u <- M (0, c'[1:])
//   (this walk of the constants needs nothing of P: the DENSE form uses k_r and u as well, so that in both forms a partial round adds one
//   scalar and every operand of a row sum is a reduced value)
//   A = M P = diag(1, Ah) S_r with Ah = A[1:][1:], first row of S_r = A[0][.], first column below the diagonal = Ah^-1 A[1:][0] (a linear
//   solve, no inverse of M), identity elsewhere;  P <- diag(1, Ah)
//   round:  z0 = (y0 + k_r)^5;  y0' = row_0 z0 + sum_(j>=1) row_j y_j;  y_j' = y_j + col_j z0          -- 3 + t + (t - 1) products
// and after the last partial round x[1:] = Ph y[1:] ((t-1)^2 products, once) and u goes into the first constant vector of the second half
// of the full rounds.  Ah = (M[1:][1:])^(r+1), so the form exists iff the lower-right block of M is regular; otherwise AUTO stays DENSE.
//
// ---- the constant image and its scales ---------------------------------------------------------------------------------------------------
// Entries are 9 x 29-bit limbs (FrL of fr.hip.h), canonical.  frl_mul divides by 2^261, not 2^256: a product of two Montgomery values comes
// out short by 2^5.  The S-box is x2 = x x (2^-5), x4 = x2 x2 (2^-15), x5 = x4 x (2^-20); the state itself is always an exact Montgomery
// value (scale 1).  Hence the scale of every multiplier:
//   multiplies an S-box output (every column of the full-round matrix, column 0 of the dense partial matrix, row_0 and col_j)     2^25
//   multiplies a state element that skipped the S-box (columns 1.. of the dense partial matrix, row_j for j >= 1, the pending Ph)  2^5
//   added (round constants, k_r)                                                                                                  1
// products_per_permutation counts the field products a b of the rounds, R_F (3t + t^2) + R_P (2t + 2) + (t-1)^2 sparse and
// R_F (3t + t^2) + R_P (3 + t^2) dense; the products of a row sum share Montgomery reductions (frl_dot), so it is NOT a count of reductions.
// Layout, in entries (FrpArgs carries the offsets):
//   rc1    R_F/2 x t                 constants of the first full rounds
//   part   dense: R_P x 1 = k_r; sparse: R_P x 2t = per round [k_r, row_0 .. row_(t-1), col_1 .. col_(t-1)]
//   pend   sparse: (t-1)^2           Ph 2^5, row-major
//   rc2    R_F/2 x t                 constants of the last full rounds, u added to the first vector
//   mfull  t x t                     M 2^25, row-major
//   mpart  dense: t x t              M with column 0 scaled 2^25 and the others 2^5
//
// ---- launches ----------------------------------------------------------------------------------------------------------------------------
//   permute    PERMUTE                one state per lane
//   hash_many  HASH                   one preimage per lane
//   merkle     height 0: COPY.  Level l = 1 .. height of ALL k trees is one array of k a^(height-l) nodes (tree-major), and the parent of
//              node g is node g / a of the next level, so a level is a HASH over the previous one: one LEVEL launch per level.
//              (A launch that finished the last levels of whole trees in LDS, one workgroup per group of trees, was measured and LOST --
//              1.60 x the time of the per-level launches at 4096 trees of 64 leaves, a tie at one tree of 2^20 -- and is not here:
//              DESIGN.md.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace bls {

constexpr int FRP_BLOCK = 256;                    // lanes per workgroup
constexpr int FRP_MAX_T = 12;
constexpr int FRP_MAX_RF = 16, FRP_MAX_RP = 128;
constexpr size_t FRP_MAX_TOTAL = (size_t)1 << 28;
constexpr int FRP_ENTRY = 9;                      // u32 words of an image entry
constexpr int FRP_MAX_STEPS = 32;

enum FrPoseidonForm { FRP_FORM_AUTO = 0, FRP_FORM_DENSE = 1, FRP_FORM_SPARSE = 2 };
enum FrPoseidonKernel { FRP_K_PERMUTE = 0, FRP_K_HASH = 1, FRP_K_LEVEL = 2, FRP_K_COPY = 4 };
enum FrPoseidonBuf { FRP_BUF_NONE = -1, FRP_BUF_IN = 0, FRP_BUF_OUT = 1, FRP_BUF_NODES = 2 };      // IN: states / inputs / leaves; OUT: out / roots

struct FrPoseidonShape { int block = FRP_BLOCK; };

inline bool frp_width_ok(int t) { return t == 2 || t == 3 || t == 4 || t == 5 || t == 9 || t == 12; }

// what the kernels take by value: the instance's shape and the entry offsets of the image's sections
struct FrpArgs { uint32_t rf_half, rp, rc1, part, pend, rc2, mfull, mpart; };

// ---- Fr on the host: four 64-bit limbs in Montgomery form (R = 2^256), always canonical --------------------------------------------------------
struct FrpFe { uint64_t v[4]; };
constexpr uint64_t FRP_R64[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
constexpr uint64_t frp_neg_inv64() {              // -r^-1 mod 2^64 by Newton's iteration
  uint64_t x = 1;
  for (int i = 0; i < 6; i++) x *= 2 - FRP_R64[0] * x;
  return 0 - x;
}
constexpr uint64_t FRP_NINV = frp_neg_inv64();
inline bool frp_below_r(const uint64_t* a) {
  for (int i = 3; i >= 0; i--) { if (a[i] < FRP_R64[i]) return true; if (a[i] > FRP_R64[i]) return false; }
  return false;
}
inline FrpFe frp_zero() { return FrpFe{{0, 0, 0, 0}}; }
inline bool frp_is_zero(const FrpFe& a) { return !(a.v[0] | a.v[1] | a.v[2] | a.v[3]); }
inline bool frp_eq(const FrpFe& a, const FrpFe& b) { return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2] && a.v[3] == b.v[3]; }
inline void frp_sub_r(uint64_t* a) {
  uint64_t b = 0;
  for (int i = 0; i < 4; i++) { const uint64_t v = a[i], s = v - FRP_R64[i] - b; b = (v < FRP_R64[i] || (v == FRP_R64[i] && b)) ? 1 : 0; a[i] = s; }
}
inline FrpFe frp_add(const FrpFe& a, const FrpFe& b) {       // a + b < 2r < 2^256
  FrpFe r; unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) { c += (unsigned __int128)a.v[i] + b.v[i]; r.v[i] = (uint64_t)c; c >>= 64; }
  if (!frp_below_r(r.v)) frp_sub_r(r.v);
  return r;
}
inline FrpFe frp_neg(const FrpFe& a) {
  if (frp_is_zero(a)) return a;
  FrpFe r; uint64_t b = 0;
  for (int i = 0; i < 4; i++) { const uint64_t v = FRP_R64[i], s = v - a.v[i] - b; b = (v < a.v[i] || (v == a.v[i] && b)) ? 1 : 0; r.v[i] = s; }
  return r;
}
inline FrpFe frp_sub(const FrpFe& a, const FrpFe& b) { return frp_add(a, frp_neg(b)); }
inline FrpFe frp_dbl(const FrpFe& a) { return frp_add(a, a); }
inline FrpFe frp_scale(FrpFe a, int k) { for (int i = 0; i < k; i++) a = frp_dbl(a); return a; }      // 2^k a
// the Montgomery product a b / 2^256 mod r (CIOS over 64-bit limbs, 128-bit partial products)
inline FrpFe frp_mul(const FrpFe& a, const FrpFe& b) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; j++) { c += (unsigned __int128)a.v[j] * b.v[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * FRP_NINV;
    c = (unsigned __int128)m * FRP_R64[0] + t[0]; c >>= 64;
    for (int j = 1; j < 4; j++) { c += (unsigned __int128)m * FRP_R64[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
  }
  FrpFe r{{t[0], t[1], t[2], t[3]}};
  if (t[4] || !frp_below_r(r.v)) frp_sub_r(r.v);
  return r;
}
inline FrpFe frp_one() {                          // 2^256 mod r
  static const FrpFe one = frp_scale(FrpFe{{1, 0, 0, 0}}, 256);
  return one;
}
inline FrpFe frp_pow5(const FrpFe& a) { const FrpFe a2 = frp_mul(a, a); return frp_mul(frp_mul(a2, a2), a); }
inline FrpFe frp_inv(const FrpFe& a) {            // a^(r-2); 0 for 0
  uint64_t e[4] = {FRP_R64[0] - 2, FRP_R64[1], FRP_R64[2], FRP_R64[3]};
  FrpFe r = frp_one();
  for (int i = 255; i >= 0; i--) { r = frp_mul(r, r); if ((e[i >> 6] >> (i & 63)) & 1) r = frp_mul(r, a); }
  return r;
}
// solves A x = b for an n x n matrix (row-major) by Gaussian elimination with a pivot search; false when A is singular
inline bool frp_solve(int n, std::vector<FrpFe> a, std::vector<FrpFe> b, std::vector<FrpFe>* x) {
  for (int c = 0; c < n; c++) {
    int p = c;
    while (p < n && frp_is_zero(a[(size_t)p * n + c])) p++;
    if (p == n) return false;
    if (p != c) { for (int j = 0; j < n; j++) std::swap(a[(size_t)p * n + j], a[(size_t)c * n + j]); std::swap(b[p], b[c]); }
    const FrpFe inv = frp_inv(a[(size_t)c * n + c]);
    for (int j = 0; j < n; j++) a[(size_t)c * n + j] = frp_mul(a[(size_t)c * n + j], inv);
    b[c] = frp_mul(b[c], inv);
    for (int i = 0; i < n; i++) {
      if (i == c || frp_is_zero(a[(size_t)i * n + c])) continue;
      const FrpFe f = a[(size_t)i * n + c];
      for (int j = 0; j < n; j++) a[(size_t)i * n + j] = frp_sub(a[(size_t)i * n + j], frp_mul(f, a[(size_t)c * n + j]));
      b[i] = frp_sub(b[i], frp_mul(f, b[c]));
    }
  }
  *x = b;
  return true;
}

// ---- an instance, validated and planned -----------------------------------------------------------------------------------------------------------
struct FrpSparse {                                // the sparse partial rounds (see the head of this file), unscaled Montgomery values
  std::vector<FrpFe> row;                         // R_P x t
  std::vector<FrpFe> col;                         // R_P x (t - 1)
  std::vector<FrpFe> pend;                        // (t-1) x (t-1)
};
struct FrPoseidonHost {
  int t = 0, r_full = 0, r_partial = 0, form = FRP_FORM_DENSE;      // form: DENSE or SPARSE, what the handle uses
  std::vector<FrpFe> rc, mds;                     // as given
  std::vector<FrpFe> k, u;                        // the walk of the partial rounds' constants: k_r (R_P) and the carry into the second half (t)
  FrpSparse sp;                                   // filled when the sparse form was derived
  FrpArgs args = {};
  std::vector<uint32_t> image;                    // what the kernels read
  size_t products = 0;                            // frl_mul calls of one permutation
};

// The walk of the partial rounds' constants: k[r] and the carry u that is left for the next full round.
inline void frp_carry_constants(int t, int r_partial, const FrpFe* c_part /* r_partial x t */, const FrpFe* m, std::vector<FrpFe>* k, std::vector<FrpFe>* u_out) {
  std::vector<FrpFe> u(t, frp_zero());
  k->clear();
  for (int r = 0; r < r_partial; r++) {
    std::vector<FrpFe> c(t);
    for (int i = 0; i < t; i++) c[i] = frp_add(c_part[(size_t)r * t + i], u[i]);
    k->push_back(c[0]);
    for (int i = 0; i < t; i++) {                   // u = M (0, c'[1:])
      FrpFe a = frp_zero();
      for (int j = 1; j < t; j++) a = frp_add(a, frp_mul(m[(size_t)i * t + j], c[j]));
      u[i] = a;
    }
  }
  *u_out = u;
}
// Derives the sparse form; false when the lower-right block of M is singular (nothing usable in *out then).
inline bool frp_sparse_derive(int t, int r_partial, const FrpFe* m, FrpSparse* out) {
  const int n = t - 1;
  FrpSparse s;
  std::vector<FrpFe> ph((size_t)n * n, frp_zero());          // pending Ph, starts as I
  for (int i = 0; i < n; i++) ph[(size_t)i * n + i] = frp_one();
  for (int r = 0; r < r_partial; r++) {
    // A = M diag(1, Ph): column 0 is M's, A[i][1 + j] = sum_l M[i][1 + l] Ph[l][j]
    std::vector<FrpFe> a((size_t)t * t);
    for (int i = 0; i < t; i++) {
      a[(size_t)i * t] = m[(size_t)i * t];
      for (int j = 0; j < n; j++) {
        FrpFe v = frp_zero();
        for (int l = 0; l < n; l++) v = frp_add(v, frp_mul(m[(size_t)i * t + 1 + l], ph[(size_t)l * n + j]));
        a[(size_t)i * t + 1 + j] = v;
      }
    }
    std::vector<FrpFe> ah((size_t)n * n), b(n), col;
    for (int i = 0; i < n; i++) { b[i] = a[(size_t)(i + 1) * t]; for (int j = 0; j < n; j++) ah[(size_t)i * n + j] = a[(size_t)(i + 1) * t + 1 + j]; }
    if (n && !frp_solve(n, ah, b, &col)) return false;
    for (int j = 0; j < t; j++) s.row.push_back(a[j]);
    for (int j = 0; j < n; j++) s.col.push_back(col[j]);
    ph = ah;
  }
  // regularity is a property of M alone (Ah = (M[1:][1:])^(r+1)): decide it for R_P = 0 as well, so that the form does not depend on R_P
  if (r_partial == 0 && n) {
    std::vector<FrpFe> mh((size_t)n * n), b(n, frp_zero()), x;
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) mh[(size_t)i * n + j] = m[(size_t)(i + 1) * t + 1 + j];
    if (!frp_solve(n, mh, b, &x)) return false;
  }
  s.pend = ph;
  *out = s;
  return true;
}

inline void frp_image_put(std::vector<uint32_t>* img, const FrpFe& a) {       // four 64-bit limbs -> nine 29-bit limbs
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, k = bit >> 6, sh = bit & 63;
    uint64_t v = a.v[k] >> sh;
    if (sh > 35 && k + 1 < 4) v |= a.v[k + 1] << (64 - sh);
    img->push_back((uint32_t)(v & ((1u << 29) - 1)));
  }
}

inline size_t frp_products(int t, int r_full, int r_partial, bool sparse) {
  const size_t T = (size_t)t, full = (size_t)r_full * (3 * T + T * T);
  return sparse ? full + (size_t)r_partial * (2 * T + 2) + (T - 1) * (T - 1) : full + (size_t)r_partial * (3 + T * T);
}

// Validates an instance (include/bls12_381_hip.h: blsgpu_fr_poseidon_create) and builds everything a handle holds.  Returns an empty string
// when it is valid, or the text that names the offending argument or the first bad constant.
inline std::string fr_poseidon_build(int t, int r_full, int r_partial, const uint64_t* round_constants, const uint64_t* mds, int form, FrPoseidonHost* out) {
  char buf[160];
  if (!frp_width_ok(t)) return "fr_poseidon: t must be one of 2, 3, 4, 5, 9, 12";
  if (r_full < 2 || r_full > FRP_MAX_RF || (r_full & 1)) return "fr_poseidon: r_full must be even and in [2, 16]";
  if (r_partial < 0 || r_partial > FRP_MAX_RP) return "fr_poseidon: r_partial must be in [0, 128]";
  if (form != FRP_FORM_AUTO && form != FRP_FORM_DENSE) return "fr_poseidon: form must be BLSGPU_FR_POSEIDON_AUTO or BLSGPU_FR_POSEIDON_DENSE";
  if (!round_constants) return "fr_poseidon: NULL round_constants";
  if (!mds) return "fr_poseidon: NULL mds";
  if (!out) return "fr_poseidon: NULL out";
  const int rounds = r_full + r_partial, h = r_full / 2;
  for (int i = 0; i < rounds * t; i++)
    if (!frp_below_r(round_constants + 4 * (size_t)i)) {
      snprintf(buf, sizeof buf, "fr_poseidon: round_constants[%d] (round %d, element %d) is not a canonical Scalar (limbs >= r)", i, i / t, i % t);
      return buf;
    }
  for (int i = 0; i < t * t; i++)
    if (!frp_below_r(mds + 4 * (size_t)i)) {
      snprintf(buf, sizeof buf, "fr_poseidon: mds[%d] (row %d, column %d) is not a canonical Scalar (limbs >= r)", i, i / t, i % t);
      return buf;
    }
  FrPoseidonHost p;
  p.t = t; p.r_full = r_full; p.r_partial = r_partial;
  p.rc.resize((size_t)rounds * t); p.mds.resize((size_t)t * t);
  for (size_t i = 0; i < p.rc.size(); i++) for (int w = 0; w < 4; w++) p.rc[i].v[w] = round_constants[4 * i + w];
  for (size_t i = 0; i < p.mds.size(); i++) for (int w = 0; w < 4; w++) p.mds[i].v[w] = mds[4 * i + w];
  const FrpFe* c_part = p.rc.data() + (size_t)h * t;
  frp_carry_constants(t, r_partial, c_part, p.mds.data(), &p.k, &p.u);
  const bool sparse = form == FRP_FORM_AUTO && frp_sparse_derive(t, r_partial, p.mds.data(), &p.sp);
  p.form = sparse ? FRP_FORM_SPARSE : FRP_FORM_DENSE;
  p.products = frp_products(t, r_full, r_partial, sparse);
  // the image
  std::vector<uint32_t>& img = p.image;
  FrpArgs& a = p.args;
  a.rf_half = (uint32_t)h; a.rp = (uint32_t)r_partial;
  auto at = [&]() { return (uint32_t)(img.size() / FRP_ENTRY); };
  a.rc1 = at();
  for (int i = 0; i < h * t; i++) frp_image_put(&img, p.rc[i]);
  a.part = at();
  if (sparse) {
    for (int r = 0; r < r_partial; r++) {
      frp_image_put(&img, p.k[r]);
      for (int j = 0; j < t; j++) frp_image_put(&img, frp_scale(p.sp.row[(size_t)r * t + j], j == 0 ? 25 : 5));
      for (int j = 0; j < t - 1; j++) frp_image_put(&img, frp_scale(p.sp.col[(size_t)r * (t - 1) + j], 25));
    }
  } else {
    for (int r = 0; r < r_partial; r++) frp_image_put(&img, p.k[r]);
  }
  a.pend = at();
  if (sparse) for (size_t i = 0; i < p.sp.pend.size(); i++) frp_image_put(&img, frp_scale(p.sp.pend[i], 5));
  a.rc2 = at();
  for (int i = 0; i < h * t; i++) {
    FrpFe c = p.rc[(size_t)(h + r_partial) * t + i];
    if (i < t) c = frp_add(c, p.u[i]);
    frp_image_put(&img, c);
  }
  a.mfull = at();
  for (int i = 0; i < t * t; i++) frp_image_put(&img, frp_scale(p.mds[i], 25));
  a.mpart = at();
  if (!sparse) for (int i = 0; i < t * t; i++) frp_image_put(&img, frp_scale(p.mds[i], i % t == 0 ? 25 : 5));
  *out = p;
  return std::string();
}

// ---- the permutation on the host arithmetic (what the tests of the derivation compare): textbook, and through the sparse form ------------------
inline void frp_host_full_round(const FrPoseidonHost& p, const FrpFe* c, std::vector<FrpFe>* s) {
  const int t = p.t;
  std::vector<FrpFe> x(t), y(t);
  for (int i = 0; i < t; i++) x[i] = frp_pow5(frp_add((*s)[i], c[i]));
  for (int i = 0; i < t; i++) { FrpFe a = frp_zero(); for (int j = 0; j < t; j++) a = frp_add(a, frp_mul(p.mds[(size_t)i * t + j], x[j])); y[i] = a; }
  *s = y;
}
inline void frp_host_textbook(const FrPoseidonHost& p, std::vector<FrpFe>* s) {
  const int t = p.t, h = p.r_full / 2;
  for (int r = 0; r < p.r_full + p.r_partial; r++) {
    const FrpFe* c = p.rc.data() + (size_t)r * t;
    if (r < h || r >= h + p.r_partial) { frp_host_full_round(p, c, s); continue; }
    std::vector<FrpFe> x(t), y(t);
    for (int i = 0; i < t; i++) x[i] = frp_add((*s)[i], c[i]);
    x[0] = frp_pow5(x[0]);
    for (int i = 0; i < t; i++) { FrpFe a = frp_zero(); for (int j = 0; j < t; j++) a = frp_add(a, frp_mul(p.mds[(size_t)i * t + j], x[j])); y[i] = a; }
    *s = y;
  }
}
inline void frp_host_sparse(const FrPoseidonHost& p, std::vector<FrpFe>* s) {      // p.form must be SPARSE
  const int t = p.t, h = p.r_full / 2, n = t - 1;
  for (int r = 0; r < h; r++) frp_host_full_round(p, p.rc.data() + (size_t)r * t, s);
  std::vector<FrpFe>& y = *s;
  for (int r = 0; r < p.r_partial; r++) {
    const FrpFe z0 = frp_pow5(frp_add(y[0], p.k[r]));
    FrpFe y0 = frp_mul(p.sp.row[(size_t)r * t], z0);
    for (int j = 1; j < t; j++) y0 = frp_add(y0, frp_mul(p.sp.row[(size_t)r * t + j], y[j]));
    for (int j = 1; j < t; j++) y[j] = frp_add(y[j], frp_mul(p.sp.col[(size_t)r * n + j - 1], z0));
    y[0] = y0;
  }
  std::vector<FrpFe> x(t);
  x[0] = y[0];
  for (int i = 0; i < n; i++) { FrpFe a = frp_zero(); for (int j = 0; j < n; j++) a = frp_add(a, frp_mul(p.sp.pend[(size_t)i * n + j], y[1 + j])); x[1 + i] = a; }
  for (int r = 0; r < h; r++) {
    std::vector<FrpFe> c(p.rc.begin() + (size_t)(h + p.r_partial + r) * t, p.rc.begin() + (size_t)(h + p.r_partial + r + 1) * t);
    if (r == 0) for (int i = 0; i < t; i++) c[i] = frp_add(c[i], p.u[i]);
    frp_host_full_round(p, c.data(), &x);
  }
  *s = x;
}

// ---- launch plans ------------------------------------------------------------------------------------------------------------------------
struct FrPoseidonStep {
  int kernel;                  // FrPoseidonKernel
  unsigned grid, block;
  size_t items;                // PERMUTE: states; HASH / LEVEL: digests; COPY: scalars
  int src, dst;                // FrPoseidonBuf
  size_t src_off, dst_off;     // scalars into src / dst (levels inside NODES)
  int roots;                   // LEVEL: the last level, written to OUT as well when dst is NODES
};
struct FrPoseidonPlan {
  int n_steps = 0;             // -1: refused
  FrPoseidonStep step[FRP_MAX_STEPS];
  size_t leaves = 0;           // merkle: k a^height
  size_t node_count = 0;       // merkle: k (a^height - 1) / (a - 1), what `nodes` holds
  size_t scratch = 0;          // merkle with nodes == NULL: scalars of the inner levels kept in the context's scratch (it takes the place of NODES)
};
inline unsigned frp_grid(size_t items, FrPoseidonShape s) { return (unsigned)((items + s.block - 1) / s.block); }

// n states of t scalars (PERMUTE) or n preimages of t - 1 scalars (HASH)
inline FrPoseidonPlan fr_poseidon_many_plan(int kernel, int t, size_t n, FrPoseidonShape s = FrPoseidonShape()) {
  FrPoseidonPlan p;
  if (!frp_width_ok(t) || n > FRP_MAX_TOTAL / (size_t)t || (kernel != FRP_K_PERMUTE && kernel != FRP_K_HASH)) { p.n_steps = -1; return p; }
  if (!n) return p;
  p.step[p.n_steps++] = FrPoseidonStep{kernel, frp_grid(n, s), (unsigned)s.block, n, FRP_BUF_IN, FRP_BUF_OUT, 0, 0, 0};
  return p;
}

// k trees of a^height leaves, a = t - 1; keep_nodes: the caller gave `nodes`
inline FrPoseidonPlan fr_poseidon_merkle_plan(int t, int height, size_t k, bool keep_nodes, FrPoseidonShape s = FrPoseidonShape()) {
  FrPoseidonPlan p;
  p.n_steps = -1;
  if (!frp_width_ok(t) || height < 0 || height > 28) return p;
  const size_t a = (size_t)t - 1;
  size_t per = 1;                                 // a^height, overflow-checked against 2^28
  for (int i = 0; i < height; i++) { if (per > FRP_MAX_TOTAL / a) return p; per *= a; }
  if (k > FRP_MAX_TOTAL / per) return p;
  if (a == 1 && height > 0 && k > FRP_MAX_TOTAL / (size_t)height) return p;      // arity 1: height nodes per tree
  p.n_steps = 0;
  p.leaves = k * per;
  p.node_count = a == 1 ? k * (size_t)height : k * ((per - 1) / (a - 1));
  if (p.node_count > FRP_MAX_TOTAL) { p.n_steps = -1; return p; }
  if (!k) return p;
  if (height == 0) { p.step[p.n_steps++] = FrPoseidonStep{FRP_K_COPY, 0, 0, k, FRP_BUF_IN, FRP_BUF_OUT, 0, 0, 1}; return p; }
  size_t n = per, off = 0, prev_off = 0;           // n: nodes per tree of the level being read
  for (int l = 1; l <= height; l++) {
    n /= a;                                       // nodes per tree of level l
    const int src = l == 1 ? FRP_BUF_IN : FRP_BUF_NODES;
    const bool last = l == height;
    // the last level of a tree with nodes == NULL goes to the roots alone
    p.step[p.n_steps++] = FrPoseidonStep{FRP_K_LEVEL, frp_grid(k * n, s), (unsigned)s.block, k * n, src, last && !keep_nodes ? FRP_BUF_OUT : FRP_BUF_NODES, prev_off,
                                         last && !keep_nodes ? 0 : off, last ? 1 : 0};
    if (!last) p.scratch = off + k * n;
    prev_off = off;
    off += k * n;
  }
  if (keep_nodes) p.scratch = 0;
  return p;
}

}  // namespace bls
