// gntt.hip.h -- radix-2 transforms over GROUP elements: k vectors of 2^log_n G1 or G2 points, in place, natural order in and out.
//
//   forward  Y[m] = sum_j [w^(jm)] P[j]        inverse  P[j] = [n^-1] sum_m [w^(-jm)] Y[m]        w = ROOT_OF_UNITY^(2^(32 - log_n))
//
// the w of fr.hip.h, so the transform of [s_j] G is [fr_ntt(s)_m] G.  The reference crate has no such function; the definition above is
// what the kernels are tested against, with the oracle's `g1_mul` / `g2_mul` / `fr_omega` (tests/test_simt_gntt.py, tests/test_g_ntt.py).
// w^(jm) is a residue mod r: the transform is defined on the prime-order subgroup only, the endomorphism ladders of mulbatch.hip.h are
// always used, and points outside the subgroup give unspecified results (as the MSM does under blsgpu_set_assume_subgroup).
//
// Points are projective wire records X | Y | Z (3 x 12 words for G1, 3 x 24 for G2), what k_mul_batch writes and batch_normalize reads;
// Z = 0 is the identity.  The launch sequence -- permutation, stage 0, stages 1 .. log_n - 1 -- and the two shapes of a stage (a
// butterfly per lane / lane pair, or per team of eight lanes) are described in gntt_plan.h, which api_msm.hip launches from.
//
// The scalar of a butterfly comes from the Fr twiddle table of fr.hip.h (level s at element offset 2^s - 1, entries 2^5 w^j in
// Montgomery form): one Montgomery product with the plain integer 2^-5 gives the canonical w^j, which glv_split / gls_split take.  That is
// under 1 % of the ladder that follows, so there is no second table of recoded digits.  A butterfly with j = 0 goes through the ladder
// like any other (one per block of 2^s: a branch would cost the other lanes of its wavefront the same time).
#pragma once
#include "mulbatch.hip.h"
#include "gntt_plan.h"

namespace bls {

static_assert(GNTT_TEAM_LANES == TEAM, "gntt_plan.h and team.hip.h disagree on the team");
static_assert(TEAM_SLOTS * TeamTraits<FpPolicy>::WORDS == 6 * 14 && TEAM_SLOTS * TeamTraits<Fp2Policy>::WORDS == 6 * 28, "gntt_plan.h sizes the team mailboxes");

// element offset of level s (half-span 2^s) in the Fr twiddle buffer: fr_tw_off of fr.hip.h, which lives in the other translation unit
DEV size_t gn_tw_off(int s) { return ((size_t)1 << s) - 1; }

// table entry 2^5 v R (canonical Montgomery words) -> the canonical integer v, eight words
DEV void gn_scalar(const u32* entry, u32* k) {
  constexpr FrWords c = {BLS_FR_INV_2P5_W};
  Fr u;
#pragma unroll
  for (int i = 0; i < 8; i++) u.l[i] = c.w[i];
  const Fr v = fr_mul(fr_load(entry), u);
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = v.l[i];
}

// whole Fp2 coordinates per lane (the team shape of G2); the lane shapes use MbIO
struct GnIOFp2 {
  static constexpr int WW = 24;
  static DEV Fp2Policy::elem load(const u32* w) { return Fp2Policy::st(fe2_from_ref(w)); }
  template <class T> static DEV void save(const T& a, u32* w) { fe2_to_ref(a, w); }
};
template <class F> struct GnTeamOps {
  u32* mbox; int tl;
  DEV Proj<F> add(const Proj<F>& a, const Proj<F>& b) const { return pt_add_team<F>(a, b, mbox, tl); }
  DEV Proj<F> dbl(const Proj<F>& a) const { return pt_double_team<F>(a, mbox, tl); }
};

// ---- the four shapes of a stage: field policy, wire I/O, lanes per butterfly, point operations -------------------------------------------
struct GnG1Lane {
  typedef FpPolicy F; typedef MbIO<F> IO;
  static constexpr int LANES = 1, GROUP = 1; static constexpr bool TEAMED = false;
  static DEV MbLaneOps<F> ops(u32*) { return MbLaneOps<F>(); }
};
struct GnG2Lane {
  typedef Fp2PairPolicy F; typedef MbIO<F> IO;
  static constexpr int LANES = 2, GROUP = 2; static constexpr bool TEAMED = false;
  static DEV MbLaneOps<F> ops(u32*) { return MbLaneOps<F>(); }
};
struct GnG1Team {
  typedef FpPolicy F; typedef MbIO<F> IO;
  static constexpr int LANES = TEAM, GROUP = 1; static constexpr bool TEAMED = true;
  static DEV GnTeamOps<F> ops(u32* lds) { return GnTeamOps<F>{lds + (threadIdx.x / TEAM) * TEAM_SLOTS * TeamTraits<F>::WORDS, (int)(threadIdx.x & (TEAM - 1))}; }
};
struct GnG2Team {
  typedef Fp2Policy F; typedef GnIOFp2 IO;
  static constexpr int LANES = TEAM, GROUP = 2; static constexpr bool TEAMED = true;
  static DEV GnTeamOps<F> ops(u32* lds) { return GnTeamOps<F>{lds + (threadIdx.x / TEAM) * TEAM_SLOTS * TeamTraits<F>::WORDS, (int)(threadIdx.x & (TEAM - 1))}; }
};

template <class S> DEV Proj<typename S::F> gn_load(const u32* xyz, size_t p) {
  constexpr int WW = S::IO::WW;
  const u32* w = xyz + p * 3 * WW;
  Proj<typename S::F> r;
  r.x = S::IO::load(w); r.y = S::IO::load(w + WW); r.z = S::IO::load(w + 2 * WW);
  return r;
}
template <class S> DEV void gn_save(u32* xyz, size_t p, const Proj<typename S::F>& a) {
  constexpr int WW = S::IO::WW;
  u32* w = xyz + p * 3 * WW;
  S::IO::save(a.x, w); S::IO::save(a.y, w + WW); S::IO::save(a.z, w + 2 * WW);
}
// [v] p for the table entry of v
template <class S, class Ops> DEV Proj<typename S::F> gn_mul(const u32* entry, const Proj<typename S::F>& p, const Ops& op) {
  u32 k[10];
  gn_scalar(entry, k);
  if constexpr (S::GROUP == 1) return mb_ladder_glv(k, p, op);
  else return mb_ladder_gls<typename S::F>(k, p, op);
}

// ---- the permutation pass: point j of every vector <-> point bitrev(j), a lane per point (the lane of the smaller index moves both) -----
// WW = wire words per coordinate.  A record with Z = 0 is rewritten as (0 : 1 : 0): Z = 0 alone is what the interface calls the identity,
// and the complete formulas want a point of the curve.
template <int WW> DEV void gn_canon_identity(u32* w) {
  u32 z = 0;
#pragma unroll
  for (int i = 0; i < WW; i++) z |= w[2 * WW + i];
  if (z) return;
  u32 one[12];
  fe_to_ref(fe_one(), one);
#pragma unroll
  for (int i = 0; i < WW; i++) { w[i] = 0; w[WW + i] = i < 12 ? one[i] : 0; }
}
template <int WW>
__global__ void __launch_bounds__(256) k_gntt_permute(u32* xyz, int log_n, size_t total) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const size_t j = p & (((size_t)1 << log_n) - 1);
  const size_t r = (size_t)(__brevll((unsigned long long)j) >> (64 - log_n));
  if (r < j) return;
  constexpr int Q = 3 * WW / 4;                       // 16-byte pieces of a record
  uint4* pa = reinterpret_cast<uint4*>(xyz) + p * Q;
  uint4* pb = reinterpret_cast<uint4*>(xyz) + (p - j + r) * Q;
  u32 a[3 * WW], b[3 * WW];
#pragma unroll
  for (int i = 0; i < Q; i++) {
    const uint4 u = pa[i], v = pb[i];
    a[4 * i] = u.x; a[4 * i + 1] = u.y; a[4 * i + 2] = u.z; a[4 * i + 3] = u.w;
    b[4 * i] = v.x; b[4 * i + 1] = v.y; b[4 * i + 2] = v.z; b[4 * i + 3] = v.w;
  }
  gn_canon_identity<WW>(a); gn_canon_identity<WW>(b);
#pragma unroll
  for (int i = 0; i < Q; i++) {
    pb[i] = make_uint4(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
    if (r != j) pa[i] = make_uint4(b[4 * i], b[4 * i + 1], b[4 * i + 2], b[4 * i + 3]);
  }
}

// ---- one stage: B butterflies, in place ----------------------------------------------------------------------------------------------------
// Butterfly i of stage s: j = i mod 2^s, a = x[pa], b = x[pa + 2^s] with pa = (i >> s) 2^(s+1) + j;  t = [w_s^j] b,  x[pa] = a + t,
// x[pa + 2^s] = a - t.  Stage 0 has no product (w^0 = 1) unless `ninv` is given (the inverse transform), which makes it
// ([n^-1] a + [n^-1] b, [n^-1] a - [n^-1] b).
// The ladder is inlined ONCE: the loop below runs two rounds over the pair (x, y), and a round multiplies x by its scalar if it has one.
//   round 0   x = b, scalar e0 = the twiddle (stage > 0) or n^-1 (stage 0 of the inverse) or none; then y = x (the finished b side)
//             and x = a, loaded only now, so that the common stage holds ONE point across the ladder, not two
//   round 1   x = a, scalar e1 = n^-1 (stage 0 of the inverse) or none
// y is not live during round 0 (its initial value is never read); after the loop x is the a side and y the b side.
// Team shapes: every lane of a workgroup takes part in the mailbox barriers, so a team beyond B runs on identities and stores nothing.
template <class S>
__global__ void __launch_bounds__(S::TEAMED ? 64 : 256, S::TEAMED ? 1 : 2)
k_gntt_stage(u32* xyz, const u32* __restrict__ tw, const u32* __restrict__ ninv, int stage, size_t B) {
  typedef typename S::F F;
  u32* lds = nullptr;
  if constexpr (S::TEAMED) { BLS_DYN_LDS(team_lds); lds = team_lds; }
  const auto op = S::ops(lds);
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / S::LANES;
  const bool live = i < B;
  if (!S::TEAMED && !live) return;
  const size_t h = (size_t)1 << stage, j = i & (h - 1);
  const size_t pa = ((i >> stage) << (stage + 1)) + j, pb = pa + h;
  const u32* e0 = stage ? tw + (gn_tw_off(stage) + (live ? j : 0)) * 8 : ninv;
  const u32* e1 = stage ? nullptr : ninv;
  Proj<F> x = live ? gn_load<S>(xyz, pb) : pt_identity<F>(), y = x;                // y: assigned in round 0
#pragma nounroll
  for (int r = 0; r < 2; r++) {
    const u32* e = r ? e1 : e0;
    if (e) x = gn_mul<S>(e, x, op);
    if (r == 0) { y = x; x = live ? gn_load<S>(xyz, pa) : pt_identity<F>(); }
  }
  const Proj<F> s = op.add(x, y);
  const Proj<F> d = op.add(x, pt_neg<F>(y));
  if (live && (!S::TEAMED || (threadIdx.x & (TEAM - 1)) == 0)) { gn_save<S>(xyz, pa, s); gn_save<S>(xyz, pb, d); }
}

}  // namespace bls
