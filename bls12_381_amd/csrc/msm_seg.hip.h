// msm_seg.hip.h -- segmented MSM: k independent small MSMs  out[j] = sum_{i < len_j} s[offsets[j] + i] * P[base_first[j] + i]  in two
// launches, for any k (api_msm.hip: blsgpu_g{1,2}_msm_segments*).
//
// The pipeline of msm.hip.h is shaped for ONE large MSM: a dozen launches, a global sort and a latency-bound tail per call.  A segment
// of tens to thousands of points needs none of that:
//
//   k_msm_seg_accumulate  one workgroup per (segment, window group).  c = 4-bit signed windows, 8 buckets per window; every
//                         accumulator (window, bucket) belongs to one lane (G1) or one lane pair (G2, pairlane.hip.h), 256 lanes per
//                         workgroup.  The segment is walked in chunks of SEG_CHUNK scalars: decompose (GLV / psi split or plain),
//                         counting-sort the chunk's (window, |digit|) entries in LDS, and every accumulator walks its own list with the
//                         XYZZ mixed addition (exceptional cases exact, as in k_msm_accumulate).  After the last chunk the 8 bucket
//                         lanes of a window form  sum_b b * B_b  by shuffles (suffix sums, then a tree) and write one window sum.
//   k_msm_seg_combine     one lane (pair) per segment: Horner over the window sums (4 doublings + 1 addition per window), the same
//                         schedule in every lane.  A launch of its own: its ~128-250 dependent doublings would otherwise hold the issue
//                         slots of a whole accumulation workgroup for one lane's work.
//
// Windows per scalar: G1 GLV 2 x 127-bit halves -> 32 windows (one group of 32); G2 psi split 4 x 63-bit digits -> 16 windows (one
// group of 16 on lane pairs); plain 256-bit scalars -> 64 windows (G1: 2 groups, G2: 4 groups, each workgroup recomputes the digits
// of the windows below its own to carry the signed recoding).
#pragma once
#include "msm.hip.h"

namespace bls {

constexpr int SEG_C = 4;                      // window bits
constexpr int SEG_NB = 1 << (SEG_C - 1);      // buckets per window (signed digits, |d| in 1..8)
constexpr int SEG_CHUNK = 128;                // scalars sorted in LDS at a time
constexpr int SEG_THREADS = 256;
constexpr u32 SEG_STATUS_BAD = 8u;            // d_status bit: a segment broke the offsets / length / base-range contract (device form)
enum { SEG_PLAIN = 0, SEG_GLV = 1, SEG_GLS = 2 };

template <class F, int MODE> struct SegCfg {
  static constexpr int LPA = std::is_same<F, FpPolicy>::value ? 1 : 2;     // lanes per accumulator
  static constexpr int NACC = SEG_THREADS / LPA;                            // accumulators per workgroup
  static constexpr int WB = NACC / SEG_NB;                                  // windows per workgroup
  static constexpr int S = MODE == SEG_GLV ? 2 : MODE == SEG_GLS ? 4 : 1;   // sub-scalars per scalar
  static constexpr int DW = 8 / S;                                          // words per sub-scalar (DigitIter<DW>)
  static constexpr int NWIN = (32 * DW + SEG_C - 1) / SEG_C;                // windows per sub-scalar
  static constexpr int NGRP = NWIN / WB;                                    // workgroups per segment
  static constexpr int MAXENT = SEG_CHUNK * S * WB;                         // entries of one chunk, at most
  static_assert(NWIN % WB == 0 && NACC % 64 == 0, "segment window layout");
};

// the Proj of the lane `d` above (within groups of `width` lanes); every lane executes it
template <class F> DEV Proj<F> seg_shfl_down(const Proj<F>& p, int d, int width) {
  static_assert(sizeof(Proj<F>) % 4 == 0, "Proj layout");
  constexpr int W = sizeof(Proj<F>) / 4;
  const u32* s = reinterpret_cast<const u32*>(&p);
  Proj<F> r;
  u32* o = reinterpret_cast<u32*>(&r);
#pragma unroll
  for (int i = 0; i < W; i++) o[i] = (u32)__shfl_down((int)s[i], (unsigned)d, width);
  return r;
}

// F = FpPolicy (G1) or Fp2PairPolicy (G2 on lane pairs).  wsums[(j - seg0) * NWIN + w] = window sum w of segment j (PROJ records).
template <class F, int MODE>
__global__ void __launch_bounds__(SEG_THREADS, 2) k_msm_seg_accumulate(const u32* __restrict__ rec, const u32* __restrict__ endo, size_t nbases,
                                                                      const u32* __restrict__ base_first, const u32* __restrict__ offsets,
                                                                      const u32* __restrict__ scalars, u32 seg0, u32 total, int form,
                                                                      u32* __restrict__ status, u32* __restrict__ wsums) {
  typedef SegCfg<F, MODE> C;
  constexpr bool G1 = C::LPA == 1;
  constexpr int AW = G1 ? Store<FpPolicy>::AFF_WORDS : Store<Fp2Policy>::AFF_WORDS;
  constexpr int PW = G1 ? Store<FpPolicy>::PROJ_WORDS : Store<Fp2Policy>::PROJ_WORDS;
  __shared__ __align__(16) u32 sc[SEG_CHUNK * 8];       // the chunk's sub-scalars, 8 words per scalar
  __shared__ u32 ent[C::MAXENT];                        // sorted entries: chunk item (scalar * S + sub) | sign << 31
  __shared__ u32 cnt[C::NACC], beg[C::NACC], cur[C::NACC];
  const u32 tid = threadIdx.x;
  const u32 seg_local = blockIdx.x / C::NGRP;
  const int w0 = (int)(blockIdx.x % C::NGRP) * C::WB;
  const u32 seg = seg0 + seg_local;
  // the segment (every lane reads the same words); a segment that breaks the contract is reported and treated as empty
  const u32 o0 = offsets[seg], o1 = offsets[seg + 1];
  const u32 bf = base_first ? base_first[seg] : o0;
  u32 len = o1 - o0;
  if (o1 < o0 || len > SEG_LEN_MAX || o1 > total || (size_t)bf + len > nbases) {
    if (tid == 0 && w0 == 0) atomicOr(status, SEG_STATUS_BAD);
    len = 0;
  }
  const u32 a = tid / C::LPA;                           // this lane's accumulator: window a / SEG_NB of the group, bucket a % SEG_NB
  const u32 par = tid & 1;                              // (G2) the Fp2 coefficient this lane holds
  auto rec_of = [&](u32 item, u32 c0) -> const u32* {
    const size_t p = (size_t)bf + c0 + item / C::S;
    if constexpr (MODE == SEG_GLV) return ((item & 1) ? endo : rec) + p * AW;
    else if constexpr (MODE == SEG_GLS) return endo + (4 * p + (item & 3)) * AW;
    else return rec + p * AW;
  };
  Xyzz<F> acc;
  acc.x = F::zero(); acc.y = F::zero(); acc.zz = F::zero(); acc.zzz = F::zero();
  bool acc_inf = true;
  for (u32 c0 = 0; c0 < len; c0 += SEG_CHUNK) {
    const u32 m = len - c0 < (u32)SEG_CHUNK ? len - c0 : (u32)SEG_CHUNK;
    // 1. scalars -> sub-scalars (canonical check, Montgomery form reduced by scalar_load)
    if (tid < (u32)SEG_CHUNK) {
      u32 o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (tid < m) {
        u32 k[10];
        if (!scalar_load(scalars, (size_t)o0 + c0 + tid, form, k)) atomicOr(status, 1u);
        if constexpr (MODE == SEG_GLV) glv_split(k, o, o + 4);
        else if constexpr (MODE == SEG_GLS) {
          k[8] = 0; k[9] = 0;
          u64 d[4]; u32 sb[4];
          gls_split(k, d, sb);
#pragma unroll
          for (int j = 0; j < 4; j++) { o[2 * j] = (u32)d[j]; o[2 * j + 1] = (u32)(d[j] >> 32) | (sb[j] << 31); }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) o[j] = k[j];
        }
      }
      uint4* dst = reinterpret_cast<uint4*>(sc + tid * 8);
      dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
      dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
    for (u32 i = tid; i < (u32)C::NACC; i += SEG_THREADS) cnt[i] = 0;
    __syncthreads();
    // 2. count the chunk's entries per (window, |digit|); 4. place them (the same digits again, ranked by an LDS atomic)
    auto digits = [&](auto&& put) {
      for (u32 it = tid; it < m * C::S; it += SEG_THREADS) {
        DigitIter<C::DW> d;
        d.init(sc + (it / C::S) * 8, it % C::S, SEG_C);
        u32 mag, neg;
        for (int w = 0; w < w0; w++) d.next(mag, neg);
#pragma unroll
        for (int w = 0; w < C::WB; w++) {
          d.next(mag, neg);
          if (mag) put((u32)w * SEG_NB + mag - 1, it | (neg << 31));
        }
      }
    };
    digits([&](u32 key, u32) { atomicAdd(&cnt[key], 1u); });
    __syncthreads();
    // 3. exclusive scan of the counters by the first wavefront
    if (tid < 64) {
      constexpr int PER = C::NACC / 64;
      u32 v[PER], s = 0;
#pragma unroll
      for (int j = 0; j < PER; j++) { v[j] = cnt[tid * PER + j]; s += v[j]; }
      u32 incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { u32 t = (u32)__shfl_up((int)incl, (unsigned)d, 64); if (tid >= (u32)d) incl += t; }
      u32 ex = incl - s;
#pragma unroll
      for (int j = 0; j < PER; j++) { beg[tid * PER + j] = ex; cur[tid * PER + j] = ex; ex += v[j]; }
    }
    __syncthreads();
    digits([&](u32 key, u32 e) { ent[atomicAdd(&cur[key], 1u)] = e; });
    __syncthreads();
    // 5. every accumulator walks its own list (the lanes of a wavefront in lockstep); the record of the next entry is in flight
    //    while the current one is added (index clamped to the list's last entry: an unconditional load)
    const u32 s0 = beg[a], s1 = cur[a];
    if (s0 < s1) {
      if constexpr (G1) {
        u32 e = ent[s0];
        Aff<F> q; u32 inf;
        load_aff_word<F>(rec_of(e & 0x7fffffffu, c0), q, inf);
        for (u32 j = s0; j < s1; j++) {
          const u32 en = ent[j + 1 < s1 ? j + 1 : j];
          Aff<F> qn; u32 infn;
          load_aff_word<F>(rec_of(en & 0x7fffffffu, c0), qn, infn);
          if (inf == 0) acc = xyzz_add_mixed_inl(acc, acc_inf, q.x, cond_neg(q.y, (e >> 31) != 0));
          q = qn; inf = infn; e = en;
        }
      } else {
        // this lane's halves of a record: x coefficient `par`, y coefficient `par`, and the identity flag (k_msm_accumulate_g2pair)
        auto load_half = [&](const u32* r, FeP<1, 1>& qx, FeP<1, 1>& qy, u32& flag) {
          const uint2* px = reinterpret_cast<const uint2*>(r + par * NL);
          const uint2* py = reinterpret_cast<const uint2*>(r + 2 * NL + par * NL);
#pragma unroll
          for (int i = 0; i < NL / 2; i++) {
            uint2 u = px[i], v = py[i];
            qx.v.l[2 * i] = u.x; qx.v.l[2 * i + 1] = u.y; qy.v.l[2 * i] = v.x; qy.v.l[2 * i + 1] = v.y;
          }
          flag = r[4 * NL];
        };
        // madd-2008-s, generic case only (k_msm_accumulate_g2pair): when P = U2 - X MAY be zero the pair finishes the list with the
        // complete mixed addition and converts back to XYZZ.  Every decision is the same in both lanes of the pair.
        u32 j = s0;
        for (; j < s1; j++) {
          const u32 e = ent[j];
          FeP<1, 1> qx, qy1; u32 flag;
          load_half(rec_of(e & 0x7fffffffu, c0), qx, qy1, flag);
          if (flag != 0) continue;                      // identity base
          FeP<2, 2> qy = select((e >> 31) != 0, neg(qy1), (FeP<2, 2>)qy1);
          if (acc_inf) { acc_inf = false; acc = xyzz_from_affine<F>(qx, qy); continue; }
          auto U2 = mul(qx, acc.zz);
          auto S2 = mul(qy, acc.zzz);
          auto P = norm(sub(U2, acc.x));
          auto R = norm(sub(S2, acc.y));
          {
            bool mz = maybe_zero(P.v);
            bool pm = partner_flag(mz);
            if (mz && pm) break;                        // entry j is NOT consumed
          }
          auto PP = sqr(P);
          auto PPP = mul(P, PP);
          auto Q = mul(acc.x, PP);
          auto X3 = norm(sub(sqr(R), add(PPP, dbl(Q))));
          auto Y3 = sub(mul(R, norm(sub(Q, X3))), mul(acc.y, PPP));
          auto ZZ3 = mul(acc.zz, PP);
          auto ZZZ3 = mul(acc.zzz, PPP);
          acc.x = F::st(X3); acc.y = F::st(Y3); acc.zz = F::st(ZZ3); acc.zzz = F::st(ZZZ3);
        }
        if (j < s1) {
          Proj<F> pr = xyzz_to_proj<F>(acc, acc_inf);
          for (; j < s1; j++) {
            const u32 e = ent[j];
            FeP<1, 1> qx, qy1; u32 flag;
            load_half(rec_of(e & 0x7fffffffu, c0), qx, qy1, flag);
            if (flag != 0) continue;
            FeP<2, 2> qy = select((e >> 31) != 0, neg(qy1), (FeP<2, 2>)qy1);
            pr = pt_add_mixed_y<F>(pr, qx, qy);
          }
          // (X : Y : Z) -> XYZZ (X Z, Y Z^2, Z^2, Z^3)
          acc_inf = is_zero(pr.z);
          auto zz = F::st(sqr(pr.z));
          acc.x = F::st(mul(pr.x, pr.z)); acc.y = F::st(mul(pr.y, zz)); acc.zzz = F::st(mul(zz, pr.z)); acc.zz = zz;
        }
      }
    }
    __syncthreads();                                    // the LDS of this chunk is rewritten by the next one
  }
  // sum_b (b + 1) B_b over the SEG_NB bucket lanes of every window: suffix sums S_b = sum_{b' >= b} B_b', then sum_b S_b
  Proj<F> B = xyzz_to_proj<F>(acc, acc_inf);
  const u32 b = a % SEG_NB;
  constexpr int WIDTH = SEG_NB * C::LPA;
#pragma unroll
  for (int d = 1; d < SEG_NB; d <<= 1) {
    Proj<F> o = seg_shfl_down<F>(B, d * C::LPA, WIDTH);
    if (b + d < (u32)SEG_NB) B = pt_add<F>(B, o);
  }
#pragma unroll
  for (int d = 1; d < SEG_NB; d <<= 1) {
    Proj<F> o = seg_shfl_down<F>(B, d * C::LPA, WIDTH);
    if ((b & (2 * d - 1)) == 0) B = pt_add<F>(B, o);
  }
  if (b == 0) {
    u32* out = wsums + ((size_t)seg_local * C::NWIN + w0 + a / SEG_NB) * PW;
    if constexpr (G1) store_proj<F>(out, B);
    else store_proj_pair(out, par, B);
  }
}

// Horner over the window sums of nseg segments: rec[j] = sum_w 2^(4 w) wsums[j * NWIN + w]
template <class F, int NWIN>
__global__ void __launch_bounds__(256) k_msm_seg_combine(const u32* __restrict__ wsums, u32* __restrict__ rec, u32 nseg) {
  constexpr bool G1 = std::is_same<F, FpPolicy>::value;
  constexpr int PW = G1 ? Store<FpPolicy>::PROJ_WORDS : Store<Fp2Policy>::PROJ_WORDS;
  const u32 t = (blockIdx.x * blockDim.x + threadIdx.x) / (G1 ? 1 : 2);
  if (t >= nseg) return;                                // (both lanes of a pair leave together)
  const u32 par = threadIdx.x & 1;
  auto load = [&](int w, Proj<F>& p) {
    const u32* r = wsums + ((size_t)t * NWIN + w) * PW;
    if constexpr (G1) load_proj<F>(r, p); else load_proj_pair(r, par, p);
  };
  Proj<F> acc;
  load(NWIN - 1, acc);
  for (int w = NWIN - 2; w >= 0; w--) {
#pragma unroll
    for (int i = 0; i < SEG_C; i++) acc = pt_double<F>(acc);
    Proj<F> s; load(w, s);
    acc = pt_add<F>(acc, s);
  }
  if constexpr (G1) store_proj<F>(rec + (size_t)t * PW, acc);
  else store_proj_pair(rec + (size_t)t * PW, par, acc);
}

}  // namespace bls
