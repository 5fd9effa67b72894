// gsum.hip.h -- segmented, gathered point sums: out[s] = sum of the points idx[t], t in [offsets[s], offsets[s + 1]), for many
// segments of any length in one call (blsgpu_g{1,2}_sum_segments[_device]).
//
// Reference: `impl Sum for G1Projective` (src/g1.rs:161-171: a fold of `+` from `identity()`), the same for G2 (src/g2.rs); the terms
// are `G1Affine` values, so every step is the reference's `add_mixed` (g1.rs:715-752, RCB15 Algorithm 8) and the partial sums meet in
// `add` (:670-712, Algorithm 7).  Both are the COMPLETE formulas of curve.hip.h: a repeated index doubles, P + (-P) gives (0 : y : 0),
// an identity term is skipped by its flag, a point outside the subgroup adds like any curve point -- no exceptional case anywhere, so
// the lanes of a wavefront never diverge over the VALUES they add.  The projective representative depends on the cut; the group
// element does not (results are compared after batch_normalize, as for mul_batch).
//
// The cut, the records and the jobs are gsum_plan.h's; this file holds the two kernels.  Points arrive in the public affine wire
// format (two coordinates of 6 u64 Montgomery limbs + an infinity byte) and are converted as they are gathered; the partial records of
// the scratch are the resident form of msm.hip.h (load_proj / store_proj); the sums leave in the projective wire format.
//
// -DGSUM_FAULT=n builds one of four seeded faults (tests/test_simt_gsum.py must tell each from the real kernels):
//   1 the last term of a chunk is dropped, 2 the combine pass skips a segment's first partial, 3 the identity flag is ignored,
//   4 the head of a lane's slice never reaches the lane before it.
#pragma once
#include "msm.hip.h"
#include "gsum_plan.h"

namespace bls {

template <class F> DEV void gsum_write_out(u32* __restrict__ out, u32 s, const Proj<F>& p) {
  constexpr int WW = Wire<F>::WORDS;
  u32* o = out + (size_t)s * 3 * WW;
  Wire<F>::save(p.x, o); Wire<F>::save(p.y, o + WW); Wire<F>::save(p.z, o + 2 * WW);
}

// pass 1: a workgroup per chunk.  LDS: blockDim.x records, then blockDim.x keys, then blockDim.x head flags.
template <class F>
__global__ void __launch_bounds__(256) k_gsum_chunks(const u32* __restrict__ xy, const uint8_t* __restrict__ inf, u32 npoints, const u32* __restrict__ idx,
                                                     const unsigned long long* __restrict__ offsets, u32 nseg, u32 total, u32 terms, u32* __restrict__ out,
                                                     u32* __restrict__ part, u32* __restrict__ meta, u32* __restrict__ status) {
  BLS_DYN_LDS(gsum_lds);
  constexpr int WW = Wire<F>::WORDS, PW = Store<F>::PROJ_WORDS;
  const u32 B = blockDim.x, l = threadIdx.x;
  const size_t c = blockIdx.x;
  const u32 chunk = B * terms, cb = (u32)c * chunk, ce = total - cb < chunk ? total : cb + chunk;
  u32* recs = gsum_lds;
  u32* keys = gsum_lds + (size_t)B * PW;
  u32* heads = keys + B;
  const u32 b = (size_t)cb + (size_t)l * terms < ce ? cb + l * terms : ce, e = ce - b < terms ? ce : b + terms;
  const bool active = b < e;
  u32 s = GSUM_NONE;
  bool has_head = false;
  Proj<F> acc = pt_identity<F>();
  if (active) {
    s = gsum_seg_of(offsets, nseg, total, b);
    const u32 first = s;
    u32 send = gsum_off(offsets, nseg, total, s + 1);
#if defined(GSUM_FAULT) && GSUM_FAULT == 1
    const u32 stop = e == ce ? e - 1 : e;
#else
    const u32 stop = e;
#endif
    for (u32 t = b; t < stop; t++) {
      if (t >= send) {
        // segment s ends inside this slice.  It began before the slice: the lane before this one holds the rest (lane 0: the chunk
        // before this one does, and this is the chunk's HEAD partial).  It began in the slice: it is whole.
        const u32 so = gsum_off(offsets, nseg, total, s);
        if (s == first && so < b) {
          if (l == 0) store_proj<F>(part + gsum_record(c, so, cb) * PW, acc);
          else { store_proj<F>(recs + (size_t)l * PW, acc); has_head = true; }
        } else {
          gsum_write_out<F>(out, s, acc);
        }
        acc = pt_identity<F>();
        do { s++; send = gsum_off(offsets, nseg, total, s + 1); } while (t >= send);          // off(nseg) = total > t ends it
      }
      const u32 p = idx ? idx[t] : t;
      if (p >= npoints) { atomicOr(status, GSUM_STATUS_BAD); continue; }                       // never dereferenced
      Aff<F> q;
      q.x = Wire<F>::load(xy + (size_t)p * 2 * WW);
      q.y = Wire<F>::load(xy + (size_t)p * 2 * WW + WW);
#if defined(GSUM_FAULT) && GSUM_FAULT == 3
      const bool q_inf = false;
#else
      const bool q_inf = inf[p] != 0;
#endif
      acc = pt_add_mixed<F>(acc, q, q_inf);
    }
  }
  keys[l] = s;
  heads[l] = has_head ? 1u : 0u;
  if (active && l == 0) meta[2 * c] = gsum_seg_of(offsets, nseg, total, cb);
  if (active && e == ce) meta[2 * c + 1] = s;
  __syncthreads();
  // the head of the next lane's slice belongs to the segment this lane ends in (its term b - 1 is this lane's last)
#if !(defined(GSUM_FAULT) && GSUM_FAULT == 4)
  if (active && l + 1 < B && heads[l + 1]) {
    Proj<F> h; load_proj<F>(recs + (size_t)(l + 1) * PW, h);
    acc = pt_add<F>(acc, h);
  }
#endif
  __syncthreads();
  if (active) store_proj<F>(recs + (size_t)l * PW, acc);
  __syncthreads();
  // segmented tree: after the step with distance d, lane l holds the sum of the lanes l .. l + 2 d - 1 that share its key
  for (u32 d = 1; d < B; d <<= 1) {
    const bool take = active && l + d < B && keys[l + d] == s;
    Proj<F> o;
    if (take) load_proj<F>(recs + (size_t)(l + d) * PW, o);
    __syncthreads();
    if (take) { acc = pt_add<F>(acc, o); store_proj<F>(recs + (size_t)l * PW, acc); }
    __syncthreads();
  }
  // the first lane of every run of equal keys holds the run's sum
  if (active && (l == 0 || keys[l - 1] != s)) {
    const u32 so = gsum_off(offsets, nseg, total, s), se = gsum_off(offsets, nseg, total, s + 1);
    if (gsum_inside(so, se, cb, chunk)) gsum_write_out<F>(out, s, acc);
    else store_proj<F>(part + gsum_record(c, so, cb) * PW, acc);
  }
}

// pass 2: job blockIdx.x of gsum_plan.h, and the identity for the empty segments.  LDS: blockDim.x records.
template <class F>
__global__ void __launch_bounds__(256) k_gsum_combine(const unsigned long long* __restrict__ offsets, u32 nseg, u32 total, u32 chunk, size_t nchunks,
                                                      const u32* __restrict__ part, const u32* __restrict__ meta, u32* __restrict__ out) {
  BLS_DYN_LDS(gsum_lds);
  constexpr int PW = Store<F>::PROJ_WORDS;
  const u32 B = blockDim.x, l = threadIdx.x;
  const size_t j = blockIdx.x;
  {
    const size_t i = j * B + l;
    if (i < nseg && gsum_off(offsets, nseg, total, (u32)i) >= gsum_off(offsets, nseg, total, (u32)i + 1)) gsum_write_out<F>(out, (u32)i, pt_identity<F>());
  }
  if (j >= 2 * nchunks) return;
  const size_t c = j >> 1;
  u32 s = 0; size_t c_last = 0;
  if (!gsum_job(offsets, nseg, total, chunk, c, (int)(j & 1), meta[2 * c], meta[2 * c + 1], &s, &c_last)) return;      // the same answer in every lane
  const size_t count = c_last - c + 1;                       // this chunk's record, then the HEAD records of the chunks behind it
  Proj<F> acc = pt_identity<F>();
#if defined(GSUM_FAULT) && GSUM_FAULT == 2
  for (size_t k = l ? l : B; k < count; k += B) {
#else
  for (size_t k = l; k < count; k += B) {
#endif
    Proj<F> p; load_proj<F>(part + (k ? 2 * (c + k) : j) * PW, p);
    acc = pt_add<F>(acc, p);
  }
  store_proj<F>(gsum_lds + (size_t)l * PW, acc);
  __syncthreads();
  for (u32 d = B >> 1; d >= 1; d >>= 1) {
    if (d >= count) continue;                                // the lanes from d on hold identities
    if (l < d) {
      Proj<F> o; load_proj<F>(gsum_lds + (size_t)(l + d) * PW, o);
      acc = pt_add<F>(acc, o);
      store_proj<F>(gsum_lds + (size_t)l * PW, acc);
    }
    __syncthreads();
  }
  if (l == 0) gsum_write_out<F>(out, s, acc);
}

}  // namespace bls
