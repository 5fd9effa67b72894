// lagrange_combine.hip.h -- the last stage of blsgpu_g{1,2}_lagrange_combine[_device]: out[s] = the sum of the products
// lambda_i * P_i of segment s, which k_mul_batch left as projective wire points in scratch.
//
// Not k_gsum_chunks: that kernel takes AFFINE points (a batch_normalize of every product would sit in between), u64 offsets, and can
// not leave a segment that breaks the offsets contract untouched while its neighbours stay right -- what this call promises, as the
// coefficient stage does (fr_lagrange_plan.h: flg_segment; that stage has raised the status bit already).  The additions are the same
// COMPLETE formula (curve.hip.h pt_add, g1.rs:670-712): identities among the products, equal products and opposite ones need no case.
// One workgroup per segment: lane l adds the products l, l + B, ...; the lanes meet in a tree in LDS, as in k_gsum_combine.
#pragma once
#include "msm.hip.h"
#include "fr_lagrange_plan.h"

namespace bls {

// LDS: blockDim.x records of Store<F>::PROJ_WORDS
template <class F>
__global__ void __launch_bounds__(256) k_flg_point_sums(const u32* __restrict__ prod, const u32* __restrict__ offsets, u32 nseg, u32 total, u32* __restrict__ out) {
  BLS_DYN_LDS(flgs_lds);
  constexpr int WW = Wire<F>::WORDS, PW = Store<F>::PROJ_WORDS;
  const u32 B = blockDim.x, l = threadIdx.x;
  const size_t s = blockIdx.x;
  if (s >= nseg) return;
  u32 so = 0, t = 0;
  if (!flg_segment(offsets, total, s, &so, &t)) return;        // nothing of it is written
  Proj<F> acc = pt_identity<F>();
  for (u32 k = l; k < t; k += B) {
    const u32* w = prod + ((size_t)so + k) * 3 * WW;
    Proj<F> p;
    p.x = F::st(Wire<F>::load(w)); p.y = F::st(Wire<F>::load(w + WW)); p.z = F::st(Wire<F>::load(w + 2 * WW));
    acc = pt_add<F>(acc, p);
  }
  store_proj<F>(flgs_lds + (size_t)l * PW, acc);
  __syncthreads();
  for (u32 d = B >> 1; d >= 1; d >>= 1) {
    if (d >= t) continue;                                      // the lanes from d on hold identities
    if (l < d) {
      Proj<F> o; load_proj<F>(flgs_lds + (size_t)(l + d) * PW, o);
      acc = pt_add<F>(acc, o);
      store_proj<F>(flgs_lds + (size_t)l * PW, acc);
    }
    __syncthreads();
  }
  if (l == 0) {
    u32* o = out + s * 3 * WW;
    Wire<F>::save(acc.x, o); Wire<F>::save(acc.y, o + WW); Wire<F>::save(acc.z, o + 2 * WW);
  }
}

}  // namespace bls
