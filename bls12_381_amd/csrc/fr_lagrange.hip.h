// fr_lagrange.hip.h -- Lagrange coefficients of many subsets of ARBITRARY nodes in one call, and optionally the interpolated value
// (blsgpu_fr_lagrange_segments[_device]; the coefficient stage of blsgpu_g{1,2}_lagrange_combine).  For segment s with nodes x_i, i < t,
// and point z:
//     N_i = prod_{j != i} (z - x_j)      D_i = prod_{j != i} (x_i - x_j)      lambda_i = N_i * inv0(D_i)      y = sum_i lambda_i v_i
// with inv0(0) = 0 (blsgpu_fr_batch_invert's convention).  The arithmetic is scalar.hip.h's (fr_sub / fr_mul: scalar.rs:420-503) and the
// one inversion per segment is fr_scan.hip.h's frs_inv; what is here is the schedule, whose cut is fr_lagrange_plan.h's.
//
// A team of lanes owns a segment (the plan says which lanes: a whole workgroup, or 8 .. 64 lanes of one wavefront).
//   sweep 1  t^2 products.  Lane l holds R of its nodes x_i (i = k * team + l) in registers; ALL nodes of the segment pass through the
//            team's LDS tile; every lane reads the same x_j at the same time (one broadcast read) and multiplies x_i - x_j into its R
//            running denominators, 1 in place of the factor j == i.  After the last tile:  w_i = z - x_i (1 where it is 0, counted),
//            e_i = w_i D_i, the lane's part of ell' = prod of the non-zero w, and the step of Montgomery's trick over the lane's own
//            non-zero e_i (the product so far goes to `pre`, e_i to `lambda` or scratch).
//   meet     three trees in LDS: ell' and the number nz of nodes that z sits on; the product of all non-zero e_i and the number of
//            zero D_i; ONE frs_inv of that product; the tree walked downward turns it into 1 / (each lane's product).
//   sweep 2  the lane walks its nodes backward: 1 / e_i = pre_i * (inverse so far), and
//                nz = 0   lambda_i = ell' / e_i = ell(z) / ((z - x_i) D_i)            (the barycentric form)
//                nz = 1   lambda_m = ell' / e_m = N_m / D_m at the node z sits on, 0 elsewhere (N_i holds the factor z - x_m = 0)
//                nz > 1   every lambda_i = 0 (z sits on a repeated node: every N_i holds a zero factor)
//            and lambda_i = 0 wherever D_i = 0 (a repeated node), whatever z is.  Every case is the formula above evaluated in another
//            order; field elements are canonical, so the limbs are the formula's.  y is summed per lane, then by a fixed tree.
// t^2 + 7 t products per segment and the trees.  No lane waits for another team, nothing is counted with atomics but the status bit.
//
// -DFLG_FAULT=n builds one of five seeded faults (tests/test_simt_fr_lagrange.py must tell each from the real kernels):
//   1 the factor j == i is replaced by 1 in the first tile only, 2 a point on a node is not recognised (the barycentric form for every z),
//   3 a repeated node is seen only inside the tile that holds it, 4 the WAVE shape reads a whole tile where the segment ends inside it
//   (the next segment's nodes), 5 the y sum drops the lanes that own one node fewer than lane 0.
#pragma once
#include "fr_scan.hip.h"
#include "fr_lagrange_plan.h"

namespace bls {

// the lanes of a team meet: what each wrote to the team's LDS before is visible to all after.  WG: the team is the workgroup.  Else the
// team lies inside one wavefront, whose LDS operations run in program order: the compiler must keep that order, nothing has to wait.
template <bool WG> DEV void flg_meet(unsigned team) {
  if (WG) { __syncthreads(); return; }
#if defined(__HIPCC__)
  (void)team;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  (void)__shfl_up(0, 0u, (int)team);                   // host emulation: a meeting of the team's lane threads
#endif
}
// tree over the team: leaf l is element team + l of tr (8 words each) and of cn; node k holds the product (SUM: the sum) and the count
// of its children 2 k and 2 k + 1; the root is element 1.  The leaves are written by their lanes before the call.
template <bool WG, bool SUM> DEV void flg_up(u32* tr, u32* cn, unsigned team, unsigned l) {
#pragma unroll 1
  for (unsigned n = team >> 1; n >= 1; n >>= 1) {
    flg_meet<WG>(team);
    if (l < n) {
      const unsigned k = n + l;
      const Fr a = fr_load(tr + (size_t)(2 * k) * 8), b = fr_load(tr + (size_t)(2 * k + 1) * 8);
      fr_store(tr + (size_t)k * 8, SUM ? fr_add(a, b) : frs_mul(a, b));
      cn[k] = cn[2 * k] + cn[2 * k + 1];
    }
  }
  flg_meet<WG>(team);
}
// the root holds the inverse of what it held: every node, then every leaf, gets the inverse of what it held
template <bool WG> DEV void flg_down(u32* tr, unsigned team, unsigned l) {
#pragma unroll 1
  for (unsigned n = 1; n < team; n <<= 1) {
    if (l < n) {
      const unsigned k = n + l;
      const Fr iv = fr_load(tr + (size_t)k * 8), a = fr_load(tr + (size_t)(2 * k) * 8), b = fr_load(tr + (size_t)(2 * k + 1) * 8);
      fr_store(tr + (size_t)(2 * k) * 8, frs_mul(iv, b));
      fr_store(tr + (size_t)(2 * k + 1) * 8, frs_mul(iv, a));
    }
    flg_meet<WG>(team);
  }
}

// R: nodes per lane per pass; WG: the BLOCK shape (team == blockDim.x).  work: the factors e_i when lambda is NULL; pre: the running
// products.  Both are addressed like lambda, by node.  lambda and work are the same array to this kernel: no __restrict__ on them.
template <int R, bool WG>
__global__ void __launch_bounds__(FLG_BLOCK) k_flg_segments(const u32* __restrict__ nodes, const u32* __restrict__ offsets, u32 nseg, u32 total, const u32* __restrict__ points,
                                                            const u32* __restrict__ values, u32* lambda, u32* __restrict__ y, uint8_t* __restrict__ flags, u32* work,
                                                            u32* __restrict__ pre, u32 team, u32 tile, u32* __restrict__ status) {
  BLS_DYN_LDS(flg_lds);
  const u32 teams = blockDim.x / team, tm = threadIdx.x / team, l = threadIdx.x % team;
  const size_t s = (size_t)blockIdx.x * teams + tm;
  if (s >= nseg) return;                                 // (every exit before the first meeting is taken by the whole team)
  u32 so = 0, t = 0;
  if (!flg_segment(offsets, total, s, &so, &t)) { if (l == 0) atomicOr(status, FLG_STATUS_BAD); return; }
  if (t == 0) {
    if (l == 0) { if (y) fr_store(y + s * 8, fr_zero()); if (flags) flags[s] = 1; }
    return;
  }
  u32* tl = flg_lds + (size_t)tm * flg_team_lds_words(team, tile);
  u32* tr = tl + (size_t)tile * 8;
  u32* cn = tr + (size_t)2 * team * 8;
  const Fr one = fr_one();
  const Fr z = points ? fr_load(points + s * 8) : fr_zero();
  const u32* x = nodes + (size_t)so * 8;
  u32* W = (lambda ? lambda : work) + (size_t)so * 8;
  u32* P = pre + (size_t)so * 8;
  Fr run = one, ell = one;
  u32 nz = 0, nd = 0;
  const u32 passes = flg_passes(t, team, R), tiles = flg_tiles(t, tile);
  // ---- sweep 1 ----
#pragma unroll 1
  for (u32 p = 0; p < passes; p++) {
    Fr xi[R], d[R];
    u32 idx[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      idx[r] = flg_node(p * R + r, l, team);
      xi[r] = idx[r] < t ? fr_load(x + (size_t)idx[r] * 8) : fr_zero();
      d[r] = one;
    }
#pragma unroll 1
    for (u32 q = 0; q < tiles; q++) {
      const u32 base = q * tile;
#if defined(FLG_FAULT) && FLG_FAULT == 4
      const u32 left = WG ? t - base : total - so - base;
#else
      const u32 left = t - base;
#endif
      const u32 cnt = left < tile ? left : tile;
      flg_meet<WG>(team);                                // the tile is free again
      for (u32 w = l; w < 2 * cnt; w += team) reinterpret_cast<uint4*>(tl)[w] = reinterpret_cast<const uint4*>(x + (size_t)base * 8)[w];
      flg_meet<WG>(team);
#pragma unroll 1
      for (u32 j = 0; j < cnt; j++) {
        const Fr xj = fr_load(tl + (size_t)j * 8);       // the same address in every lane: a broadcast
#pragma unroll
        for (int r = 0; r < R; r++) {
          if (idx[r] < t) {
            Fr f = fr_sub(xi[r], xj);
#if defined(FLG_FAULT) && FLG_FAULT == 1
            if (base + j == idx[r] && q == 0) f = one;
#else
            if (base + j == idx[r]) f = one;
#endif
#if defined(FLG_FAULT) && FLG_FAULT == 3
            if (q != idx[r] / tile && fr_is_zero(f)) f = one;
#endif
            d[r] = fr_mul(d[r], f);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (idx[r] < t) {
        Fr w = fr_sub(z, xi[r]);
        if (fr_is_zero(w)) { nz++; w = one; }
        ell = frs_mul(ell, w);
        const Fr e = frs_mul(w, d[r]);                   // 0 exactly where D_i = 0
        fr_store(P + (size_t)idx[r] * 8, run);
        fr_store(W + (size_t)idx[r] * 8, e);
        if (fr_is_zero(e)) nd++; else run = frs_mul(run, e);
      }
    }
  }
  // ---- meet ----
  fr_store(tr + (size_t)(team + l) * 8, ell); cn[team + l] = nz;
  flg_up<WG, false>(tr, cn, team, l);
  const Fr ell_all = fr_load(tr + 8);
#if defined(FLG_FAULT) && FLG_FAULT == 2
  const u32 nz_all = 0;
#else
  const u32 nz_all = cn[1];
#endif
  flg_meet<WG>(team);
  fr_store(tr + (size_t)(team + l) * 8, run); cn[team + l] = nd;
  flg_up<WG, false>(tr, cn, team, l);
  const Fr prod_all = fr_load(tr + 8);
  const u32 nd_all = cn[1];
  flg_meet<WG>(team);
  if (!WG || threadIdx.x < FLG_WAVE) {                   // one wavefront inverts, every lane of it with the same value
    const Fr inv = frs_inv(prod_all);
    if (l == 0) fr_store(tr + 8, inv);
  }
  flg_meet<WG>(team);
  flg_down<WG>(tr, team, l);
  Fr rinv = fr_load(tr + (size_t)(team + l) * 8);        // 1 / (the product of the lane's non-zero e_i)
  // ---- sweep 2 ----
  Fr ysum = fr_zero();
#pragma unroll 1
  for (u32 k = flg_count(t, l, team); k-- > 0;) {
    const u32 i = flg_node(k, l, team);
    const Fr e = fr_load(W + (size_t)i * 8);
    Fr lam = fr_zero();
    if (!fr_is_zero(e)) {
      const Fr inv = frs_mul(fr_load(P + (size_t)i * 8), rinv);
      rinv = frs_mul(rinv, e);
      if (nz_all == 0) lam = frs_mul(ell_all, inv);
      else if (nz_all == 1 && fr_is_zero(fr_sub(z, fr_load(x + (size_t)i * 8)))) lam = frs_mul(ell_all, inv);
    }
    if (lambda) fr_store(lambda + ((size_t)so + i) * 8, lam);
    if (y) ysum = fr_add(ysum, frs_mul(lam, fr_load(values + ((size_t)so + i) * 8)));
  }
  if (y) {
#if defined(FLG_FAULT) && FLG_FAULT == 5
    if (flg_count(t, l, team) != flg_count(t, 0, team)) ysum = fr_zero();
#endif
    fr_store(tr + (size_t)(team + l) * 8, ysum); cn[team + l] = 0;
    flg_up<WG, true>(tr, cn, team, l);
    if (l == 0) fr_store(y + s * 8, fr_load(tr + 8));
  }
  if (flags && l == 0) flags[s] = nd_all == 0 ? 1 : 0;
}

}  // namespace bls
