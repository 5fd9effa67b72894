// fr_poseidon.hip.h -- Poseidon over Fr: permutations, fixed-length hashes and Merkle levels (blsgpu_fr_poseidon_*).
//
// The instance (width, rounds, constants, matrix) is the caller's; fr_poseidon_plan.h validates it, derives the sparse form of the partial
// rounds and builds the constant image read here, already in the 9 x 29-bit lazy limbs of fr.hip.h and pre-scaled for the 2^5 every
// frl_mul leaves behind (the table of scales is at the head of fr_poseidon_plan.h).  Nothing but products: 604 (t = 3) to 3043
// (t = 12) field products per permutation in the sparse form at (8, 57) rounds, for 100 to 400 bytes moved.
//
// Mapping: ONE STATE PER LANE for every width, the state in registers.  Every index into the image is wave-uniform (kernel arguments and
// loop counters only), so the constants arrive by scalar loads and cost no vector register or LDS.  A round unrolled over its t^2 + 3t
// products would be large (an ESTIMATE from ~1.5 KB of code per product: 60 KB at t = 5, several hundred at t = 12), so the loops over the output rows and over the S-boxes of a full
// round stay ROLLED and the register arrays ROTATE instead (a fixed register position is consumed / produced per iteration, then the array
// shifts by one element): 9 moves per element next to a row of t products.  A row sum is unrolled; a sparse partial round is unrolled
// up to t = 5 and walks its column products in a rolled, rotating loop above that.
// The state arrays are only ever touched by WHOLE-ELEMENT copies at constant indices (a product works on copies of its operands): the
// compiler turns an array into registers only while it sees few enough distinct accesses to it, and with limb-wise accesses the arrays of
// t = 9 and 12 stayed in scratch memory.  THE WIDTHS 9 AND 12 STILL USE SCRATCH (0.2 to 1.6 KB per lane, the resource table is
// profiles/fr_poseidon_kernel_stats.md) and run at a third of the rate of the narrow widths per product (DESIGN.md has the figures):
// splitting a state over a lane group (pairlane.hip.h / quad.hip.h style) is the open work, not done here.
//
// A row sum is frl_dot: the products of up to six elements accumulate in the columns of ONE Montgomery reduction (81 multiply-adds per
// product + 81 per sum instead of 162 per product), which is also one serial carry chain, so the scheduler cannot spread a row over the
// register file.  Independent products (the column products of a sparse round, the two dots of a long row) are kept apart with
// FRP_FENCE (a scheduling barrier): interleaved, they keep all their operands live at once, and the compiler's resource report showed
// the widths from 4 on filling the register file (256 VGPRs + AGPRs at one wavefront per SIMD, scratch at t = 5) without the fences
// against 3 wavefronts and no scratch with them.  That interleaving would not have paid in issue rate is an ASSUMPTION (dependent
// integer multiply-adds taken to issue back to back); the two schedules were not timed against each other.
//
// Bounds ("A": limbs < A 2^29, "V": value < V r; the table in fr.hip.h has the rules of frl_dot / frl_carry / frl_reduce):
//   state at the head of a round                A1 V2   (a dot, or a reduced sum of two; canonical A1 V1 on the first round)
//   + round constant (canonical)                A2 V3
//   S-box  x2 = x x: A 2 x 2, V 3 x 3;  x4 = x2 x2;  x5 = x4 x: A 1 x 2, V 2 x 3        -> A1 V2
//   row sum over N <= 6 elements: one dot, sum A <= 6, sum V <= 12 (full / dense rounds) -> A1 V2;  N > 6: two dots of at most six,
//   added (A2 V4) and reduced -> A1 V2
//   sparse partial round: y_j' = y_j + col_j z0 is A2 -> frl_carry -> A1, and V grows by 2 per round; every fourth round the y_j are
//   reduced (V2 again), so an operand y_j has V <= 8 and a dot of six sum V <= 48
#pragma once
#include "fr.hip.h"
#include "fr_poseidon_plan.h"

#ifndef FRP_WAVES
#define FRP_WAVES 2                               // wavefronts per SIMD the kernels are compiled for (profiles/fr_poseidon_kernel_stats.md)
#endif

#define FRP_FENCE() __builtin_amdgcn_sched_barrier(0)

namespace bls {

// entry `idx` of the image; idx is wave-uniform at every call site
DEV FrL frp_c(const u32* __restrict__ img, u32 idx) {
  FrL r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = img[(size_t)idx * FRP_ENTRY + k];
  return r;
}
DEV FrL frp_zero_l() { FrL r; for (int k = 0; k < 9; k++) r.l[k] = 0; return r; }
// x^5 2^-20: x A2 V3 -> A1 V2
DEV FrL frp_sbox(const FrL& x) {
  FRP_FENCE();
  const FrL x2 = frl_mul(x, x);
  const FrL x4 = frl_mul(x2, x2);
  const FrL x5 = frl_mul(x4, x);
  FRP_FENCE();
  return x5;
}
// sum_(j < G) s[j] * (entries e .. e + G - 1), G <= 6
template <int G> DEV FrL frp_dot(const FrL* s, const u32* __restrict__ img, u32 e) {
  static_assert(G >= 1 && G <= 6, "a dot takes at most six A1 operands");
  FrL a[G], b[G];                                                   // whole-element copies: see the note on register arrays above
#pragma unroll
  for (int g = 0; g < G; g++) { a[g] = s[g]; b[g] = frp_c(img, e + (u32)g); }
  const FrL r = frl_dot<G>(a, b);
  FRP_FENCE();
  return r;
}
// sum_(j < N) s[j] * (entries e .. e + N - 1): s[j] A1 with sum V <= 70 per half, the result A1 V2
template <int N> DEV FrL frp_row(const FrL* s, const u32* __restrict__ img, u32 e) {
  static_assert(N >= 1 && N <= 12, "two dots of at most six");
  if constexpr (N <= 6) {
    return frp_dot<N>(s, img, e);
  } else {
    constexpr int H = (N + 1) / 2;
    const FrL lo = frp_dot<H>(s, img, e);
    return frl_reduce(frl_add(lo, frp_dot<N - H>(s + H, img, e + H)));
  }
}
// s[0 .. N) <- s[1 .. N), s[0]: registers only, every index a constant
template <int N> DEV void frp_rotl(FrL* s) {
  const FrL t = s[0];
#pragma unroll
  for (int i = 0; i + 1 < N; i++) s[i] = s[i + 1];
  s[N - 1] = t;
}
// s <- Mat s for the N x N matrix at entry m (row-major): s[j] A1 V2, the result A1 V2
template <int N> DEV void frp_matvec(FrL* s, const u32* __restrict__ img, u32 m) {
  FrL o[N];
#pragma unroll
  for (int i = 0; i < N; i++) o[i] = frp_zero_l();
#pragma unroll 1
  for (int i = 0; i < N; i++) {
    const FrL row = frp_row<N>(s, img, m + (u32)(i * N));
    frp_rotl<N>(o);
    o[N - 1] = row;                                                 // row i; N - 1 - i shifts later it sits at o[i]
  }
#pragma unroll
  for (int i = 0; i < N; i++) s[i] = o[i];
}
// one full round: constants at entry c, the matrix at a.mfull
template <int T> DEV void frp_full_round(FrL* s, const u32* __restrict__ img, const FrpArgs& a, u32 c) {
#pragma unroll 1
  for (int i = 0; i < T; i++) {
    const FrL s0 = s[0];
    const FrL x = frp_sbox(frl_add(s0, frp_c(img, c + (u32)i)));
    frp_rotl<T>(s);
    s[T - 1] = x;                                                   // after T iterations every element is back in its place
  }
  frp_matvec<T>(s, img, a.mfull);
}

// the permutation on a state in registers: s[i] A1 V2 in, A1 V2 out
template <int T, bool SPARSE> DEV void frp_permute(FrL* s, const u32* __restrict__ img, const FrpArgs& a) {
#pragma unroll 1
  for (u32 r = 0; r < a.rf_half; r++) frp_full_round<T>(s, img, a, a.rc1 + r * T);
  if (SPARSE) {
#pragma unroll 1
    for (u32 r = 0; r < a.rp; r++) {
      const u32 e = a.part + r * (2 * T);                           // [k_r, row_0 .. row_(t-1), col_1 .. col_(t-1)]
      const FrL s0 = s[0];
      const FrL z0 = frp_sbox(frl_add(s0, frp_c(img, e)));
      s[0] = z0;
      const FrL y0 = frp_row<T>(s, img, e + 1);
      if constexpr (T > 6) {                                          // rolled like the rows of a full round: less than half the scratch of the unrolled form
#pragma unroll 1
        for (int j = 1; j < T; j++) {
          const FrL yj = s[1];
          const FrL nj = frl_carry(frl_add(yj, frl_mul(z0, frp_c(img, e + T + (u32)j))));
          frp_rotl<T - 1>(s + 1);
          s[T - 1] = nj;
        }
      } else {
#pragma unroll
        for (int j = 1; j < T; j++) {
          const FrL yj = s[j];
          s[j] = frl_carry(frl_add(yj, frl_mul(z0, frp_c(img, e + T + (u32)j))));
          FRP_FENCE();
        }
      }
      s[0] = y0;
      if ((r & 3) == 3) {
#pragma unroll
        for (int j = 1; j < T; j++) { const FrL yj = s[j]; s[j] = frl_reduce(yj); }
      }
    }
#pragma unroll
    for (int j = 1; j < T; j++) { const FrL yj = s[j]; s[j] = frl_reduce(yj); }
    frp_matvec<T - 1>(s + 1, img, a.pend);
  } else {
#pragma unroll 1
    for (u32 r = 0; r < a.rp; r++) {
      const FrL s0 = s[0];
      s[0] = frp_sbox(frl_add(s0, frp_c(img, a.part + r)));
      frp_matvec<T>(s, img, a.mpart);
    }
  }
#pragma unroll 1
  for (u32 r = 0; r < a.rf_half; r++) frp_full_round<T>(s, img, a, a.rc2 + r * T);
}

// ---- PERMUTE: n states of T scalars laid end to end; out == in is the in-place form (a lane reads its state before it writes it) -------------
template <int T, bool SPARSE>
__global__ void __launch_bounds__(FRP_BLOCK, FRP_WAVES) k_frp_permute(FrpArgs a, const u32* __restrict__ img, const u32* in, u32* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  FrL s[T];
#pragma unroll
  for (int j = 0; j < T; j++) s[j] = frl_load(in + (i * T + j) * 8);
  frp_permute<T, SPARSE>(s, img, a);
#pragma unroll
  for (int j = 0; j < T; j++) fr_store(out + (i * T + j) * 8, frl_canon(s[j]));
}

// ---- HASH / LEVEL: n preimages of T - 1 scalars; the state is (tag, x_1 .. x_(T-1)), the digest element 1 after the permutation.  A Merkle
// level is this kernel over the level below; out2 (may be NULL) receives the same digests (the roots, next to the nodes array) ------------------
template <int T, bool SPARSE>
__global__ void __launch_bounds__(FRP_BLOCK, FRP_WAVES) k_frp_hash(FrpArgs a, const u32* __restrict__ img, FrArg tag, const u32* __restrict__ in, u32* __restrict__ out, u32* __restrict__ out2,
                                                         size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  FrL s[T];
  Fr tg;
#pragma unroll
  for (int w = 0; w < 8; w++) tg.l[w] = tag.w[w];
  s[0] = frl_unpack(tg);
#pragma unroll
  for (int j = 1; j < T; j++) s[j] = frl_load(in + (i * (T - 1) + (j - 1)) * 8);
  frp_permute<T, SPARSE>(s, img, a);
  const Fr d = frl_canon(s[1]);
  fr_store(out + i * 8, d);
  if (out2) fr_store(out2 + i * 8, d);
}

}  // namespace bls
