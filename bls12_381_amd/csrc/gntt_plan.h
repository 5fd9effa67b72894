// gntt_plan.h -- the launch plan of the group transforms (blsgpu_g1_ntt_many* / blsgpu_g2_ntt_many*) as plain host code: which kernels of
// gntt.hip.h run, in which order, with which grid / block / dynamic LDS and stage index, for k vectors of 2^log_n points laid end to
// end.  No HIP calls here: api_msm.hip walks the plan and launches, tests/simt/emu_gntt.cpp walks the same plan on the host.
//
// Radix-2 decimation in time, in place:
//   GN_K_PERMUTE   one pass: the bit-reversal permutation inside every vector (a lane per point; it also rewrites every record with
//                  Z = 0 as (0 : 1 : 0), the identity the complete formulas expect)
//   GN_K_FIRST     stage 0: every twiddle is 1, a butterfly is (a + b, a - b); the inverse transform multiplies both by n^-1 here
//                  (two products per butterfly, n per vector) instead of scaling the result in a pass of its own
//   GN_K_STAGE     stages 1 .. log_n - 1, one per launch: t = [w^e] b, a' = a + t, b' = a - t.  Butterfly i of stage s has the offset
//                  j = i mod 2^s inside its block of 2^(s+1) points, so the concatenation of k vectors is k times as many blocks (as in
//                  fr_plan.h) and the twiddle is entry j of level s of the Fr twiddle table.
// Every stage has B = k 2^(log_n - 1) butterflies, and the product is the whole cost of one (about 1 860 field multiplications for G1
// against 24 for the two additions), so a stage is B dependent chains.  Two shapes:
//   GN_LANE   a butterfly per lane (G1) or lane pair (G2, pairlane.hip.h), 256 lanes per workgroup: the throughput shape
//   GN_TEAM   a butterfly per team of eight lanes (team.hip.h): two multiplication latencies per point operation instead of eight
//             to twelve, for calls whose B leaves most of the chip idle in the lane shape
// One shape per call, chosen from B (G2: 2 B) against GNTT_TEAM_MAX_B.
#pragma once
#include <stddef.h>

namespace bls {

enum GnKernel { GN_K_PERMUTE = 0, GN_K_FIRST = 1, GN_K_STAGE = 2 };
enum GnShape { GN_LANE = 0, GN_TEAM = 1 };
constexpr int GNTT_MAX_LOG = 24;                  // log_n <= 24 and k 2^log_n <= 2^24
constexpr unsigned GNTT_LANE_BLOCK = 256;         // as k_mul_batch_glv / k_mul_batch_gls
constexpr unsigned GNTT_TEAM_BLOCK = 64;          // one wavefront = eight teams: the mailbox barriers stay inside a wavefront
constexpr int GNTT_TEAM_LANES = 8;                // = TEAM (team.hip.h; gntt.hip.h static_asserts it)
// The crossover between the shapes, in lanes of the LANE shape: a call takes the team shape while B (G1) or 2 B (G2: a lane pair per
// butterfly) does not exceed it.  BLSGPU_GNTT_TEAM_MAX=<value> overrides it (0: always the lane shape, a huge value: always the team
// shape).  Measured on MI355X by tools/g_ntt_time.py, which runs every size in both shapes (profiles/g_ntt_time.json, `sweep`, k x 2^10
// points), team / lane: G1 9.1 / 23.7 ms at B = 8 192, 17.9 / 24.0 ms at 16 384, 35.2 / 24.5 ms at 32 768; G2 22.5 / 25.5 ms at B = 8 192,
// 44.0 / 26.3 ms at 16 384.  The team shape's time doubles with B from B = 8 192 on (the chip is full of teams), the lane shape's stays
// flat until the chip is full of lanes, and they cross between 16 384 and 32 768 lane-shape lanes in both groups.
constexpr size_t GNTT_TEAM_MAX_B = 16384;
// the value of BLSGPU_GNTT_TEAM_MAX (NULL or not a number: the built-in constant); diag.h and the host emulation both read it here
inline size_t gntt_team_max_from(const char* v) {
  if (!v || *v < '0' || *v > '9') return GNTT_TEAM_MAX_B;
  size_t b = 0;
  for (; *v >= '0' && *v <= '9'; v++) b = b > ((size_t)1 << 40) ? b : b * 10 + (size_t)(*v - '0');
  return b;
}

struct GnStep {
  int kernel;                  // GnKernel
  int shape;                   // GnShape (GN_K_PERMUTE: GN_LANE, a lane per point in both groups)
  unsigned grid, block;
  size_t lds;                  // bytes of dynamic LDS (the team mailboxes)
  int stage;                   // GN_K_FIRST: 0; GN_K_STAGE: s, half-span 2^s
};
struct GnPlan {
  int n_steps = 0;
  GnStep step[GNTT_MAX_LOG + 1];
  size_t total = 0;            // k * 2^log_n points
  size_t butterflies = 0;      // B = total / 2
  int shape = GN_LANE;
};

// group: 1 = G1, 2 = G2.  log_n in [0, GNTT_MAX_LOG], k * 2^log_n <= 2^GNTT_MAX_LOG.
inline GnPlan gntt_plan_many(int group, int log_n, size_t k, size_t team_max_b = GNTT_TEAM_MAX_B) {
  GnPlan p;
  p.total = k << log_n;
  if (log_n == 0 || k == 0) return p;             // no step: a vector of one point is its own transform (and n^-1 = 1)
  const size_t B = p.total >> 1;
  p.butterflies = B;
  const unsigned lanes_per_bf = group == 2 ? 2 : 1;                  // lane shape: a lane pair per G2 butterfly
  p.shape = B * lanes_per_bf <= team_max_b ? GN_TEAM : GN_LANE;
  const size_t mbox_words = (size_t)6 * (group == 2 ? 28 : 14);      // TEAM_SLOTS * TeamTraits<F>::WORDS (gntt.hip.h static_asserts it)
  unsigned grid, block; size_t lds;
  if (p.shape == GN_TEAM) {
    block = GNTT_TEAM_BLOCK; lds = (size_t)(block / GNTT_TEAM_LANES) * mbox_words * 4;
    grid = (unsigned)((B * GNTT_TEAM_LANES + block - 1) / block);
  } else {
    block = GNTT_LANE_BLOCK; lds = 0;
    grid = (unsigned)((B * lanes_per_bf + block - 1) / block);
  }
  p.step[p.n_steps++] = GnStep{GN_K_PERMUTE, GN_LANE, (unsigned)((p.total + 255) / 256), 256, 0, 0};
  p.step[p.n_steps++] = GnStep{GN_K_FIRST, p.shape, grid, block, lds, 0};
  for (int s = 1; s < log_n; s++) p.step[p.n_steps++] = GnStep{GN_K_STAGE, p.shape, grid, block, lds, s};
  return p;
}

}  // namespace bls
