// fr_lagrange_plan.h -- Lagrange coefficients at arbitrary nodes (blsgpu_fr_lagrange_segments[_device], and the coefficient stage of
// blsgpu_g{1,2}_lagrange_combine) as plain host code: the limits, the two launch shapes and the choice between them, which lanes own
// which nodes, the tiles the nodes pass through LDS in, the LDS and scratch bytes, the status bit and every argument check.  No HIP
// calls here: api_fr.hip launches from the plan, fr_lagrange.hip.h reads the cut through the FLG_HD functions below,
// tests/simt/emu_fr_lagrange.cpp walks the same plan on the host and tests/cpp/fr_lagrange_plan_main.cpp sweeps it under sanitizers.
//
// The cut.  A TEAM of `team` lanes owns one segment from its first node to its results; segment s belongs to team s % teams of
// workgroup s / teams (teams = block / team), so the launch is a function of nseg alone and a team never waits for another one.
//   BLOCK shape  team = block = 256: one workgroup per segment, the team meets at the workgroup barrier.
//   WAVE shape   team = 8 .. 64 lanes (the smallest power of two that holds the average segment), all inside ONE wavefront: several
//                segments per wavefront, four wavefronts per workgroup, no workgroup barrier anywhere (the teams of a workgroup run
//                segments of different lengths); a team's lanes meet in the wavefront's own program order.
// Either shape is right for every length up to FLG_LEN_MAX: lane l of the team owns the nodes i = k * team + l (flg_node), R of them
// at a time in registers (a PASS covers team * R nodes, flg_passes), and every pass walks ALL nodes of the segment through the team's
// LDS tile, `tile` nodes at a time (flg_tiles): one broadcast read of x_j feeds the R denominators D_i of every lane.
// What a team keeps between its two sweeps lies in global memory, 32 bytes per node each: the factors e_i (in `lambda` itself when the
// caller wants the coefficients, else in scratch) and the running products of Montgomery's trick (always scratch).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FLG_HD __host__ __device__ inline
#else
#define FLG_HD inline
#endif

// lanes per workgroup of both shapes, nodes per lane per pass, LDS tile of the BLOCK shape in nodes (WAVE: tile = team); -D overrides
#ifndef FLG_BLOCK
#define FLG_BLOCK 256
#endif
#ifndef FLG_R
#define FLG_R 4
#endif
#ifndef FLG_TILE
#define FLG_TILE 512
#endif
#ifndef FLG_WAVE
#define FLG_WAVE 64
#endif

namespace bls {

constexpr uint32_t FLG_LEN_MAX = 4096;                       // nodes of one segment (= SEG_LEN_MAX: the same offsets feed *_msm_segments)
constexpr size_t FLG_MAX_TOTAL = (size_t)1 << 27;            // nodes of one call
constexpr size_t FLG_MAX_SEGS = (size_t)1 << 27;             // segments of one call
constexpr uint32_t FLG_STATUS_BAD = 32u;                     // d_status bit: a segment's offsets decrease, exceed FLG_LEN_MAX or end beyond total (device form)
constexpr size_t FLG_LDS_LIMIT = 64 * 1024;                  // what a kernel gets unasked
constexpr int FLG_AUTO = 0, FLG_SHAPE_BLOCK = 1, FLG_SHAPE_WAVE = 2;
constexpr size_t FLG_WAVE_BELOW = 128;                       // total / nseg below it: the WAVE shape

// what a launch is made of; `wave` is the widest team that can meet without the workgroup barrier (64 on the device)
struct FlgShape { int block, team, tile, r, wave; };

// ---- the cut, as the kernels read it -----------------------------------------------------------------------------------------------
// the nodes [*so, *so + *t) of segment s, or false for a segment that breaks the contract (nothing of it is ever used as an address)
FLG_HD bool flg_segment(const uint32_t* offsets, uint32_t total, size_t s, uint32_t* so, uint32_t* t) {
  const uint32_t a = offsets[s], b = offsets[s + 1];
  if (b < a || b - a > FLG_LEN_MAX || b > total) return false;
  *so = a; *t = b - a;
  return true;
}
FLG_HD uint32_t flg_passes(uint32_t t, uint32_t team, uint32_t r) { return (t + team * r - 1) / (team * r); }
FLG_HD uint32_t flg_tiles(uint32_t t, uint32_t tile) { return (t + tile - 1) / tile; }
// node k of lane l (k counts the lane's own nodes across the passes); the lane owns flg_count of them
FLG_HD uint32_t flg_node(uint32_t k, uint32_t l, uint32_t team) { return k * team + l; }
FLG_HD uint32_t flg_count(uint32_t t, uint32_t l, uint32_t team) { return l < t ? (t - l + team - 1) / team : 0u; }
// LDS words of one team: the tile, the tree of 2 team elements, the tree of 2 team counters
constexpr FLG_HD uint32_t flg_team_lds_words(uint32_t team, uint32_t tile) { return tile * 8 + 2 * team * 8 + 2 * team; }

inline int flg_shape_from(const char* v) {                   // BLSGPU_LAGRANGE_SHAPE=block|wave (diag.h): anything else is automatic
  if (!v) return FLG_AUTO;
  if (!strcmp(v, "block")) return FLG_SHAPE_BLOCK;
  if (!strcmp(v, "wave")) return FLG_SHAPE_WAVE;
  return FLG_AUTO;
}

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal -------------------------------------------------
struct FlgArgs {
  const void* nodes = nullptr; const void* offsets = nullptr; uint64_t nseg = 0, total = 0;
  const void* points = nullptr; const void* values = nullptr;
  const void* lambda = nullptr; const void* y = nullptr; const void* flags = nullptr;
  bool device = false;
  bool lambda_in_scratch = false;      // the combines: the coefficients go to the context's scratch, neither lambda nor y is the caller's
};
inline bool flg_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}
inline const char* flg_check(const FlgArgs& a) {
  if (a.nseg > FLG_MAX_SEGS) return "fr_lagrange_segments: nseg must not exceed 2^27";
  if (a.total > FLG_MAX_TOTAL) return "fr_lagrange_segments: total must not exceed 2^27";
  if (!a.nseg) return a.total ? "fr_lagrange_segments: nodes but no segment" : nullptr;
  if (!a.offsets) return "fr_lagrange_segments: NULL offsets with segments to do";
  if (a.total && !a.nodes) return "fr_lagrange_segments: NULL nodes with nodes to read";
  if (a.y && !a.values && a.total) return "fr_lagrange_segments: y needs values";
  if (!a.lambda && !a.y && !a.lambda_in_scratch) return "fr_lagrange_segments: at least one of lambda and y must be given";
  if (a.device) {
    if (((uintptr_t)a.nodes | (uintptr_t)a.points | (uintptr_t)a.values | (uintptr_t)a.lambda | (uintptr_t)a.y) & 15)
      return "fr_lagrange_segments_device: scalar arrays must be 16-byte aligned";
    if ((uintptr_t)a.offsets & 3) return "fr_lagrange_segments_device: d_offsets must be 4-byte aligned";
  }
  const struct { const void* p; uint64_t bytes; } in[4] = {{a.nodes, a.total * 32}, {a.offsets, (a.nseg + 1) * 4}, {a.points, a.nseg * 32}, {a.values, a.total * 32}},
                                                  out[3] = {{a.lambda, a.total * 32}, {a.y, a.nseg * 32}, {a.flags, a.nseg}};
  for (int o = 0; o < 3; o++) {
    for (int i = 0; i < 4; i++) if (flg_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return "fr_lagrange_segments: an output overlaps an input (there is no in-place form)";
    for (int q = o + 1; q < 3; q++) if (flg_overlap(out[o].p, out[o].bytes, out[q].p, out[q].bytes)) return "fr_lagrange_segments: two outputs overlap";
  }
  return nullptr;
}
// what only the host forms can see: the offsets as the interface states them
inline const char* flg_check_host(const uint32_t* offsets, uint64_t nseg, uint64_t total) {
  if (!nseg) return nullptr;
  if (offsets[0] != 0) return "fr_lagrange_segments: offsets[0] must be 0";
  for (uint64_t s = 0; s < nseg; s++) {
    if (offsets[s] > offsets[s + 1]) return "fr_lagrange_segments: offsets must be non-decreasing";
    if (offsets[s + 1] - offsets[s] > FLG_LEN_MAX) return "fr_lagrange_segments: a segment is longer than BLSGPU_FR_LAGRANGE_LEN_MAX";
  }
  if (offsets[nseg] != total) return "fr_lagrange_segments: total must be offsets[nseg]";
  return nullptr;
}

// blsgpu_g{1,2}_lagrange_combine: the checks above for the coefficient stage, then the points and the sums
struct FlgcArgs {
  int group = 1;
  const void* xy = nullptr; const void* inf = nullptr;
  const void* nodes = nullptr; const void* offsets = nullptr; uint64_t nseg = 0, total = 0;
  const void* points = nullptr; const void* out = nullptr; const void* flags = nullptr;
  bool device = false;
};
inline const char* flgc_check(const FlgcArgs& a) {
  if (a.group != 1 && a.group != 2) return "lagrange_combine: group must be 1 or 2";
  FlgArgs f;
  f.nodes = a.nodes; f.offsets = a.offsets; f.nseg = a.nseg; f.total = a.total; f.points = a.points; f.flags = a.flags; f.device = a.device; f.lambda_in_scratch = true;
  if (const char* why = flg_check(f)) return why;
  if (!a.nseg) return nullptr;
  if (!a.out) return "lagrange_combine: NULL output with segments to combine";
  if (a.total && (!a.xy || !a.inf)) return "lagrange_combine: NULL points with shares to combine";
  if (a.device && (((uintptr_t)a.xy | (uintptr_t)a.out) & 7)) return "lagrange_combine_device: d_xy and d_out_xyz must be 8-byte aligned";
  const uint64_t pb = a.group == 1 ? 48 : 96;                  // bytes of one coordinate
  const struct { const void* p; uint64_t bytes; } in[5] = {{a.xy, a.total * 2 * pb}, {a.inf, a.total}, {a.nodes, a.total * 32}, {a.offsets, (a.nseg + 1) * 4}, {a.points, a.nseg * 32}};
  for (int i = 0; i < 5; i++) {
    if (flg_overlap(a.out, a.nseg * 3 * pb, in[i].p, in[i].bytes)) return "lagrange_combine: the output overlaps an input (there is no in-place form)";
    if (flg_overlap(a.flags, a.nseg, in[i].p, in[i].bytes)) return "lagrange_combine: the flags overlap an input";
  }
  if (flg_overlap(a.out, a.nseg * 3 * pb, a.flags, a.nseg)) return "lagrange_combine: two outputs overlap";
  return nullptr;
}
// lanes of the workgroup that sums one segment's products: the smallest power of two that holds the average segment, 64 .. 256 (G2: 128)
inline unsigned flgc_block(int group, size_t nseg, size_t total) {
  const size_t avg = nseg ? total / nseg : 0;
  unsigned b = 64;
  while (b < (group == 1 ? 256u : 128u) && b < avg) b *= 2;
  return b;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
struct FlgPlan {
  int ok = 0;                          // 0: refused (sizes or the shape out of range)
  int shape = 0;                       // FLG_SHAPE_BLOCK / FLG_SHAPE_WAVE
  unsigned block = 0, team = 0, tile = 0, r = 0;
  unsigned teams = 0;                  // segments per workgroup = block / team
  unsigned grid = 0;                   // workgroups (0: no launch)
  size_t lds = 0;                      // dynamic LDS of the workgroup: teams * flg_team_lds_words * 4
  size_t pre_bytes = 0;                // scratch: the running products, 32 bytes per node
  size_t work_bytes = 0;               // scratch: the factors e_i when the caller takes no lambda (else they live in lambda)
};
inline bool flg_pow2(unsigned v) { return v && !(v & (v - 1)); }
inline bool flg_shape_ok(const FlgShape& s) {
  if (s.block < 1 || s.block > 1024 || !flg_pow2((unsigned)s.team) || s.team > s.block || s.block % s.team) return false;
  if (s.tile < 1 || s.tile > (int)FLG_LEN_MAX || s.r < 1 || s.r > 8 || !flg_pow2((unsigned)s.wave)) return false;
  if (s.team != s.block && s.team > s.wave) return false;      // several teams per workgroup: each inside one wavefront
  if (s.team != s.block && s.block % s.wave) return false;
  return (size_t)(s.block / s.team) * flg_team_lds_words((uint32_t)s.team, (uint32_t)s.tile) * 4 <= FLG_LDS_LIMIT;
}
// the shipped shapes: which = FLG_SHAPE_BLOCK / FLG_SHAPE_WAVE, or FLG_AUTO for the choice by the average length
inline FlgShape flg_shape(size_t nseg, size_t total, int which) {
  const size_t avg = nseg ? total / nseg : 0;
  if (which == FLG_AUTO) which = avg < FLG_WAVE_BELOW ? FLG_SHAPE_WAVE : FLG_SHAPE_BLOCK;
  if (which == FLG_SHAPE_BLOCK) return FlgShape{FLG_BLOCK, FLG_BLOCK, FLG_TILE, FLG_R, FLG_WAVE};
  int team = 8;
  while (team < FLG_WAVE && (size_t)team < avg) team *= 2;
  return FlgShape{FLG_BLOCK, team, team, FLG_R, FLG_WAVE};
}
inline FlgPlan flg_plan(size_t nseg, size_t total, bool want_lambda, FlgShape shape) {
  FlgPlan p;
  if (nseg > FLG_MAX_SEGS || total > FLG_MAX_TOTAL || !flg_shape_ok(shape)) return p;
  p.shape = shape.team == shape.block ? FLG_SHAPE_BLOCK : FLG_SHAPE_WAVE;
  p.block = (unsigned)shape.block; p.team = (unsigned)shape.team; p.tile = (unsigned)shape.tile; p.r = (unsigned)shape.r;
  p.teams = p.block / p.team;
  p.grid = (unsigned)((nseg + p.teams - 1) / p.teams);
  p.lds = (size_t)p.teams * flg_team_lds_words(p.team, p.tile) * 4;
  p.pre_bytes = nseg ? total * 32 : 0;
  p.work_bytes = nseg && !want_lambda ? total * 32 : 0;
  p.ok = 1;
  return p;
}
inline FlgPlan flg_plan(size_t nseg, size_t total, bool want_lambda, int which = FLG_AUTO) { return flg_plan(nseg, total, want_lambda, flg_shape(nseg, total, which)); }
static_assert((FLG_BLOCK & (FLG_BLOCK - 1)) == 0 && FLG_BLOCK % FLG_WAVE == 0, "the trees halve the team");

}  // namespace bls
