// gsum_plan.h -- the segmented, gathered point sums (blsgpu_g{1,2}_sum_segments[_device]) as plain host code: the limits, the cut of
// the term list into chunks and lane slices, which record of the scratch a partial sum goes to, the jobs of the combine pass, the
// launch shapes, the scratch bytes and every argument check.  No HIP calls here: api_msm.hip launches from the plan, gsum.hip.h reads
// the cut through the GSUM_HD functions below, tests/simt/emu_gsum.cpp walks the same plan on the host and
// tests/cpp/gsum_plan_main.cpp sweeps it under sanitizers.
//
// The cut.  The `total` terms of a call form ONE list, whatever the segments are.  Chunk c is the terms [c * chunk, (c + 1) * chunk) of
// that list, chunk = block * terms: one workgroup of `block` lanes, lane l taking the `terms` consecutive terms from c * chunk +
// l * terms.  A segment is the terms [off(s), off(s + 1)), off(s) = min(offsets[s], total) with off(0) = 0 and off(nseg) = total, so a
// lane's slice holds the end of at most one segment that began before it (its HEAD), any number of whole segments, and the beginning
// of at most one segment that goes on behind it.
//
//   pass 1 (k_gsum_chunks, one workgroup per chunk)  a lane adds its slice serially, closing a segment where it ends: a whole segment
//           goes straight to the output, a head is added to the lane before it; what a lane holds at the end of its slice meets the
//           equal-keyed values of the lanes behind it in a tree in LDS.  A segment that lies inside ONE chunk is final there.  Of a
//           segment that crosses a chunk's border the chunk keeps a partial: record 2 c (HEAD: the segment holds the chunk's first term)
//           or 2 c + 1 (TAIL) of the scratch, and the segments of its first and last term in meta[2 c], meta[2 c + 1].
//   pass 2 (k_gsum_combine)  job 2 c + w (w = 0 HEAD, 1 TAIL) belongs to the segment that record names IF the segment begins in chunk c
//           and ends in a later one: it adds that record and the HEAD records of the chunks up to the segment's last.  Every
//           multi-chunk segment begins in exactly one chunk, as its first or as its last segment: one job, each partial read once.
//           The same launch writes the identity for every empty segment (lane i of the grid looks at segment i).
// No workgroup waits for another, nothing is counted with atomics; the passes are ordered by the stream.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define GSUM_HD __host__ __device__ inline
#else
#define GSUM_HD inline
#endif

// lanes per workgroup (G1 / G2: the tree's LDS is block * 176 / 336 bytes) and terms per lane; -D overrides them for a build
#ifndef GSUM_BLOCK_G1
#define GSUM_BLOCK_G1 256
#endif
#ifndef GSUM_BLOCK_G2
#define GSUM_BLOCK_G2 128
#endif
#ifndef GSUM_TERMS
#define GSUM_TERMS 8
#endif

namespace bls {

constexpr size_t GSUM_MAX_TOTAL = (size_t)1 << 28;           // terms of one call
constexpr size_t GSUM_MAX_SEGS = (size_t)1 << 28;            // segments of one call
constexpr uint64_t GSUM_MAX_POINTS = (uint64_t)1 << 32;      // npoints must be below it: an index is 32 bits
constexpr uint32_t GSUM_NONE = 0xffffffffu;                  // the key of a lane without terms
constexpr uint32_t GSUM_STATUS_BAD = 16u;                    // d_status bit: an index was >= npoints (device form; the term was skipped)
constexpr size_t GSUM_LDS_LIMIT = 64 * 1024;                 // what a kernel gets unasked
constexpr int GSUM_REC_WORDS_G1 = 44, GSUM_REC_WORDS_G2 = 84;      // msm.hip.h Store<F>::PROJ_WORDS
constexpr int GSUM_OUT_WORDS_G1 = 36, GSUM_OUT_WORDS_G2 = 72;      // a projective point on the wire, u32 words

struct GsumShape { int block, terms; };
inline GsumShape gsum_shape(int group) { return GsumShape{group == 1 ? GSUM_BLOCK_G1 : GSUM_BLOCK_G2, GSUM_TERMS}; }

// ---- the cut, as the kernels read it ---------------------------------------------------------------------------------------------
// off(s), s in [0, nseg]: clamped to total; the two ends are what they must be whatever the array holds.  Offsets that DECREASE (the device
// form cannot refuse them) stay as they are: every index the kernels form from them lies inside out, part and meta, but a segment may
// then be written by two workgroups -- its value is unspecified, as the public header says.
GSUM_HD uint32_t gsum_off(const unsigned long long* offsets, uint32_t nseg, uint32_t total, uint32_t s) {
  if (s == 0) return 0;
  if (s >= nseg) return total;
  const unsigned long long o = offsets[s];
  return o < total ? (uint32_t)o : total;
}
// the segment of term t < total: the LAST s < nseg with off(s) <= t (the empty segments that begin at t's segment's start come before it)
GSUM_HD uint32_t gsum_seg_of(const unsigned long long* offsets, uint32_t nseg, uint32_t total, uint32_t t) {
  uint32_t lo = 0, hi = nseg;                                // off(lo) <= t, off(hi) > t
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (gsum_off(offsets, nseg, total, mid) <= t) lo = mid; else hi = mid;
  }
  return lo;
}
// a segment [so, se) that the chunk beginning at cb holds whole: final in pass 1.  (se <= total always: the chunk's end needs no clamp.)
GSUM_HD bool gsum_inside(uint32_t so, uint32_t se, uint32_t cb, uint32_t chunk) { return so >= cb && se - cb <= chunk; }
// where chunk c keeps its partial of a segment [so, ..) it does not hold whole: record 2 c (HEAD) or 2 c + 1 (TAIL)
GSUM_HD size_t gsum_record(size_t c, uint32_t so, uint32_t cb) { return 2 * c + (so <= cb ? 0 : 1); }
// job 2 c + w of pass 2, first / last = meta[2 c], meta[2 c + 1]: the segment it sums and the last chunk of it, or false (no work)
GSUM_HD bool gsum_job(const unsigned long long* offsets, uint32_t nseg, uint32_t total, uint32_t chunk, size_t c, int w, uint32_t first, uint32_t last,
                      uint32_t* seg, size_t* c_last) {
  if (w && last == first) return false;                      // one segment covers the chunk: job 2 c, or an earlier chunk's
  const uint32_t s = w ? last : first;
  if (s >= nseg) return false;
  const uint32_t so = gsum_off(offsets, nseg, total, s), se = gsum_off(offsets, nseg, total, s + 1);
  if (se <= so) return false;
  if (so / chunk != c) return false;                         // it begins in an earlier chunk: that chunk's job
  if ((se - 1) / chunk == c) return false;                   // whole inside this chunk: final since pass 1
  *seg = s; *c_last = (se - 1) / chunk;
  return true;
}

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal -------------------------------------------------
struct GsumArgs {
  int group = 1;
  const void* xy = nullptr; const void* inf = nullptr; uint64_t npoints = 0;
  const void* idx = nullptr; const void* offsets = nullptr; uint64_t nseg = 0, total = 0;
  const void* out = nullptr;
  bool device = false;
};
inline const char* gsum_check(const GsumArgs& a) {
  if (a.group != 1 && a.group != 2) return "sum_segments: group must be 1 or 2";
  if (a.total > GSUM_MAX_TOTAL) return "sum_segments: total must not exceed 2^28";
  if (a.nseg > GSUM_MAX_SEGS) return "sum_segments: nseg must not exceed 2^28";
  if (a.npoints >= GSUM_MAX_POINTS) return "sum_segments: npoints must be below 2^32";
  if (a.nseg && (!a.offsets || !a.out)) return "sum_segments: NULL offsets or output with segments to sum";
  if (a.nseg && a.total && (!a.xy || !a.inf)) return "sum_segments: NULL points with terms to add";
  if (!a.nseg && a.total) return "sum_segments: terms but no segment";
  if (!a.idx && a.total > a.npoints) return "sum_segments: without idx, term t is point t: total must not exceed npoints";
  if (a.device) {
    if (((uintptr_t)a.xy & 7) || ((uintptr_t)a.offsets & 7) || ((uintptr_t)a.out & 7)) return "sum_segments: d_xy, d_offsets and d_out_xyz must be 8-byte aligned";
    if ((uintptr_t)a.idx & 3) return "sum_segments: d_idx must be 4-byte aligned";
  }
  return nullptr;
}
// what only the host forms can see: the offsets as the interface states them, every index of a term inside the point set
inline const char* gsum_check_host(const uint64_t* offsets, uint64_t nseg, uint64_t total, const uint32_t* idx, uint64_t npoints) {
  if (!nseg) return nullptr;
  if (offsets[0] != 0) return "sum_segments: offsets[0] must be 0";
  for (uint64_t s = 0; s < nseg; s++) if (offsets[s] > offsets[s + 1]) return "sum_segments: offsets must be non-decreasing";
  if (offsets[nseg] != total) return "sum_segments: total must be offsets[nseg]";
  if (idx) for (uint64_t t = 0; t < total; t++) if (idx[t] >= npoints) return "sum_segments: an index is outside the point set";
  return nullptr;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
struct GsumPlan {
  int ok = 0;                          // 0: refused (sizes or the shape out of range)
  unsigned block = 0, terms = 0;
  uint32_t chunk = 0;                  // block * terms
  size_t nchunks = 0;
  unsigned chunks_grid = 0;            // k_gsum_chunks: a workgroup per chunk (0: no launch)
  unsigned combine_grid = 0;           // k_gsum_combine: max(2 nchunks jobs, a lane per segment)
  size_t lds = 0;                      // dynamic LDS of either kernel: block records, block keys, block head flags
  size_t records = 0;                  // 2 nchunks partial records of rec_words u32
  size_t meta_words = 0;               // 2 nchunks u32
  size_t part_bytes = 0, meta_bytes = 0;
};
constexpr size_t gsum_lds_bytes(int group, int block) { return (size_t)block * ((group == 1 ? GSUM_REC_WORDS_G1 : GSUM_REC_WORDS_G2) + 2) * 4; }
inline GsumPlan gsum_plan(int group, size_t nseg, size_t total, GsumShape shape) {
  GsumPlan p;
  if ((group != 1 && group != 2) || nseg > GSUM_MAX_SEGS || total > GSUM_MAX_TOTAL) return p;
  if (shape.block < 1 || shape.block > 1024 || (shape.block & (shape.block - 1)) || shape.terms < 1 || shape.terms > 4096) return p;
  if (gsum_lds_bytes(group, shape.block) > GSUM_LDS_LIMIT) return p;
  p.block = (unsigned)shape.block; p.terms = (unsigned)shape.terms;
  p.chunk = p.block * p.terms;                                // <= 2^22
  p.nchunks = nseg ? (total + p.chunk - 1) / p.chunk : 0;
  p.chunks_grid = (unsigned)p.nchunks;
  const size_t seg_groups = (nseg + p.block - 1) / p.block;
  p.combine_grid = (unsigned)(2 * p.nchunks > seg_groups ? 2 * p.nchunks : seg_groups);
  p.lds = gsum_lds_bytes(group, shape.block);
  p.records = 2 * p.nchunks; p.meta_words = 2 * p.nchunks;
  p.part_bytes = p.records * (group == 1 ? GSUM_REC_WORDS_G1 : GSUM_REC_WORDS_G2) * 4;
  p.meta_bytes = p.meta_words * 4;
  p.ok = 1;
  return p;
}
inline GsumPlan gsum_plan(int group, size_t nseg, size_t total) { return gsum_plan(group, nseg, total, gsum_shape(group)); }
static_assert((GSUM_BLOCK_G1 & (GSUM_BLOCK_G1 - 1)) == 0 && (GSUM_BLOCK_G2 & (GSUM_BLOCK_G2 - 1)) == 0, "the trees halve the block");

}  // namespace bls
