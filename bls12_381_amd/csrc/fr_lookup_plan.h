// fr_lookup_plan.h -- the Fr lookup tables (blsgpu_fr_lookup_*) as plain host code: the limits, the key hash, the size of the slot
// array, the launch shapes of the three kernels, which of the two counting paths a table takes, and every argument check.  No HIP calls
// here: api_fr.hip launches from the plan, tests/simt/emu_fr_lookup.cpp walks the same plan on the host,
// tests/cpp/fr_lookup_plan_main.cpp sweeps it under sanitizers.
//
// The index.  A key is a row of c scalars = 8 c 32-bit words.  The handle keeps the keys row-major and an open-addressed array of
// `slots` 32-bit words, slots = the power of two >= 2 * rows (load factor <= 1/2): a word holds row + 1 of the FIRST table row with the
// key that claimed the slot, or 0.  A key starts at frl_hash(key) & (slots - 1) and probes linearly.
//
// Counting.  Tables of at most FRL_LDS_ROWS rows count in per-workgroup LDS counters, one per table row (path 1); larger tables count
// in a per-workgroup direct-mapped LDS cache of FRL_CACHE entries {row + 1, count} in front of the global counters (path 2).  Either way
// a workgroup takes many looked-up rows (a grid-stride loop of `iters` batches) and flushes what it gathered once, at its end.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define FRL_HD __host__ __device__ inline
#else
#define FRL_HD inline
#endif

namespace bls {

constexpr int FRL_MAX_COLS = 8;                               // BLSGPU_FR_FRAC_MAX_COLS
constexpr size_t FRL_MAX_ROWS = (size_t)1 << 24;
constexpr size_t FRL_MAX_TOTAL = (size_t)1 << 28;             // n, and the footprint (c - 1) * pitch + n of a column set
constexpr int FRL_BLOCK = 256;
constexpr size_t FRL_LDS_ROWS = 4096;                         // BLSGPU_FR_LOOKUP_LDS_ROWS: the largest table of path 1 (16 KB of counters)
constexpr unsigned FRL_CACHE = 2048;                          // entries of path 2's cache: 8 KB of tags + 8 KB of counts
constexpr unsigned FRL_CACHE_LOG = 11;
constexpr unsigned FRL_COUNT_GRID_MAX = 1024;                 // workgroups of the count kernel: four per CU, each flushing once
constexpr size_t FRL_LDS_LIMIT = 64 * 1024;                   // what a kernel gets unasked; two workgroups share a CU well below it
constexpr uint32_t FRL_MISS = 0xffffffffu;                    // d_index of a looked-up row that is in no table row
static_assert(FRL_CACHE == 1u << FRL_CACHE_LOG, "the cache is indexed by the top FRL_CACHE_LOG bits of a product");

// ---- the hash --------------------------------------------------------------------------------------------------------------------
// MurmurHash3's 32-bit rounds over the 8 c words of a key, then its finaliser.  Every round is a bijection of the state for a fixed
// word and of the word's contribution for a fixed state, so two keys that differ in exactly ONE word never collide in the 32-bit
// value; every word reaches every output bit through the finaliser.  Correctness of the table never depends on it: -DFRL_HASH_BITS=b
// (test builds) keeps only the low b bits and sets every other bit, so every chain starts in the last 2^b slots and wraps.
constexpr uint32_t FRL_HASH_SEED = 0x9747b28cu;
FRL_HD uint32_t frl_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
FRL_HD uint32_t frl_hash_step(uint32_t h, uint32_t w) {
  w *= 0xcc9e2d51u; w = frl_rotl(w, 15); w *= 0x1b873593u;
  h ^= w; h = frl_rotl(h, 13);
  return h * 5u + 0xe6546b64u;
}
FRL_HD uint32_t frl_hash_finish(uint32_t h, uint32_t words) {
  h ^= words * 4u;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
#if defined(FRL_HASH_BITS)
  h |= ~((1u << FRL_HASH_BITS) - 1u);
#endif
  return h;
}
// key: 8 * c words, contiguous
FRL_HD uint32_t frl_hash(const uint32_t* key, int c) {
  uint32_t h = FRL_HASH_SEED;
  for (int i = 0; i < 8 * c; i++) h = frl_hash_step(h, key[i]);
  return frl_hash_finish(h, (uint32_t)(8 * c));
}
// the cache entry of a table row (path 2): the top bits of a Fibonacci product, so rows a power of two apart do not share one
FRL_HD uint32_t frl_cache_entry(uint32_t row) { return (row * 0x9e3779b1u) >> (32 - FRL_CACHE_LOG); }

// ---- sizes -----------------------------------------------------------------------------------------------------------------------
// the power of two >= 2 * rows (rows in [1, 2^24]: at most 2^25)
inline size_t frl_slots(size_t rows) {
  size_t s = 2;
  while (s < 2 * rows) s <<= 1;
  return s;
}
// the footprint (c - 1) * pitch + n scalars of a column set; false when it does not fit 2^28 (64-bit overflow included)
inline bool frl_footprint(int c, size_t pitch, size_t n, size_t* scalars) {
  *scalars = 0;
  if (pitch > FRL_MAX_TOTAL || n > FRL_MAX_TOTAL) return false;
  const size_t f = (size_t)(c - 1) * pitch + n;               // (c - 1) <= 7, pitch <= 2^28: no overflow
  if (f > FRL_MAX_TOTAL) return false;
  *scalars = f;
  return true;
}
inline bool frl_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// ---- argument checks: NULL when the arguments are fine, or the text of the refusal ------------------------------------------------
// building a table from c columns of `rows` scalars, column j at j * pitch scalars (device: pointers are device pointers, aligned)
inline const char* frl_table_check(int c, const void* t, size_t pitch, size_t rows, bool device) {
  if (c < 1 || c > FRL_MAX_COLS) return "fr_lookup: c must be in [1, 8]";
  if (rows < 1 || rows > FRL_MAX_ROWS) return "fr_lookup: rows must be in [1, 2^24]";
  if (!t) return "fr_lookup: NULL table";
  if (pitch < rows) return "fr_lookup: pitch must be at least rows";
  size_t fp;
  if (!frl_footprint(c, pitch, rows, &fp)) return "fr_lookup: (c - 1) * pitch + rows must not exceed 2^28";
  if (device && ((uintptr_t)t & 15)) return "fr_lookup: device pointers must be 16-byte aligned";
  return nullptr;
}
struct FrlCountArgs {
  int c = 0; size_t rows = 0;                                 // of the handle
  const void* f = nullptr; size_t pitch = 0, n = 0; int negate = 0;
  const void* mult = nullptr; const void* index = nullptr; const void* missing = nullptr;
  bool device = false;
};
inline const char* frl_count_check(const FrlCountArgs& a) {
  if (a.c < 1 || a.c > FRL_MAX_COLS || a.rows < 1 || a.rows > FRL_MAX_ROWS) return "fr_lookup_count: the handle is not a built table";
  if (a.negate != 0 && a.negate != 1) return "fr_lookup_count: negate must be 0 or 1";
  if (a.n > FRL_MAX_TOTAL) return "fr_lookup_count: n must not exceed 2^28";
  if (a.n && !a.f) return "fr_lookup_count: NULL f with rows to look up";
  if (a.pitch < a.n) return "fr_lookup_count: pitch must be at least n";
  size_t fp;
  if (!frl_footprint(a.c, a.pitch, a.n, &fp)) return "fr_lookup_count: (c - 1) * pitch + n must not exceed 2^28";
  if (a.device) {
    if ((a.n && ((uintptr_t)a.f & 15)) || ((uintptr_t)a.mult & 15)) return "fr_lookup_count: device pointers must be 16-byte aligned";
    if ((uintptr_t)a.index & 3) return "fr_lookup_count: d_index must be 4-byte aligned";
    if ((uintptr_t)a.missing & 7) return "fr_lookup_count: d_missing must be 8-byte aligned";
  }
  const size_t fb = a.n ? fp * 32 : 0, mb = a.rows * 32, ib = a.n * 4, sb = 8;
  if (frl_overlap(a.mult, mb, a.f, fb) || frl_overlap(a.index, ib, a.f, fb) || frl_overlap(a.missing, sb, a.f, fb)) return "fr_lookup_count: an output overlaps f";
  if (frl_overlap(a.mult, mb, a.index, ib) || frl_overlap(a.mult, mb, a.missing, sb) || frl_overlap(a.index, ib, a.missing, sb))
    return "fr_lookup_count: the outputs overlap each other";
  return nullptr;
}

// ---- the launch plan ---------------------------------------------------------------------------------------------------------------
struct FrLookupPlan {
  int ok = 0;                          // 0: refused (rows, n or the block out of range)
  size_t slots = 0;
  unsigned block = 0;
  unsigned build_grid = 0;             // k_frl_build: one lane per table row
  int lds_path = 0;                    // 1: counters by row in LDS (rows <= lds_rows); 0: the cache in front of the global counters
  size_t count_lds = 0;                // bytes of dynamic LDS of k_frl_count
  unsigned count_grid = 0, iters = 0;  // k_frl_count: lane l of workgroup g takes the rows (it * count_grid + g) * block + l, it < iters
  unsigned finish_grid = 0;            // k_frl_finish: one lane per table row
};
// lds_rows: FRL_LDS_ROWS in the product; the tests lower it so that a small table takes path 2
inline FrLookupPlan fr_lookup_plan(size_t rows, size_t n, int block = FRL_BLOCK, size_t lds_rows = FRL_LDS_ROWS) {
  FrLookupPlan p;
  if (rows < 1 || rows > FRL_MAX_ROWS || n > FRL_MAX_TOTAL) return p;
  if (block < 64 || block > 1024 || block % 64 || lds_rows > FRL_LDS_ROWS) return p;
  p.slots = frl_slots(rows);
  p.block = (unsigned)block;
  p.build_grid = (unsigned)((rows + block - 1) / block);
  p.finish_grid = p.build_grid;
  p.lds_path = rows <= lds_rows ? 1 : 0;
  p.count_lds = p.lds_path ? rows * 4 : (size_t)FRL_CACHE * 8;
  const size_t batches = (n + block - 1) / block;
  p.count_grid = (unsigned)(batches < FRL_COUNT_GRID_MAX ? batches : FRL_COUNT_GRID_MAX);
  p.iters = p.count_grid ? (unsigned)((batches + p.count_grid - 1) / p.count_grid) : 0;
  p.ok = 1;
  return p;
}
static_assert(FRL_LDS_ROWS * 4 <= FRL_LDS_LIMIT && FRL_CACHE * 8 <= FRL_LDS_LIMIT, "the counters of either path fit the LDS a kernel gets unasked");

}  // namespace bls
