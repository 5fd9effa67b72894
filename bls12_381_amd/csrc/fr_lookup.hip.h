// fr_lookup.hip.h -- Fr lookup tables (blsgpu_fr_lookup_*): an index over the rows of a table of c-scalar keys, built once, and the
// count of how often each table row occurs among n looked-up rows -- the multiplicity column m of a logUp argument, which a prover
// commits to before it draws its challenges.  fr_lookup_plan.h holds the hash, the sizes, the launch shapes and the argument checks.
//
// Keys are compared as 8 c 32-bit words: inputs are canonical Montgomery limbs, so word equality is field equality.  No field
// arithmetic until the finishing pass turns a 32-bit count into a scalar (count * R mod r: scalar.hip.h's fr_to_mont).
//
// k_frl_build   one lane per table row.  It copies its key into the handle's row-major array, hashes it and probes linearly:
//               old = atomicCAS(&slot[h], 0, row + 1).  old == 0: the row owns the slot.  Otherwise, if row old - 1 has the same key, the
//               slot is lowered to the smaller row with atomicMin and the row is done; else the next slot.  A claimed slot's KEY never
//               changes (whatever row it names has the key that claimed it), only the representative falls, so no lane ever waits for
//               another: every iteration either ends the lane's work or moves it one slot on, and the loop is bounded by `slots`
//               iterations (at most `rows` <= slots / 2 slots are ever occupied, so an empty or matching one is met before that).
//               distinct = the number of successful claims: summed per workgroup in LDS, one global atomic per workgroup.
// k_frl_count   one lane per looked-up row, `iters` batches per workgroup.  The slot word is read with a plain load (the build ran in an
//               earlier launch): 0 is a miss, an equal key a hit at row v - 1.  BYROW (path 1): one LDS counter per table row.  Else
//               (path 2): a direct-mapped LDS cache {tag, count} of FRL_CACHE entries; the first row to reach an entry claims it for
//               the life of the workgroup (atomicCAS on the tag), a row that finds its entry taken by another adds to the global counter
//               directly.  At the end the workgroup adds every non-zero LDS count to the global counters (consecutive lanes on
//               consecutive words on path 1) and its misses to the 64-bit miss word: lookups that all hit one row cost one LDS
//               atomic each and one global atomic per workgroup.
// k_frl_finish  one lane per table row: counter -> canonical Montgomery scalar, negated if asked (0 stays 0).
//
// Only integer sums, so the results do not depend on the order the lanes arrive in.
#pragma once
#include "scalar.hip.h"
#include "fr_lookup_plan.h"

namespace bls {

// the hash of row i of a column set (column j at j * pitch scalars), optionally copying the key to `copy` (8 c words)
DEV u32 frl_hash_cols(const u32* __restrict__ t, size_t pitch, int c, size_t i, u32* copy) {
  u32 h = FRL_HASH_SEED;
  for (int j = 0; j < c; j++) {
    const Fr k = fr_load(t + ((size_t)j * pitch + i) * 8);
    if (copy) fr_store(copy + j * 8, k);
#pragma unroll
    for (int w = 0; w < 8; w++) h = frl_hash_step(h, k.l[w]);
  }
  return frl_hash_finish(h, (u32)(8 * c));
}
DEV bool frl_fr_equal(const Fr& a, const Fr& b) {
  u32 d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d |= a.l[w] ^ b.l[w];
  return d == 0;
}
// rows a and b of one column set hold the same key
DEV bool frl_equal_cols(const u32* __restrict__ t, size_t pitch, int c, size_t a, size_t b) {
  for (int j = 0; j < c; j++)
    if (!frl_fr_equal(fr_load(t + ((size_t)j * pitch + a) * 8), fr_load(t + ((size_t)j * pitch + b) * 8))) return false;
  return true;
}
// row i of the column set f holds the key at `key` (row-major, 8 c words)
DEV bool frl_equal_key(const u32* __restrict__ f, size_t pitch, int c, size_t i, const u32* __restrict__ key) {
#if defined(FRL_FAULT) && FRL_FAULT == 3
  c = 1;
#endif
  for (int j = 0; j < c; j++)
    if (!frl_fr_equal(fr_load(f + ((size_t)j * pitch + i) * 8), fr_load(key + j * 8))) return false;
  return true;
}

// t: c columns of `rows` scalars, column j at j * pitch; keys: rows * c scalars; slot: mask + 1 words, zeroed; distinct: one word, zeroed
__global__ void __launch_bounds__(FRL_BLOCK) k_frl_build(const u32* __restrict__ t, size_t pitch, u32 rows, int c, u32* __restrict__ keys, u32* slot, u32 mask, u32* distinct) {
  __shared__ unsigned wg_claimed;
  if (threadIdx.x == 0) wg_claimed = 0;
  __syncthreads();
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row < rows) {
    u32 h = frl_hash_cols(t, pitch, c, row, keys + row * (size_t)c * 8) & mask;
    for (u32 step = 0; step <= mask; step++) {
      const u32 old = atomicCAS(&slot[h], 0u, (u32)row + 1);
      if (old == 0) { atomicAdd(&wg_claimed, 1u); break; }
      if (frl_equal_cols(t, pitch, c, old - 1, row)) {
#if !(defined(FRL_FAULT) && FRL_FAULT == 1)
        atomicMin(&slot[h], (u32)row + 1);
#endif
        break;
      }
      h = (h + 1) & mask;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && wg_claimed) atomicAdd(distinct, wg_claimed);
}

// f: c columns of n scalars, column j at j * pitch; keys / slot: the handle's; counters: `rows` words, zeroed (NULL: nothing is counted);
// index: n words or NULL; missing: one 64-bit word, zeroed, or NULL.  Dynamic LDS: rows * 4 bytes (BYROW) or FRL_CACHE * 8.
template <bool BYROW>
__global__ void __launch_bounds__(FRL_BLOCK) k_frl_count(const u32* __restrict__ f, size_t pitch, size_t n, int c, const u32* __restrict__ keys, const u32* __restrict__ slot, u32 mask,
                                                          u32 rows, unsigned iters, u32* counters, u32* __restrict__ index, unsigned long long* missing) {
  BLS_DYN_LDS(lds);
  __shared__ unsigned wg_miss;
  const unsigned block = blockDim.x, lane = threadIdx.x;
  const u32 entries = BYROW ? rows : 2 * FRL_CACHE;
  if (counters) for (u32 e = lane; e < entries; e += block) lds[e] = 0;
  if (lane == 0) wg_miss = 0;
  __syncthreads();
  for (unsigned it = 0; it < iters; it++) {
    const size_t i = ((size_t)it * gridDim.x + blockIdx.x) * block + lane;
    if (i >= n) break;
    u32 h = frl_hash_cols(f, pitch, c, i, nullptr) & mask;
    u32 hit = 0;                                       // row + 1
    for (u32 step = 0; step <= mask; step++) {
      const u32 v = slot[h];
      if (v == 0) break;
      if (frl_equal_key(f, pitch, c, i, keys + (size_t)(v - 1) * c * 8)) { hit = v; break; }
#if defined(FRL_FAULT) && FRL_FAULT == 2
      h = h + 1;
#else
      h = (h + 1) & mask;
#endif
    }
#if defined(FRL_FAULT) && FRL_FAULT == 5
    if (index) index[i] = hit ? hit - 1 : 0u;
#else
    if (index) index[i] = hit ? hit - 1 : FRL_MISS;
#endif
    if (!hit) { atomicAdd(&wg_miss, 1u); continue; }
    if (!counters) continue;
    if (BYROW) {
      atomicAdd(&lds[hit - 1], 1u);
    } else {
      const u32 e = frl_cache_entry(hit - 1);
      const u32 tag = atomicCAS(&lds[e], 0u, hit);     // a tag is written once: the entry is this row's, or another's for good
      if (tag == 0 || tag == hit) atomicAdd(&lds[FRL_CACHE + e], 1u);
      else atomicAdd(&counters[hit - 1], 1u);
    }
  }
  __syncthreads();
  if (lane == 0 && wg_miss && missing) atomicAdd(missing, (unsigned long long)wg_miss);
  if (!counters) return;
#if defined(FRL_FAULT) && FRL_FAULT == 4
  {                                                    // a workgroup whose last batch is a partial one drops what it gathered
    const size_t last = ((size_t)(iters - 1) * gridDim.x + blockIdx.x) * block;
    if (last < n && last + block > n) return;
  }
#endif
  if (BYROW) {
    for (u32 e = lane; e < rows; e += block) { const u32 v = lds[e]; if (v) atomicAdd(&counters[e], v); }
  } else {
    for (u32 e = lane; e < FRL_CACHE; e += block) { const u32 tag = lds[e], v = lds[FRL_CACHE + e]; if (tag && v) atomicAdd(&counters[tag - 1], v); }
  }
}

// counters: `rows` words; mult: `rows` scalars
__global__ void __launch_bounds__(FRL_BLOCK) k_frl_finish(const u32* __restrict__ counters, u32 rows, int negate, u32* __restrict__ mult) {
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  Fr v = fr_zero();
  v.l[0] = counters[row];
  v = fr_to_mont(v);
  if (negate) v = fr_neg(v);
  fr_store(mult + row * 8, v);
}

}  // namespace bls
