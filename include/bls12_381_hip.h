/* bls12_381_hip.h -- C ABI of the MI355X-native BLS12-381 hot path (libblsgpu.so).
 *
 * This is the drop-in boundary for the data-parallel path of zkcrypto/bls12_381 v0.8.0: multi-scalar
 * multiplication over G1/G2 and batched Miller-loop / final-exponentiation pairings.  The reference has
 * no FFI (it is `#![deny(unsafe_code)]`, src/lib.rs:17); each entry point below names the Rust
 * operator / trait method it replaces.  INTEGRATION.md shows the `extern "C"` block and the wrapper a
 * maintainer would add on the Rust side.
 *
 * Wire formats (all little-endian, plain memory, caller-owned):
 *   Fp      6 x u64   canonical Montgomery limbs, R = 2^384       (`Fp([u64;6])`, src/fp.rs:11-15)
 *   Fp2     c0 | c1                                               (src/fp2.rs:11-14)
 *   Fp12    c0.c0.c0 c0.c0.c1 c0.c1.c0 ... c1.c2.c1 (72 u64)      (src/fp12.rs:13-16, src/fp6.rs:12-16)
 *   Scalar  32 bytes, little-endian canonical integer in [0, r)   (`Scalar::to_bytes`, src/scalar.rs:284-296)
 *   G1 affine      x | y          (12 u64)  + out-of-band infinity byte   (src/g1.rs:28-32)
 *   G1 projective  X | Y | Z      (18 u64), x = X/Z, identity (0:1:0)     (src/g1.rs:442-446,605-611)
 *   G2 affine      x.c0 x.c1 y.c0 y.c1 (24 u64) + infinity byte           (src/g2.rs)
 *   G2 projective  36 u64
 * Results are exact group / field elements in canonical limbs: after affine conversion (G1/G2) or as they
 * are (Gt) they are bit-identical to what the reference computes on the same inputs.
 *
 * Every function returns BLSGPU_OK (0) or a negative error code; nothing is retained from caller buffers
 * after return.  A context owns one device, one HIP stream and its scratch memory; it is not re-entrant
 * (use one context per host thread).  The rule is enforced: an entry point called while another host thread is inside an
 * entry point of the SAME context returns BLSGPU_ERR_ARG ("the context is in use by another host thread") and touches
 * nothing; contexts are independent of one another (tests: two contexts on two threads; one context from two threads).
 */
#ifndef BLS12_381_HIP_H
#define BLS12_381_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLSGPU_OK 0
#define BLSGPU_ERR_HIP (-1)      /* a HIP runtime call failed (blsgpu_last_error gives the text) */
#define BLSGPU_ERR_ARG (-2)      /* bad argument (NULL pointer, length mismatch, unsupported size) */
#define BLSGPU_ERR_NODEV (-3)    /* no usable gfx950 device */

typedef struct blsgpu_ctx blsgpu_ctx;
typedef struct blsgpu_bases blsgpu_bases;   /* device-resident base points in the library's internal form */

/* ---- context ------------------------------------------------------------------------------------ */
int blsgpu_create(int device, blsgpu_ctx** out);
void blsgpu_destroy(blsgpu_ctx* ctx);
const char* blsgpu_last_error(void);
int blsgpu_device_count(void);
/* Use an existing HIP stream (e.g. torch's current stream) for all work of this context; NULL restores
 * the context's own stream. */
int blsgpu_set_stream(blsgpu_ctx* ctx, void* hip_stream);
/* Wait for everything queued on the context.  Scalars must be canonical (< r; `Scalar::to_bytes` produces nothing else): a
 * synchronous entry point (`*_msm`, `*_msm_many`, `*_msm_bytes`, `*_msm_host`, `*_mul_batch`) that meets one returns
 * BLSGPU_ERR_ARG ITSELF -- its verdict travels with its result; the asynchronous `*_device` entry points cannot, so their
 * verdict is kept in a sticky flag that THIS call reports (BLSGPU_ERR_ARG) and clears.  A valid synchronous call is never blamed
 * for an earlier asynchronous one. */
int blsgpu_synchronize(blsgpu_ctx* ctx);
/* MSM pipelining.  An MSM is three phases with different bottlenecks: digit sort (LDS atomics), bucket
 * accumulation (integer VALU) and a latency-bound tail (bucket reduction + window combine: a few wavefronts
 * for ~ms).  The library runs them on internal streams chained by events.  By default the context's stream
 * waits for the tail, so results are ordered like any other work on that stream.  With pipelining on,
 * `*_msm_device` only records a dependency on the work already queued on the context's stream (the producer
 * of the scalars) and returns; sort, accumulation and tail of up to four calls then overlap one another.
 * The caller must keep each call's scalars and output buffer untouched, and use `blsgpu_join` (stream-level
 * wait, no host sync) or `blsgpu_synchronize` before consuming results. */
int blsgpu_set_pipelining(blsgpu_ctx* ctx, int enabled);
int blsgpu_join(blsgpu_ctx* ctx);
/* As blsgpu_join, but leaves the `lag` most recent MSM calls in flight (lag = 1: wait for everything except
 * the call just enqueued -- the pattern "enqueue MSM i, consume result i-1"). */
int blsgpu_join_lag(blsgpu_ctx* ctx, int lag);

/* ---- resident bases ------------------------------------------------------------------------------- */
/* Upload n affine points (host memory).  `infinity` may be NULL (no identities).
 * Replaces holding a `&[G1Affine]` / `&[G2Affine]` on the Rust side. */
int blsgpu_g1_bases_upload(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t n, blsgpu_bases** out);
int blsgpu_g2_bases_upload(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t n, blsgpu_bases** out);
/* Same, but `xy` / `infinity` are device pointers (e.g. torch tensors' data_ptr). */
int blsgpu_g1_bases_from_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t n, blsgpu_bases** out);
int blsgpu_g2_bases_from_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t n, blsgpu_bases** out);
/* bases[i] = [k_i] * generator for n 32-byte LE scalars (device-side fixed-base multiplication; used to
 * build synthetic inputs and SRS-style tables).  `group` is 1 or 2. */
int blsgpu_bases_from_scalars(blsgpu_ctx* ctx, int group, const uint8_t* scalars, size_t n, blsgpu_bases** out);
/* Optional, for bases that are reused (an SRS): build resident window-shifted tables [2^(c*w)] P_i (W x the memory;
 * W = ceil(256/c), c = window_bits, 0 -> 20).  Later MSMs over these bases put every window into ONE bucket set:
 * no window combine, a W-times smaller bucket reduction, fewer windows.  Requires n * W <= 2^24.  Results are the
 * same group elements.  The default width is the tuned one (2^20 points: 2.5 ms per pipelined MSM against 2.8 without tables); 16 works
 * as well, the widths between and 21 are correct but 1.3-1.6x slower (the sort's bin geometry). */
int blsgpu_bases_precompute(blsgpu_ctx* ctx, blsgpu_bases* b, int window_bits);
size_t blsgpu_bases_len(const blsgpu_bases* b);
/* Subgroup contract of the MSM.  The reference's `multiply` (src/g1.rs:754-774, src/g2.rs:825-845) is plain
 * double-and-add and therefore defined for EVERY curve point, including the on-curve points outside the prime-order
 * subgroup that `from_uncompressed_unchecked` / `from_compressed_unchecked` (src/g1.rs:273-322, 336-390) hand out.  The
 * fast MSM path splits scalars with the endomorphisms phi (G1) / psi (G2), whose eigenvalue relations hold only on the
 * subgroup.  Every upload therefore runs the reference's own `is_on_curve() & is_torsion_free()` (src/g1.rs:396-416,
 * src/g2.rs:475-489) over the set once, on the device: sets that pass keep endomorphism images and take the fast path;
 * a set with ANY point outside the subgroup runs on plain 256-bit windows with complete addition formulas, which
 * compute sum [s_i]P_i for arbitrary curve points exactly as the reference's `multiply` + `Sum` do.  Either way the
 * result is the reference's group element.  Bases built by blsgpu_bases_from_scalars are multiples of the generator and
 * skip the test.  A caller that already knows its points are in the subgroup (e.g. `G1Affine` values that came from
 * the checked decoders) may skip the per-upload test with blsgpu_set_assume_subgroup(ctx, 1); with that flag set,
 * results for off-subgroup inputs are unspecified.  Default: 0 (test every upload).
 * blsgpu_bases_subgroup_state: 1 = verified (or built as [k]G), 2 = assumed by the caller, 0 = at least one point is
 * outside the subgroup (plain windows), 3 = not tested: the set is beyond the size the split supports (G2: more than 2^22
 * points) and runs on plain windows in any case.
 * The ONE-SHOT entry points (blsgpu_g{1,2}_msm_host, blsgpu_g{1,2}_msm_bytes) upload a set for a single MSM: the test would
 * cost several times the MSM it speeds up, so they skip it and run on plain windows (exact for every curve point, state 3)
 * unless blsgpu_set_assume_subgroup(ctx, 1) is set, in which case they take the fast path untested.
 * Synchronisation: an upload that runs the test (`*_bases_upload`, `*_bases_from_device` with the default
 * assume_subgroup = 0) reads the verdict back and therefore SYNCHRONISES the context's stream (blsgpu_set_stream: the
 * caller's stream) -- it blocks the host and cannot be captured into a graph.  With blsgpu_set_assume_subgroup(ctx, 1)
 * `*_bases_from_device` only enqueues work and returns. */
int blsgpu_set_assume_subgroup(blsgpu_ctx* ctx, int enabled);
int blsgpu_bases_subgroup_state(const blsgpu_bases* b);
/* Read points [first, first+count) back in wire format (xy: count*12 or count*24 u64; infinity: count bytes). */
int blsgpu_bases_download(blsgpu_ctx* ctx, const blsgpu_bases* b, size_t first, size_t count, uint64_t* xy, uint8_t* infinity);
void blsgpu_bases_free(blsgpu_bases* b);

/* ---- multi-scalar multiplication ------------------------------------------------------------------- */
/* out = sum_{i<n} scalars[i] * bases[first + i]   as a projective point (18 / 36 u64).
 * Replaces  bases.iter().zip(scalars).map(|(p, s)| p * s).sum::<G1Projective>()
 * (`Mul<&Scalar> for &G1Affine` src/g1.rs:573-579 -> `multiply` :754-774, `Sum` :161-171; G2: src/g2.rs:626-632,
 * 825-845, 162-172).  n = 0 yields the identity (0:1:0). */
int blsgpu_g1_msm(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, uint64_t out_xyz[18]);
int blsgpu_g2_msm(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, uint64_t out_xyz[36]);
/* Asynchronous variants: scalars and the result live in device memory, work is enqueued on the
 * context's stream and the call returns without synchronising. */
int blsgpu_g1_msm_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, void* d_out_xyz);
int blsgpu_g2_msm_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, void* d_out_xyz);
/* Scalars as the reference STORES them.  Every entry point above (and blsgpu_*_mul_batch*, blsgpu_gt_mul_scalar_batch*, the `*_many`,
 * `*_host` and `*_sharded` MSMs) reads n x 32 bytes per scalar vector; what the 32 bytes are is the context's scalar form:
 *   BLSGPU_SCALAR_BYTES (default)  the canonical little-endian integer, `Scalar::to_bytes()` (src/scalar.rs:284-296), the bit source
 *                                  of `multiply` (src/g1.rs:559-561);
 *   BLSGPU_SCALAR_MONT             the four u64 Montgomery limbs of `Scalar([u64; 4])` (src/scalar.rs:23-27), i.e. the memory of a
 *                                  `&[Scalar]`: `to_bytes` = one `montgomery_reduce` (src/scalar.rs:506-550) then runs on the device,
 *                                  fused into the kernels that decompose the scalars, and an in-tree `msm(&[G1Affine], &[Scalar])`
 *                                  passes its slice as it is (2^20 host-side `to_bytes` calls cost several times the MSM).
 * Limbs / bytes that no `Scalar` can hold (>= r) are reported like non-canonical bytes (BLSGPU_ERR_ARG from the synchronous entry
 * points / blsgpu_synchronize).  blsgpu_set_scalar_form changes the form for all later calls on the context (members of a device
 * group: through blsgpu_group_ctx); the `*_mont` entry points are the four MSMs above with BLSGPU_SCALAR_MONT for that one call.
 * blsgpu_g{1,2}_msm_bytes always take `to_bytes()` output. */
#define BLSGPU_SCALAR_BYTES 0
#define BLSGPU_SCALAR_MONT 1
int blsgpu_set_scalar_form(blsgpu_ctx* ctx, int form);
int blsgpu_g1_msm_mont(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint64_t* scalars, size_t n, uint64_t out_xyz[18]);
int blsgpu_g2_msm_mont(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint64_t* scalars, size_t n, uint64_t out_xyz[36]);
int blsgpu_g1_msm_mont_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, void* d_out_xyz);
int blsgpu_g2_msm_mont_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, void* d_out_xyz);
/* k MSMs over the same resident bases (k scalar vectors of n x 32 bytes back to back -> k projective results back to back),
 * e.g. commitments to k polynomials under one SRS.  Synchronous like blsgpu_g1_msm, but the k calls run through the
 * library's pipeline (sort / accumulation / tail of consecutive MSMs overlap): the sustained rate of the asynchronous API
 * without managing streams. */
int blsgpu_g1_msm_many(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, size_t k, uint64_t* out_xyz);
int blsgpu_g2_msm_many(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const uint8_t* scalars, size_t n, size_t k, uint64_t* out_xyz);
int blsgpu_g1_msm_many_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, size_t k, void* d_out_xyz);
int blsgpu_g2_msm_many_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, size_t first, const void* d_scalars, size_t n, size_t k, void* d_out_xyz);
/* Segmented MSM: k independent small MSMs of different lengths, each over its own slice of the resident bases, in one call
 * (e.g. the verifier equations of many proofs, randomised batch checks grouped by key, commitments to many short polynomials):
 *   out[j] = sum_{i < len_j} scalars[offsets[j] + i] * bases[base_first[j] + i],   len_j = offsets[j+1] - offsets[j],  j < k.
 * offsets holds k + 1 non-decreasing u32 values with offsets[0] = 0; total = offsets[k] scalars of 32 bytes.  base_first holds k
 * u32 values; base_first == NULL means base_first[j] = offsets[j] (points and scalars side by side).  Slices may overlap (a shared
 * SRS prefix: base_first all 0).  Results are k projective wire points (18 / 36 u64 each): possibly another representative than
 * `*_msm` returns, the same affine point.  Exact for every curve point, as `*_msm` is: the endomorphism split is used only for sets
 * in the subgroup (state 1 or 2) whose images are resident, plain 256-bit windows otherwise.  An empty segment gives the identity;
 * k = 0 does nothing.
 * Limits: len_j <= BLSGPU_SEG_LEN_MAX, total <= 2^27, k <= 2^27.  Longer MSMs belong to `*_msm` / `*_msm_many` (at 4096 points
 * the segmented path is still faster than `*_msm_many` over shared bases; profiles/msm_segments_time.json).
 * Host form: scalars are ALWAYS `Scalar::to_bytes()` output, whatever blsgpu_set_scalar_form says (as `*_msm_bytes`).  Offsets,
 * lengths and base ranges are checked before anything is staged (BLSGPU_ERR_ARG); a scalar >= r gives BLSGPU_ERR_ARG from the call.
 * Device form: d_offsets / d_base_first / d_scalars / d_out_xyz in device memory, `total` = offsets[k] as the caller knows it; the
 * scalars follow the context's scalar form (a `blsgpu_fr_from_bytes_device` -> segments chain needs no conversion).  Enqueued on the
 * context's stream without synchronising.  A segment that breaks the rules above (decreasing offsets, offsets[j+1] > total, too
 * long, bases outside the set) and a scalar >= r are reported by the next blsgpu_synchronize (BLSGPU_ERR_ARG); the value of a bad
 * segment is unspecified.  Both forms use scratch of their own, not the buffers of pipelined `*_msm_device` calls in flight. */
#define BLSGPU_SEG_LEN_MAX 4096
int blsgpu_g1_msm_segments(blsgpu_ctx* ctx, const blsgpu_bases* bases, const uint32_t* base_first, const uint32_t* offsets,
                           const uint8_t* scalars, size_t k, uint64_t* out_xyz);
int blsgpu_g2_msm_segments(blsgpu_ctx* ctx, const blsgpu_bases* bases, const uint32_t* base_first, const uint32_t* offsets,
                           const uint8_t* scalars, size_t k, uint64_t* out_xyz);
int blsgpu_g1_msm_segments_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, const void* d_base_first, const void* d_offsets,
                                  const void* d_scalars, size_t k, size_t total, void* d_out_xyz);
int blsgpu_g2_msm_segments_device(blsgpu_ctx* ctx, const blsgpu_bases* bases, const void* d_base_first, const void* d_offsets,
                                  const void* d_scalars, size_t k, size_t total, void* d_out_xyz);
/* Opt-in cache for callers that pass the SAME base array to the one-shot entry points again and again (a drop-in `msm(&bases, &scalars)`
 * over an SRS: the reference's surface has no resident handle).  entries = 0 (default) switches it off and drops what is cached.  An
 * array is recognised by its length and a fingerprint of 64 evenly spaced points, so the caller promises NOT to modify an array it
 * passes again.  First sight: the one-shot path as always.  Second sight: the set is uploaded as resident bases (subgroup test,
 * endomorphism images) and kept; later calls only move their scalars and run on the path of blsgpu_g1_msm. */
int blsgpu_set_bases_cache(blsgpu_ctx* ctx, int entries);
/* HAZARD of the cache above: with the default fingerprint a caller that reuses a same-length buffer and changes only points that are
 * not among the 65 sampled ones gets an MSM over the STALE resident bases, with no error.  blsgpu_set_bases_cache_verify(ctx, 1) makes the
 * cache recognise an array by a hash of every word instead (four host threads, ~3 ms per 2^20 G1 points per call): use it unless the
 * arrays are known to be immutable (an SRS loaded once).  Switching the mode drops what is cached. */
int blsgpu_set_bases_cache_verify(blsgpu_ctx* ctx, int enabled);
/* One-shot convenience: upload, multiply, free.  No subgroup test and no endomorphism split (plain windows: exact for every
 * curve point) unless blsgpu_set_assume_subgroup(ctx, 1) -- see the subgroup contract above.  For a set used more than once
 * upload it (blsgpu_g1_bases_upload) and call blsgpu_g1_msm. */
int blsgpu_g1_msm_host(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint8_t* scalars, size_t n, uint64_t out_xyz[18]);
int blsgpu_g2_msm_host(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint8_t* scalars, size_t n, uint64_t out_xyz[36]);
/* The same on the reference's PUBLIC encodings, for a wrapper crate that cannot reach limbs (`pub(crate)`, src/g1.rs:28-32):
 * bases = n x 96 (G1) / n x 192 (G2) bytes of `to_uncompressed()` (decoded like `from_uncompressed_unchecked`,
 * src/g1.rs:271-322), scalars = n x 32 bytes of `Scalar::to_bytes()`, out = `to_uncompressed()` of the affine sum. */
int blsgpu_g1_msm_bytes(blsgpu_ctx* ctx, const uint8_t* bases_uncompressed, const uint8_t* scalars, size_t n, uint8_t out[96]);
int blsgpu_g2_msm_bytes(blsgpu_ctx* ctx, const uint8_t* bases_uncompressed, const uint8_t* scalars, size_t n, uint8_t out[192]);
/* Window width c (bits) used by Pippenger; 0 = automatic, otherwise 4..16 (the LDS counting sort keys on 8 + 7 bits of
 * |digit|; wider windows exist only with resident tables, blsgpu_bases_precompute, which carry their own width).  With the
 * endomorphism split active (see the subgroup contract above) the width applies to the 128-bit (G1) / 64-bit (G2)
 * sub-scalars: c = 16 then means 8 (G1) / 4 (G2) windows instead of 16. */
int blsgpu_set_msm_window(blsgpu_ctx* ctx, int c);

/* ---- batched variable-base scalar multiplication ------------------------------------------------------------ */
/* out[i] = scalars[i] * points[i] for n independent (point, scalar) pairs: n affine points in, n projective points out
 * (18 / 36 u64 each).  Replaces n evaluations of `&G1Affine * &Scalar` / `&G2Affine * &Scalar` (src/g1.rs:556-594 ->
 * `multiply` :754-774; src/g2.rs:609-647, 825-845; the "scalar multiplication" points of benches/groups.rs:44,89,113,158).
 * Signed 4-bit windows over complete addition formulas: exact for every curve point (identity, scalars 0 and r - 1, points
 * outside the prime-order subgroup) -- no subgroup precondition.  The projective representative differs from the one the
 * reference's double-and-add produces; the group element (affine coordinates) is the same.  `infinity` may be NULL.
 * With blsgpu_set_assume_subgroup(ctx, 1) -- the caller vouches that every point lies in the prime-order subgroup, e.g. values
 * from the checked decoders -- the scalars are split with the endomorphisms as in the MSM (G1: two 127-bit halves, half the
 * doublings; G2: four 63-bit digits over psi, a quarter of the doublings); results for off-subgroup points are then
 * unspecified, as for the MSM. */
int blsgpu_g1_mul_batch(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint8_t* scalars, size_t n, uint64_t* out_xyz);
int blsgpu_g2_mul_batch(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint8_t* scalars, size_t n, uint64_t* out_xyz);
/* Same with device pointers, asynchronous on the context's stream. */
int blsgpu_g1_mul_batch_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_scalars, size_t n, void* d_out_xyz);
int blsgpu_g2_mul_batch_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_scalars, size_t n, void* d_out_xyz);
/* The same four with the scalars as Montgomery limbs (BLSGPU_SCALAR_MONT for that one call; `Mul<&Scalar>` calls `to_bytes` per
 * product, src/g1.rs:556-562). */
int blsgpu_g1_mul_batch_mont(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint64_t* scalars, size_t n, uint64_t* out_xyz);
int blsgpu_g2_mul_batch_mont(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint64_t* scalars, size_t n, uint64_t* out_xyz);
int blsgpu_g1_mul_batch_mont_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_scalars, size_t n, void* d_out_xyz);
int blsgpu_g2_mul_batch_mont_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_scalars, size_t n, void* d_out_xyz);

/* ---- group helpers ----------------------------------------------------------------------------------- */
/* out = sum of n projective points (`Sum for G1Projective`, src/g1.rs:161-171) -- the fold used after the
 * cross-GPU all-gather of per-rank partial results. */
int blsgpu_g1_sum(blsgpu_ctx* ctx, const uint64_t* xyz, size_t n, uint64_t out_xyz[18]);
int blsgpu_g2_sum(blsgpu_ctx* ctx, const uint64_t* xyz, size_t n, uint64_t out_xyz[36]);
/* Same with device pointers, asynchronous on the context's stream (no host round trip after the all-gather). */
int blsgpu_g1_sum_device(blsgpu_ctx* ctx, const void* d_xyz, size_t n, void* d_out_xyz);
int blsgpu_g2_sum_device(blsgpu_ctx* ctx, const void* d_xyz, size_t n, void* d_out_xyz);
/* Segmented, gathered sums: out_xyz[s] = sum of the points idx[t], t in [offsets[s], offsets[s + 1]), for nseg segments in ONE call
 * (`impl Sum for G1Projective` over `add_mixed`, src/g1.rs:161-171, 715-752; the same in g2.rs) -- the aggregate public keys of many
 * subsets of a resident key set, the per-column sums of a gathered commitment.
 *   points   npoints affine points in the wire format plus an infinity byte each: what `*_from_bytes_batch_device` and
 *            `*_batch_normalize_device` write.  npoints < 2^32.
 *   idx      `total` u32 indices into the points, or NULL: term t is then point t, and total <= npoints.  An index may repeat, within a
 *            segment and across segments.
 *   offsets  nseg + 1 u64 in CSR form: offsets[0] = 0, non-decreasing, offsets[nseg] = total; total <= 2^28, passed by value because
 *            the device form cannot read it back without stalling the stream (as `total_terms` of multi_miller_loop_many_device).
 *   out_xyz  nseg projective points (18 / 36 u64 each), the input form of `*_batch_normalize[_device]`.
 * The result is the group element: identity entries are skipped, an empty segment gives `identity()` = (0 : 1 : 0), P + P doubles,
 * P + (-P) is the identity, and a curve point outside the subgroup adds like any other (the complete formulas: no precondition).  The
 * projective representative is unspecified; compare after batch_normalize, as for mul_batch.
 * BLSGPU_ERR_ARG with nothing launched: a NULL array with work to do, total > 2^28, nseg > 2^28, npoints >= 2^32, total > npoints without
 * idx; in the host forms also offsets that do not start at 0, decrease or do not end at total, and an index >= npoints.
 * The device forms (8-byte aligned d_xy / d_offsets / d_out_xyz, 4-byte aligned d_idx) are asynchronous on the context's stream and use the
 * context's scratch.  They cannot refuse what only the device sees: an offset beyond total is clamped to it (offsets[0] is read as 0,
 * offsets[nseg] as total); offsets that DECREASE are not repaired -- nothing outside the caller's arrays is read or written, but the
 * values of the segments involved are unspecified (two workgroups may write one of them); and an index >= npoints is NEVER
 * dereferenced -- its term is skipped and a sticky flag is set, so that the next blsgpu_synchronize returns BLSGPU_ERR_ARG (as for a
 * non-canonical scalar); that segment's value is unspecified, every other is right. */
int blsgpu_g1_sum_segments(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t npoints, const uint32_t* idx, const uint64_t* offsets, size_t nseg,
                           size_t total, uint64_t* out_xyz);
int blsgpu_g2_sum_segments(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t npoints, const uint32_t* idx, const uint64_t* offsets, size_t nseg,
                           size_t total, uint64_t* out_xyz);
int blsgpu_g1_sum_segments_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t npoints, const void* d_idx, const void* d_offsets, size_t nseg,
                                  size_t total, void* d_out_xyz);
int blsgpu_g2_sum_segments_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t npoints, const void* d_idx, const void* d_offsets, size_t nseg,
                                  size_t total, void* d_out_xyz);
/* Projective -> affine for n points (`G1Projective::batch_normalize`, src/g1.rs:806-839; `G1Affine::from`,
 * :49-63).  Identity maps to x = 0, y = 1 (Montgomery one), infinity = 1. */
int blsgpu_g1_batch_normalize(blsgpu_ctx* ctx, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* infinity);
int blsgpu_g2_batch_normalize(blsgpu_ctx* ctx, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* infinity);

/* ---- batched point (de)serialisation and validation (the step in front of the hot path) ------------------ */
/* Decode n points from the reference's byte encodings (src/notes/serialization.rs): 48/96 B compressed or 96/192 B
 * uncompressed.  checked = 0: `from_compressed_unchecked` / `from_uncompressed_unchecked` (src/g1.rs:273-322, 336-390);
 * checked = 1: `from_compressed` (subgroup check, :326-332) / `from_uncompressed` (on-curve + subgroup, :264-267).
 * ok[i] = 1 exactly where the reference returns CtOption::some; rejected entries decode to the identity. */
int blsgpu_g1_from_bytes_batch(blsgpu_ctx* ctx, const uint8_t* bytes, size_t n, int compressed, int checked, uint64_t* xy, uint8_t* infinity, uint8_t* ok);
int blsgpu_g2_from_bytes_batch(blsgpu_ctx* ctx, const uint8_t* bytes, size_t n, int compressed, int checked, uint64_t* xy, uint8_t* infinity, uint8_t* ok);
/* Encode n affine points: `to_compressed` / `to_uncompressed` (src/g1.rs:221-260, src/g2.rs:254-299). */
int blsgpu_g1_to_bytes_batch(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t n, int compressed, uint8_t* out);
int blsgpu_g2_to_bytes_batch(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, size_t n, int compressed, uint8_t* out);

/* ---- pairings ------------------------------------------------------------------------------------------ */
/* Which kernels a call with n items (pairings, Miller loops or final exponentiations) runs on this context:
 *   256 = wide  (one item per 1024- or 512-lane workgroup: the small-batch latency path, n <= 1536; needs the generated
 *                program file `wide_prog.bin` next to the library -- build step of __graft_entry__.py -- or at
 *                $BLSGPU_WIDE_PROG),
 *     4 = quad  (one item per four lanes: the throughput path),
 *     2 = lane pair (the layout of rounds 1-2, kept for A/B runs).
 * BLSGPU_PAIRING_LAYOUT=wide|quad|pair|auto in the environment at blsgpu_create fixes the choice; with "wide" a missing
 * or mismatching program file makes the pairing entry points FAIL (BLSGPU_ERR_ARG) instead of silently running another
 * kernel; with "auto" (the default) the quad kernels take every size then, this function says so, and the library prints ONE
 * line to stderr the first time it happens (a single pairing costs ~6 ms instead of ~1.1 ms then).  Any other value of the
 * variable makes blsgpu_create fail with BLSGPU_ERR_ARG.  All layouts return limb-identical results. */
int blsgpu_pairing_layout(blsgpu_ctx* ctx, size_t n);
/* "" when the wide programs are loaded on this context, otherwise the reason they are not (file missing, stale format
 * version, generated for another kernel configuration, library path unknown in a static link: set $BLSGPU_WIDE_PROG). */
const char* blsgpu_wide_status(blsgpu_ctx* ctx);      /* (the pointer is valid until the next call on this context) */
/* out[i] = pairing(g1[i], g2[i]) for n independent pairs (`pairing`, src/pairings.rs:607-653; 72 u64 each).
 * An identity on either side yields Gt::identity() = Fp12::one(), as the reference does. */
int blsgpu_pairing_batch(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, uint64_t* out_gt);
/* out[i] = raw Miller-loop value of pair i (a `MillerLoopResult`, src/pairings.rs:26) -- bit-identical to the
 * reference's because the same line formulas are used (src/pairings.rs:696-770). */
int blsgpu_miller_loop_batch(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, uint64_t* out_f);
/* out = prod_i ML(g1[i], g2[i])  (`multi_miller_loop`, src/pairings.rs:554-603; pairs with an identity are
 * skipped).  n = 0 yields Fp12::one() (`MillerLoopResult::default`, :28-32). */
int blsgpu_multi_miller_loop(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, uint64_t out_f[72]);
/* N independent `multi_miller_loop`s in one call -- the shape of bulk signature verification, where generic `E: MultiMillerLoop`
 * callers evaluate one product of k pairings per equation (src/pairings.rs:554-603, 817-824; the test pattern :871-921).
 * Segment s = terms offsets[s] .. offsets[s+1] of the g1 / g2 arrays (CSR: nseg + 1 non-decreasing offsets, offsets[0] = 0).
 *   final_exp = 0: out[s] = multi_miller_loop(terms of s)                        (a `MillerLoopResult`, 72 u64)
 *   final_exp != 0: out[s] = multi_miller_loop(terms of s).final_exponentiation() (a `Gt`, 72 u64)
 * Terms with an identity on either side are skipped as the reference does (:566-569); an empty segment yields
 * `MillerLoopResult::default()` = Fp12::one() (:28-32), whose final exponentiation is `Gt::identity()`.  One batched Miller
 * kernel over all terms, one segmented Fp12 product, one batched final exponentiation; few terms take the wide path; from
 * 49 152 segments of at most 8 terms on, every segment shares one accumulator (the reference's own schedule) instead.  For
 * ONE product over very many terms blsgpu_multi_miller_loop is the faster entry point. */
int blsgpu_multi_miller_loop_many(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, const uint64_t* offsets,
                                  size_t nseg, int final_exp, uint64_t* out);
/* Device-pointer variant, asynchronous on the context's stream: points, flags, offsets (nseg + 1 u64) and the output in device
 * memory.  `total_terms` = offsets[nseg] and `max_seg_terms` = an upper bound of the segment lengths (0 = unknown) are passed
 * by value because the host cannot read the offsets without a synchronisation; offsets beyond total_terms are clamped, and a
 * segment longer than a max_seg_terms <= 8 the caller passed is reported by the next blsgpu_synchronize (BLSGPU_ERR_ARG; the
 * value of that segment is unspecified) -- the sticky flag of the asynchronous entry points, see blsgpu_synchronize. */
int blsgpu_multi_miller_loop_many_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, const void* d_offsets,
                                         size_t nseg, size_t total_terms, size_t max_seg_terms, int final_exp, void* d_out);
/* out[i] = final_exponentiation(in[i])  (`MillerLoopResult::final_exponentiation`, src/pairings.rs:48-176). */
int blsgpu_final_exponentiation_batch(blsgpu_ctx* ctx, const uint64_t* in_f, size_t n, uint64_t* out_gt);
/* out = prod of n Fp12 values (`MillerLoopResult + MillerLoopResult`, src/pairings.rs:179-186; `Gt + Gt`). */
int blsgpu_fp12_product(blsgpu_ctx* ctx, const uint64_t* in_f, size_t n, uint64_t out_f[72]);
/* `&Gt * &Scalar` (src/pairings.rs:297-322) for n (element, scalar) pairs: out[i] = gt[i] "times" scalars[i], i.e. the
 * Fp12 power by the canonical little-endian 32-byte scalar (double-and-add over its 255 low bits).  A scalar >= r (bytes, or limbs
 * in BLSGPU_SCALAR_MONT) gives BLSGPU_ERR_ARG. */
int blsgpu_gt_mul_scalar_batch(blsgpu_ctx* ctx, const uint64_t* gt, const uint8_t* scalars, size_t n, uint64_t* out);
/* Device-pointer variants (inputs/outputs in device memory, asynchronous on the context's stream). */
int blsgpu_pairing_batch_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, size_t n, void* d_out_gt);
int blsgpu_multi_miller_loop_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, size_t n, void* d_out_f);
/* raw Miller values of n pairs, final exponentiation of n values and the product of n values, device to device: the pieces a
 * sharded `multi_miller_loop` needs around its single exchange (rank-local product -> all-gather -> fold -> ONE final
 * exponentiation; src/pairings.rs:179-186, :48-176) and that a sharded batch of independent pairings keeps on the device. */
int blsgpu_miller_loop_batch_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, size_t n, void* d_out_f);
int blsgpu_final_exponentiation_device(blsgpu_ctx* ctx, const void* d_in_f, size_t n, void* d_out_gt);
int blsgpu_fp12_product_device(blsgpu_ctx* ctx, const void* d_in_f, size_t n, void* d_out_f);

/* ---- G2Prepared: line coefficients of FIXED G2 arguments resident on the device ----------------------------------------- */
/* `G2Prepared` (src/pairings.rs:487-502) holds the 68 coefficient triples of a point's doubling / addition steps, computed once
 * (`From<G2Affine> for G2Prepared`, :504-546), so that every later `multi_miller_loop` only EVALUATES them at P (:554-603 with
 * `ell`, :696-707): ~2.9 k field multiplications per term instead of ~6.9 k.  A `blsgpu_g2_prepared` is a device-resident table
 * of m such points in the library's limb form (26 112 B per point); verification keys (Groth16: three of four G2 arguments fixed)
 * and fixed generators (BLS) are prepared once and named by index afterwards.  The identity keeps its flag and is skipped by the
 * consumers as the reference skips it (:566-569).  The handle belongs to the context's device and outlives the context's calls;
 * free it with blsgpu_g2_prepared_free (after the work that reads it has completed). */
typedef struct blsgpu_g2_prepared blsgpu_g2_prepared;
int blsgpu_g2_prepare(blsgpu_ctx* ctx, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t m, blsgpu_g2_prepared** out);
/* the same with the points (24 u64 each) and flags in device memory; asynchronous on the context's stream */
int blsgpu_g2_prepare_device(blsgpu_ctx* ctx, const void* d_g2_xy, const void* d_g2_inf, size_t m, blsgpu_g2_prepared** out);
size_t blsgpu_g2_prepared_len(const blsgpu_g2_prepared* p);
void blsgpu_g2_prepared_free(blsgpu_g2_prepared* p);
/* The stored coefficients of point `index` in the reference's own value format -- `coeffs: Vec<(Fp2, Fp2, Fp2)>`, 68 triples of
 * 3 x 12 u64 canonical Montgomery limbs (2 448 u64) -- and its `infinity` flag: what an in-tree `G2Prepared` would hold, and the
 * parity hook against the oracle's `G2Prepared::from`. */
int blsgpu_g2_prepared_coeffs(blsgpu_ctx* ctx, const blsgpu_g2_prepared* p, size_t index, uint64_t* out_coeffs, uint8_t* out_inf);
/* `multi_miller_loop(&[(&G1Affine, &G2Prepared)])` (src/pairings.rs:554-603) with prepared and unprepared terms mixed: term i pairs
 * g1[i] with table point q_index[i], or -- q_index[i] = BLSGPU_UNPREPARED (or q_index = NULL: every term) -- with g2[i], whose
 * lines are computed on the fly as in blsgpu_multi_miller_loop (g2 may be NULL when every term is prepared).  out = the raw
 * `MillerLoopResult`, limb-identical to the unprepared entry points' and to the reference's.  An index outside the table is an
 * argument error (host-pointer forms) / reported by the next blsgpu_synchronize (device-pointer forms, where the term is skipped). */
#define BLSGPU_UNPREPARED 0xffffffffu
int blsgpu_multi_miller_loop_prepared(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, const uint32_t* q_index,
                                      const blsgpu_g2_prepared* prepared, size_t n, uint64_t out_f[72]);
int blsgpu_multi_miller_loop_prepared_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, const void* d_q_index,
                                             const blsgpu_g2_prepared* prepared, size_t n, void* d_out_f);
/* N independent products in one call (blsgpu_multi_miller_loop_many with prepared terms): segment s = terms offsets[s] ..
 * offsets[s+1]; every segment runs the reference's own schedule on one accumulator -- per step each term multiplies its line in,
 * one squaring for all -- so a verification equation with k terms pays 62 squarings, not 62 k, and a prepared term only its
 * `ell`s.  final_exp as in blsgpu_multi_miller_loop_many.  Segments of any length are accepted (more than 8 terms: several passes,
 * multiplied together); for ONE long product use blsgpu_multi_miller_loop_prepared. */
int blsgpu_multi_miller_loop_prepared_many(blsgpu_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, const uint32_t* q_index,
                                           const blsgpu_g2_prepared* prepared, const uint64_t* offsets, size_t nseg, int final_exp, uint64_t* out);
int blsgpu_multi_miller_loop_prepared_many_device(blsgpu_ctx* ctx, const void* d_g1_xy, const void* d_g1_inf, const void* d_g2_xy, const void* d_g2_inf, const void* d_q_index,
                                                  const blsgpu_g2_prepared* prepared, const void* d_offsets, size_t nseg, size_t total_terms, size_t max_seg_terms,
                                                  int final_exp, void* d_out);

/* ---- device groups: the path sharded over the GPUs of one node from ONE process ------------------------------------- */
/* "Large MSMs and pairing batches shard embarrassingly across the 8 GPUs" (SURVEY.md 8e): a group is one context per listed
 * device; every `*_sharded` call deals its independent terms to the members in contiguous slices (sizes differ by at most
 * one), runs each member on its own host thread, and folds the members' partial results -- ONE group element each: 144 B
 * G1, 288 B G2, 576 B Fp12 -- on member 0 with the reference's own operators: `Sum for G1Projective` (src/g1.rs:161-171,
 * src/g2.rs:162-172) and `MillerLoopResult + MillerLoopResult` (src/pairings.rs:179-186), then ONE final exponentiation
 * (:48-176).  Inside one process those few hundred bytes travel through host memory; no collective library is involved
 * (one process per GPU over RCCL is bls12_381_amd/distributed.py + bench.py --gpus N).  Results are the same group / field
 * elements as the single-context entry points'.  `devices` may name a device more than once (logical members on one GPU).
 * A group is driven by one host thread at a time; it owns one persistent worker thread per member beyond the first (created by
 * blsgpu_group_create, joined by blsgpu_group_destroy: no thread is started per call).  blsgpu_group_ctx gives access to a member's
 * context for the per-context settings (blsgpu_set_assume_subgroup, blsgpu_set_msm_window, ...).  The host-pointer `*_sharded`
 * calls are synchronous; the `*_sharded_device` MSMs below are asynchronous and pipelined. */
typedef struct blsgpu_group blsgpu_group;
typedef struct blsgpu_group_bases blsgpu_group_bases;   /* resident bases, member k holds points [lo_k, hi_k) on its device */
int blsgpu_group_create(const int* devices, int ndev, blsgpu_group** out);
void blsgpu_group_destroy(blsgpu_group* group);
int blsgpu_group_size(const blsgpu_group* group);
blsgpu_ctx* blsgpu_group_ctx(blsgpu_group* group, int member);
/* Shard n affine points (wire format as blsgpu_g1_bases_upload; `group_id` = 1 | 2) / the multiples [k_i]G over the members. */
int blsgpu_group_bases_upload(blsgpu_group* group, int group_id, const uint64_t* xy, const uint8_t* infinity, size_t n, blsgpu_group_bases** out);
int blsgpu_group_bases_from_scalars(blsgpu_group* group, int group_id, const uint8_t* scalars, size_t n, blsgpu_group_bases** out);
size_t blsgpu_group_bases_len(const blsgpu_group_bases* b);
void blsgpu_group_bases_free(blsgpu_group_bases* b);
/* out = sum_{i<n} scalars[i] * bases[i], n <= blsgpu_group_bases_len: every member runs a complete MSM over its slice,
 * member 0 adds the partial sums (blsgpu_g1_msm / blsgpu_g1_sum per member; same contracts, incl. canonical scalars). */
int blsgpu_g1_msm_sharded(blsgpu_group* group, const blsgpu_group_bases* bases, const uint8_t* scalars, size_t n, uint64_t out_xyz[18]);
int blsgpu_g2_msm_sharded(blsgpu_group* group, const blsgpu_group_bases* bases, const uint8_t* scalars, size_t n, uint64_t out_xyz[36]);
/* Device-pointer, asynchronous form for pipelined use (the headline path on every GPU of the node): member k multiplies its WHOLE
 * resident slice by the scalars at d_scalars[k] and writes its partial sum (18 / 36 u64) to d_partials[k], both in ITS device's memory;
 * the call only enqueues on every member (one persistent host thread per member does the enqueueing).  With
 * blsgpu_group_set_pipelining(group, 1) up to four calls per member overlap as described at blsgpu_set_pipelining.
 * blsgpu_g{1,2}_partials_fold(group, d_partials, lag, out) then waits -- per member, without holding up the `lag` most recent calls --
 * for the call whose partial sums `d_partials` name, and adds them on member 0 (`Sum`, src/g1.rs:161-171): the pattern is "enqueue MSM
 * i, fold MSM i - 2".  blsgpu_group_synchronize waits for everything and reports the sticky verdict of asynchronous calls. */
int blsgpu_g1_msm_sharded_device(blsgpu_group* group, const blsgpu_group_bases* bases, const void* const* d_scalars, void* const* d_partials);
int blsgpu_g2_msm_sharded_device(blsgpu_group* group, const blsgpu_group_bases* bases, const void* const* d_scalars, void* const* d_partials);
int blsgpu_g1_partials_fold(blsgpu_group* group, const void* const* d_partials, int lag, uint64_t out_xyz[18]);
int blsgpu_g2_partials_fold(blsgpu_group* group, const void* const* d_partials, int lag, uint64_t out_xyz[36]);
/* The fold without a host round trip: every member queues a copy of its partial sum to member 0's device behind the MSM it belongs to,
 * member 0's stream adds the w points into d_out (device memory of member 0, 18 / 36 u64); nothing is synchronised -- the fold of MSM
 * i - 3 runs under the accumulation of the later MSMs, on the members' own fold streams (an MSM's front waits for what is queued on its
 * context's stream, so the fold is kept off it).  At most four folds may be outstanding; an MSM whose output buffer one of the last eight
 * folds still has to read waits for that fold's copy, so a pipelined caller rotates at least eight partial-sum buffers per member (with
 * four, every MSM waits for the fold three calls back).  d_out is valid after blsgpu_group_synchronize. */
int blsgpu_g1_partials_fold_device(blsgpu_group* group, const void* const* d_partials, int lag, void* d_out_xyz);
int blsgpu_g2_partials_fold_device(blsgpu_group* group, const void* const* d_partials, int lag, void* d_out_xyz);
/* The pairing entry points in the same form: member k works on ITS arrays (device pointers in its memory, counts[k] items; the infinity
 * arrays may be NULL) and only enqueues.  mode 0: d_out[k] = counts[k] pairings (`Gt`), mode 1: raw Miller values -- the outputs stay sharded,
 * nothing to fold; mode 2: d_out[k] = the member-local `multi_miller_loop` of its terms (ONE Fp12 value), and
 * blsgpu_fp12_partials_fold_device(group, d_partials, final_exp, d_out) multiplies the members' values on member 0
 * (`MillerLoopResult + MillerLoopResult`, src/pairings.rs:179-186) and applies the ONE final exponentiation if asked; d_out (72 u64 in
 * member 0's memory) is valid after blsgpu_group_synchronize. */
int blsgpu_pairings_sharded_device(blsgpu_group* group, int mode, const void* const* d_g1_xy, const void* const* d_g1_inf, const void* const* d_g2_xy,
                                   const void* const* d_g2_inf, const size_t* counts, void* const* d_out);
int blsgpu_fp12_partials_fold_device(blsgpu_group* group, const void* const* d_partials, int final_exp, void* d_out_f);
int blsgpu_group_set_pipelining(blsgpu_group* group, int enabled);
int blsgpu_group_synchronize(blsgpu_group* group);
/* n independent pairings / raw Miller values: index slices, each member writes its slice of `out` (n x 72 u64); nothing to fold. */
int blsgpu_pairing_batch_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, uint64_t* out_gt);
int blsgpu_miller_loop_batch_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, uint64_t* out_f);
/* `multi_miller_loop` over n terms: member-local products of index slices, folded by member 0; final_exp != 0 applies the ONE
 * final exponentiation (out = a `Gt`), final_exp = 0 returns the `MillerLoopResult`. */
int blsgpu_multi_miller_loop_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, int final_exp,
                                     uint64_t out[72]);
/* Prepared G2 arguments for a group: the same m points prepared on EVERY member (blsgpu_g2_prepare per member), and the prepared Miller
 * loops sharded like the unprepared ones (terms / segments in contiguous slices, partial products folded on member 0, ONE final
 * exponentiation where asked). */
typedef struct blsgpu_group_g2_prepared blsgpu_group_g2_prepared;
int blsgpu_group_g2_prepare(blsgpu_group* group, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t m, blsgpu_group_g2_prepared** out);
size_t blsgpu_group_g2_prepared_len(const blsgpu_group_g2_prepared* p);
void blsgpu_group_g2_prepared_free(blsgpu_group_g2_prepared* p);
int blsgpu_multi_miller_loop_prepared_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, const uint32_t* q_index,
                                              const blsgpu_group_g2_prepared* prepared, size_t n, int final_exp, uint64_t out[72]);
int blsgpu_multi_miller_loop_prepared_many_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                                                   const uint32_t* q_index, const blsgpu_group_g2_prepared* prepared, const uint64_t* offsets, size_t nseg, int final_exp,
                                                   uint64_t* out);
/* blsgpu_multi_miller_loop_many with the SEGMENTS dealt to the members in contiguous slices. */
int blsgpu_multi_miller_loop_many_sharded(blsgpu_group* group, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                                          const uint64_t* offsets, size_t nseg, int final_exp, uint64_t* out);

/* ---- field self-test hooks (parity tests of the arithmetic core against the oracle) ---------------------- */
/* out[i] = a[i] op b[i] over n Fp elements in wire format; op: 0 mul, 1 add, 2 sub, 3 square(a), 4 invert(a), 5 neg(a). */
int blsgpu_fp_op(blsgpu_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Same over Fp2 (12 u64 per element); op: 0 mul, 1 add, 2 sub, 3 square, 4 invert, 5 neg, 6 mul_by_nonresidue. */
int blsgpu_fp2_op(blsgpu_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Same over Fp6 (36 u64 per element: c0 | c1 | c2, src/fp6.rs:12-16); op: 0 mul (fp6.rs:200-274), 3 square (:277-291), 4 invert
 * (:294-312), 5 mul_by_nonresidue (:139-150), 7 frobenius_map (:154-188), 11 mul_by_1 with c1 = b.c1 (:113-119), 12 mul_by_01 with
 * (c0, c1) = (b.c0, b.c1) (:121-136). */
int blsgpu_fp6_op(blsgpu_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Same over Fp12 (72 u64 per element); op: 0 mul, 3 square, 4 invert, 7 frobenius_map, 8 conjugate, 9 cyclotomic_square,
 * 10 the final exponentiation's power by |x| followed by conjugation (`cycolotomic_exp`, src/pairings.rs:114-132; quad layout only). */
int blsgpu_fp12_op(blsgpu_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Point ops over n pairs in wire format; op: 0 add (proj+proj), 1 double (a), 2 add_mixed (proj + affine b). group 1|2. */
int blsgpu_point_op(blsgpu_ctx* ctx, int group, int op, const uint64_t* a, const uint64_t* b, const uint8_t* b_inf, size_t n, uint64_t* out);
/* Throughput probe: `iters` dependent Fp multiplications in every lane of a full-chip launch; returns
 * multiplications per second (the arithmetic roofline evidence quoted by bench.py). */
int blsgpu_fp_mul_throughput(blsgpu_ctx* ctx, int iters, double* muls_per_second);
/* Same for a stream of independent v_mad_u64_u32 (the peak MAC32 rate used as roofline denominator). */
int blsgpu_mad_throughput(blsgpu_ctx* ctx, int iters, double* mads_per_second);
/* Duration (ms) of the most recent launch of the named phase inside the last MSM (HIP events on the
 * context's stream): 0 digits+hist, 1 scan, 2 scatter, 3 order, 4 accumulate, 5 reduce, 6 combine, 7 total. */
int blsgpu_last_msm_phase_ms(blsgpu_ctx* ctx, int phase, float* ms);
int blsgpu_set_profiling(blsgpu_ctx* ctx, int enabled);
/* Live duration of the bucket-accumulation kernel (the dominant kernel of an MSM) measured with HIP events on the stream
 * it is launched on, also while calls are pipelined: returns the average over the launches since the previous call and
 * their number, then resets the statistics and switches the measurement off (enable = 0) or on: enable = N > 0 times every
 * N-th launch (two event records per timed launch cost ~0.05-0.1 ms of queue time in a pipelined run, so benchmarks sample). */
int blsgpu_msm_accumulate_stats(blsgpu_ctx* ctx, int enable, double* avg_ms, unsigned* launches);
/* Diagnostics: the duration of EVERY kernel the context's entry points launch, measured with HIP events on the stream each kernel is
 * launched on (a call's kernels run on up to four library streams, which a caller-side event never sees).  blsgpu_kernel_timing(ctx, 1)
 * starts recording (and clears earlier records), (ctx, 0) stops; blsgpu_kernel_timing_report waits for the recorded launches and writes one
 * line per kernel name in first-launch order -- "name<TAB>launches<TAB>total_ms<TAB>min_ms<TAB>max_ms\n" -- into buf (at most cap - 1
 * characters + NUL; the full length goes to *needed, which may be NULL), then clears the records.  Two event records per launch: meant
 * for one call at a time (bench.py's `kernel_ms` rows), not for pipelined production runs. */
int blsgpu_kernel_timing(blsgpu_ctx* ctx, int enable);
int blsgpu_kernel_timing_report(blsgpu_ctx* ctx, char* buf, size_t cap, size_t* needed);

/* ---- scalar field Fr (the producer side of the MSM's scalars) ----------------------- */
/* A scalar is the reference's `Scalar([u64; 4])`: four little-endian u64 Montgomery limbs (R = 2^256), canonical
 * (scalar.rs:23-27).  Element-wise vector operation over n scalars; op: 0 mul (scalar.rs:452-503), 1 add (:435-449),
 * 2 sub (:420-432), 3 square (:334-369), 4 invert (:573-628; a zero input yields 0 and nonzero_flags[i] = 0, the
 * reference's CtOption::none), 5 neg (:552-568), 6 double (:246-250).  `b` is ignored for unary ops,
 * `nonzero_flags` (n bytes) may be NULL. */
int blsgpu_fr_op(blsgpu_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, uint8_t* nonzero_flags);
int blsgpu_fr_op_device(blsgpu_ctx* ctx, int op, const void* d_a, const void* d_b, size_t n, void* d_out, void* d_nonzero_flags);
/* `Scalar` <-> bytes over vectors of n scalars:
 *   to_bytes         Montgomery limbs -> 32 canonical little-endian bytes, `Scalar::to_bytes` (src/scalar.rs:284-296: one
 *                    `montgomery_reduce`, :506-550); ok[i] = 0 where the limbs are not below r (no `Scalar` holds them);
 *   from_bytes       32 bytes -> Montgomery limbs (multiplication by R2), ok[i] = 0 where `Scalar::from_bytes` returns
 *                    CtOption::none: the integer is not below r (src/scalar.rs:256-280);
 *   from_bytes_wide  64 bytes -> the 512-bit little-endian integer mod r as d0 R2 + d1 R3 (src/scalar.rs:300-331); always defined.
 * `ok` (n bytes) may be NULL.  The device-pointer forms are asynchronous on the context's stream, e.g.
 * blsgpu_fr_ntt_device -> blsgpu_g1_msm_mont_device needs no conversion at all, and blsgpu_fr_to_bytes_device feeds the byte-form
 * entry points. */
int blsgpu_fr_to_bytes(blsgpu_ctx* ctx, const uint64_t* scalars, size_t n, uint8_t* bytes, uint8_t* ok);
int blsgpu_fr_from_bytes(blsgpu_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* scalars, uint8_t* ok);
int blsgpu_fr_from_bytes_wide(blsgpu_ctx* ctx, const uint8_t* bytes, size_t n, uint64_t* scalars);
int blsgpu_fr_to_bytes_device(blsgpu_ctx* ctx, const void* d_scalars, size_t n, void* d_bytes, void* d_ok);
int blsgpu_fr_from_bytes_device(blsgpu_ctx* ctx, const void* d_bytes, size_t n, void* d_scalars, void* d_ok);
int blsgpu_fr_from_bytes_wide_device(blsgpu_ctx* ctx, const void* d_bytes, size_t n, void* d_scalars);
/* Radix-2 number-theoretic transform of 2^log_n scalars, in place, natural order in and out:
 *   forward  y_k = sum_j x_j w^(jk),   inverse  x_j = n^-1 sum_k y_k w^(-jk),   w = ROOT_OF_UNITY^(2^(32 - log_n))
 * with the reference's ROOT_OF_UNITY / S = 32 (scalar.rs:191-205, exported through ff::PrimeField :703-712).
 * The reference crate has no transform of its own; this is the operation its callers build on those constants.
 * log_n in [0, 28]. */
int blsgpu_fr_ntt(blsgpu_ctx* ctx, uint64_t* data, int log_n, int inverse);
int blsgpu_fr_ntt_device(blsgpu_ctx* ctx, void* d_data, int log_n, int inverse);
/* k independent transforms of 2^log_n scalars each in ONE call, in place; vector v occupies scalars [v * 2^log_n, (v+1) * 2^log_n)
 * of data (the producer side of blsgpu_g{1,2}_msm_segments: 256 polynomials of 4096 coefficients are one call, not 256).
 * coset == NULL: each vector exactly as blsgpu_fr_ntt (limb-identical results).  coset = g, the four Montgomery limbs of a non-zero
 * canonical Scalar -- a HOST pointer in both forms: it is a parameter, not data -- e.g. the reference's GENERATOR = 7
 * (scalar.rs:99-105, `MULTIPLICATIVE_GENERATOR` :708):
 *   forward  y[m] = sum_j x[j] g^j w^(jm)            (the values of the polynomial x on the coset g * <w>)
 *   inverse  x[j] = g^-j n^-1 sum_m y[m] w^(-jm)     (so inverse(g) after forward(g) is the identity)
 * w as for blsgpu_fr_ntt.  The shift is fused into the transform's own passes (no separate multiplication pass); its power table is
 * built on the device and cached per (g, log_n, direction).  Inputs and outputs are canonical.  log_n in [0, 28],
 * k * 2^log_n <= 2^28, k == 0 is a no-op.  d_data must be 16-byte aligned (the kernels read 16-byte words).  The device form is
 * asynchronous on the context's stream.  BLSGPU_ERR_ARG (nothing staged or launched): NULL data with k > 0, log_n or k * 2^log_n out
 * of range, a coset whose limbs are all zero or not below r. */
int blsgpu_fr_ntt_many(blsgpu_ctx* ctx, uint64_t* data, int log_n, size_t k, int inverse, const uint64_t* coset);
int blsgpu_fr_ntt_many_device(blsgpu_ctx* ctx, void* d_data, int log_n, size_t k, int inverse, const uint64_t* coset);
/* Recurrences ALONG a vector: k independent rows of `len` scalars each (any len > 0, not only a power of two), laid end to end; row v
 * occupies scalars [v * len, (v+1) * len).  One call scans all rows:
 *   SUM      out[v][i] = sum_{j<=i} in[v][j]            exclusive: the sum over j < i, out[v][0] = 0
 *   PRODUCT  out[v][i] = prod_{j<=i} in[v][j]           exclusive: the product over j < i, out[v][0] = 1 (a zero zeroes the rest of ITS row)
 *   HORNER   out[v][len-1] = in[v][len-1],  out[v][i] = in[v][i] + points[v] * out[v][i+1]      (exclusive must be 0)
 * For HORNER in[v][i] is the coefficient of X^i of p_v, z = points[v] the row's own point (k scalars: data, so a device pointer in the
 * device form): out[v][0] = p_v(z), and out[v][1 .. len) are the coefficients of X^0 .. X^(len-2) of (p_v(X) - p_v(z)) / (X - z), the
 * quotient of a KZG opening.  `points` is ignored for SUM and PRODUCT.  Inputs and outputs are canonical Montgomery limbs.
 * k * len <= 2^28; k == 0 and len == 0 are no-ops.  Device pointers must be 16-byte aligned.  out == in (exactly) is the in-place form;
 * any other overlap is refused.  The device form is asynchronous on the context's stream; its scratch is the context's own (about 10
 * bytes per element for a call of more than 2048 elements) and is not shared with pipelined *_msm_device calls in flight.  BLSGPU_ERR_ARG (nothing staged or launched): an unknown op, exclusive with
 * HORNER, k * len out of range (64-bit overflow included), NULL in / out with work to do, NULL points for HORNER, a misaligned device
 * pointer, a partial overlap. */
#define BLSGPU_FR_SCAN_SUM     0
#define BLSGPU_FR_SCAN_PRODUCT 1
#define BLSGPU_FR_SCAN_HORNER  2
int blsgpu_fr_scan_many(blsgpu_ctx* ctx, int op, int exclusive, const uint64_t* values, size_t len, size_t k, const uint64_t* points, uint64_t* out);
int blsgpu_fr_scan_many_device(blsgpu_ctx* ctx, int op, int exclusive, const void* d_in, size_t len, size_t k, const void* d_points, void* d_out);
/* out[i] = in[i]^-1 for a whole vector by Montgomery's trick (about three products per element and one inversion per tile of 2048,
 * against an exponentiation per element for blsgpu_fr_op op 4, whose results these equal limb for limb).  A zero gives 0 and
 * nonzero_flags[i] = 0 (1 elsewhere; nonzero_flags may be NULL) and affects no other element.  n <= 2^28, n == 0 is a no-op; alignment,
 * out == in, asynchrony and refusals as for blsgpu_fr_scan_many. */
int blsgpu_fr_batch_invert(blsgpu_ctx* ctx, const uint64_t* values, size_t n, uint64_t* out, uint8_t* nonzero_flags);
int blsgpu_fr_batch_invert_device(blsgpu_ctx* ctx, const void* d_in, size_t n, void* d_out, void* d_nonzero_flags);
/* Lagrange coefficients at ARBITRARY nodes, for many subsets in ONE call, and optionally the interpolated value: what turns a threshold
 * committee's partial results into the group's (threshold signatures and decryption, Shamir reconstruction, DKG share derivation, KZG
 * multi-point verifiers).  Everything else polynomial here (fr_ntt*, fr_bary_*) lives on the roots of unity.
 *   offsets  nseg + 1 non-decreasing u32 with offsets[0] = 0 and offsets[nseg] = total: exactly the array of `*_msm_segments`.  Segment s
 *            owns the nodes x_i = nodes[offsets[s] + i], i < t_s = offsets[s + 1] - offsets[s]; t_s <= BLSGPU_FR_LAGRANGE_LEN_MAX,
 *            total <= 2^27, nseg <= 2^27.  The device form takes total by value (it cannot read it back without stalling the stream).
 *   points   nseg scalars, z_s the point of segment s; NULL: every z_s = 0, the recovery of a shared secret.  A DEVICE pointer in the
 *            device form (a challenge computed on the device needs no synchronisation), as for HORNER.
 * All scalars are canonical Montgomery limbs.  With inv0(x) = x^-1 and inv0(0) = 0 (blsgpu_fr_batch_invert's convention) the results
 * are DEFINED by
 *     N_i = prod_{j != i} (z_s - x_j)      D_i = prod_{j != i} (x_i - x_j)      lambda_i = N_i * inv0(D_i)
 *     lambda[offsets[s] + i] = lambda_i           y[s] = sum_i lambda_i * values[offsets[s] + i]
 *     distinct_flags[s] = 1 if every D_i != 0 (the nodes of s are pairwise distinct), else 0
 * and by nothing else: an empty segment writes no lambda, y[s] = 0 and flag 1; one node gives lambda = 1 for every z; z_s on a node x_m
 * gives lambda_m = 1 and 0 elsewhere; a repeated node gives lambda = 0 at exactly the repeated positions and flag 0, the other
 * positions keeping the formula's value (meaningless as an interpolation, but the same from run to run); z_s on a repeated node gives 0
 * everywhere.  Field elements are canonical, so the limbs are the formula's whatever order the device evaluates it in: t_s^2 + O(t_s)
 * products and ONE field inversion per segment.
 * values, lambda, y and distinct_flags may each be NULL; y needs values; at least one of lambda and y must be given when nseg > 0.
 * lambda == NULL with y is a reconstruction without the coefficient traffic.  nseg == 0 is a no-op.
 * The device form is asynchronous on the context's stream and never synchronises; its one launch depends on (nseg, total) alone; its
 * scratch (32 bytes per node, 64 without lambda) is the context's own, not shared with pipelined *_msm_device calls in flight.  Scalar
 * arrays are 16-byte aligned, d_offsets 4-byte, the flags any.
 * BLSGPU_ERR_ARG with nothing staged or launched: a NULL required pointer with work to do, y without values, neither lambda nor y, nseg
 * or total out of range, a misaligned device pointer, an output that overlaps an input or another output (there is no in-place form);
 * in the host form also offsets that do not start at 0, decrease, or hold a segment over the limit.  The device form cannot see the
 * offsets: a segment that decreases, is longer than the limit or ends beyond total is never used as an address, writes NOTHING (no
 * lambda, no y, no flag) and sets a sticky flag, so that the next blsgpu_synchronize returns BLSGPU_ERR_ARG; every other segment is
 * right. */
#define BLSGPU_FR_LAGRANGE_LEN_MAX 4096      /* = BLSGPU_SEG_LEN_MAX: the same offsets array feeds *_msm_segments */
int blsgpu_fr_lagrange_segments(blsgpu_ctx* ctx, const uint64_t* nodes, const uint32_t* offsets, size_t nseg, const uint64_t* points, const uint64_t* values,
                                uint64_t* lambda, uint64_t* y, uint8_t* distinct_flags);
int blsgpu_fr_lagrange_segments_device(blsgpu_ctx* ctx, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total, const void* d_points, const void* d_values,
                                       void* d_lambda, void* d_y, void* d_distinct_flags);
/* Interpolation in the exponent: out_xyz[s] = sum_i lambda_i * P[offsets[s] + i], lambda exactly the coefficients above (so a flagged
 * segment has a defined value too) -- t partial BLS signatures into the group's signature, t decryption shares into the plaintext
 * mask, f(id') H for a new participant.  The shares are `total` affine wire points plus infinity bytes, as
 * `*_from_bytes_batch_device` writes them; share t belongs to node t.  out_xyz: nseg projective points (18 / 36 u64), the input form of
 * `*_batch_normalize`.  An empty segment gives `identity()`; identities among the shares are ordinary terms; the projective
 * representative is unspecified (compare after batch_normalize).  Exact for every curve point; the endomorphism split of the scalar
 * multiplications only under blsgpu_set_assume_subgroup, as for `*_mul_batch`.  The coefficients are Montgomery limbs whatever
 * blsgpu_set_scalar_form says.  The device forms never synchronise: coefficients, products and sums are three stages on the context's
 * stream with scratch of their own (64 + 144 / 288 bytes per share).  d_xy and d_out_xyz are 8-byte aligned; refusals and the sticky
 * flag are those of blsgpu_fr_lagrange_segments (a segment that breaks the offsets contract writes no point), plus NULL shares or
 * output with work to do and an output that overlaps an input. */
int blsgpu_g1_lagrange_combine(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint64_t* nodes, const uint32_t* offsets, size_t nseg,
                               const uint64_t* points, uint64_t* out_xyz, uint8_t* distinct_flags);
int blsgpu_g2_lagrange_combine(blsgpu_ctx* ctx, const uint64_t* xy, const uint8_t* infinity, const uint64_t* nodes, const uint32_t* offsets, size_t nseg,
                               const uint64_t* points, uint64_t* out_xyz, uint8_t* distinct_flags);
int blsgpu_g1_lagrange_combine_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total,
                                      const void* d_points, void* d_out_xyz, void* d_distinct_flags);
int blsgpu_g2_lagrange_combine_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, const void* d_nodes, const void* d_offsets, size_t nseg, size_t total,
                                      const void* d_points, void* d_out_xyz, void* d_distinct_flags);
/* Fraction scans: the accumulator column of a permutation argument (grand product) and of a log-derivative lookup argument (logUp)
 * from their c column sets in ONE call.  Rows as for blsgpu_fr_scan_many: k rows of `len` scalars laid end to end.  A column SET is c
 * tables of k * len scalars each, table j starting j * pitch scalars behind the set's base pointer, pitch >= k * len (the addressing
 * of blsgpu_fr_mle_fold_device); the host forms are packed, pitch = k * len.  challenges = (beta, gamma), two scalars behind ONE
 * pointer: a DEVICE pointer in the device forms (like d_r of the fold: a transcript on the device needs no synchronisation), a host
 * pointer in the host forms.  With inv0(x) = x^-1 and inv0(0) = 0 (blsgpu_fr_batch_invert's convention):
 *   grand_product   n_j[i] = num_a_j[i] + beta * num_b_j[i] + gamma        d_j[i] = den_a_j[i] + beta * den_b_j[i] + gamma
 *                   f[i]   = (prod_j n_j[i]) * inv0(prod_j d_j[i])
 *                   out    = the PRODUCT scan of f along each row, exactly blsgpu_fr_scan_many's (exclusive: out[v][0] = 1)
 *   frac_sum        f[i]   = sum_j mult_j[i] * inv0(gamma + den_a_j[i] + beta * den_b_j[i])
 *                   out    = the SUM scan of f along each row, exactly blsgpu_fr_scan_many's (exclusive: out[v][0] = 0)
 * so z = grand_product(exclusive, w, id, w, sigma) is PLONK's permutation accumulator and frac_sum's last element of a row is the
 * logUp identity's left-hand side (signs belong in mult).  c in [1, 8].  num_b, den_b or both may be NULL: the beta term is dropped.
 * mult may be NULL: every multiplicity is 1.  Input sets may alias each other in any way (num_a == den_a: both sides of the permutation
 * argument read the same wires).  out is k * len scalars; nonzero_flags is k * len bytes or NULL: 0 where SOME denominator factor of
 * element i is zero, 1 elsewhere.  A zero denominator follows the formulas above -- the product's f[i] is 0 and zeroes the rest of ITS
 * row, the sum loses that one term -- so the results equal, limb for limb, the composition blsgpu_fr_op / blsgpu_fr_batch_invert /
 * blsgpu_fr_scan_many in every case; a zero numerator factor is ordinary data.  The arithmetic is `Scalar`'s mul / add / invert
 * (scalar.rs:435-503, :505-580); inputs and outputs are canonical Montgomery limbs, results are identical from run to run.
 * out and nonzero_flags must overlap no input range and not each other: there is no in-place form.  k * len <= 2^28 and
 * (c - 1) * pitch + k * len <= 2^28; k == 0 and len == 0 are no-ops.  Device pointers must be 16-byte aligned (nonzero_flags: any).
 * The device forms are asynchronous on the context's stream and never synchronise; their scratch is the scans' (the context's own,
 * not shared with pipelined *_msm_device calls in flight).  One field inversion per tile of BLSGPU_FR_FRAC_TILE elements whatever c
 * is; a call of at most one tile is one launch.  BLSGPU_ERR_ARG (nothing staged or launched): c out of range, exclusive not 0 or 1, a
 * NULL required pointer (num_a, den_a, challenges, out) with work to do, pitch < k * len, a size out of range (64-bit overflow
 * included), a misaligned device pointer, out or nonzero_flags overlapping an input, the challenges or each other. */
#define BLSGPU_FR_FRAC_MAX_COLS 8
#define BLSGPU_FR_FRAC_TILE     1024   /* 512 for frac_sum with c > 4 */
int blsgpu_fr_grand_product(blsgpu_ctx* ctx, int exclusive, int c, const uint64_t* num_a, const uint64_t* num_b, const uint64_t* den_a, const uint64_t* den_b,
                            const uint64_t* challenges, size_t len, size_t k, uint64_t* out, uint8_t* nonzero_flags);
int blsgpu_fr_grand_product_device(blsgpu_ctx* ctx, int exclusive, int c, const void* d_num_a, const void* d_num_b, const void* d_den_a, const void* d_den_b, size_t pitch,
                                   const void* d_challenges, size_t len, size_t k, void* d_out, void* d_nonzero_flags);
int blsgpu_fr_frac_sum(blsgpu_ctx* ctx, int exclusive, int c, const uint64_t* mult, const uint64_t* den_a, const uint64_t* den_b, const uint64_t* challenges, size_t len, size_t k,
                       uint64_t* out, uint8_t* nonzero_flags);
int blsgpu_fr_frac_sum_device(blsgpu_ctx* ctx, int exclusive, int c, const void* d_mult, const void* d_den_a, const void* d_den_b, size_t pitch, const void* d_challenges, size_t len,
                              size_t k, void* d_out, void* d_nonzero_flags);
/* Polynomials held in EVALUATION form (the Lagrange basis): the value at a point and the quotient of a KZG opening without leaving that
 * form.  k rows of n = 2^log_n scalars laid end to end (the layout of blsgpu_fr_ntt_many); row v holds f_v[i] = p_v(D[i]) for the unique
 * p_v of degree < n, with w the root blsgpu_fr_ntt uses for log_n and
 *   order BLSGPU_FR_ORDER_NATURAL  D[i] = w^i
 *   order BLSGPU_FR_ORDER_BITREV   D[i] = w^bitrev(i, log_n)      (how blob formats store their rows)
 * `points` holds k scalars, z_v the point of row v (data, so a device pointer in the device form, as for HORNER).
 *   eval  y[v] = p_v(z_v)
 *   open  y[v] as above and q[v][i] = q_v(D[i]) for q_v(X) = (p_v(X) - y[v]) / (X - z_v), of degree < n - 1: the scalars of the proof
 *         MSM over a Lagrange SRS, in the order of the input.
 * A point that lies IN the domain (z_v = D[j]) is handled exactly -- y = f[j], and q[j] is the sum the division by zero stands for --
 * and is found and resolved on the device: the launches depend on the shape alone.  At log_n = 0, y = f[0] and q[0] = 0 for every z.
 * Inputs must be canonical Montgomery limbs, outputs are.  One pass over the data per row that fits a tile of 2048 scalars (n <= 2048),
 * one more for the quotient of longer rows; results are limb-identical from run to run.  log_n in [0, 28], k * 2^log_n <= 2^28, k == 0
 * is a no-op.  Device pointers must be 16-byte aligned.  There is no in-place form: for rows longer than a tile d_q is staging while
 * d_evals is still being read.  The device forms are asynchronous on the context's stream and never synchronise; their scratch is the
 * context's own (the forward twiddle table of log_n, shared with the transform, and 112 bytes per tile of a long row) and is not shared
 * with pipelined *_msm_device calls in flight.  BLSGPU_ERR_ARG (nothing staged or launched): a NULL pointer with work to do, log_n,
 * k * 2^log_n (64-bit overflow included) or order out of range, a misaligned device pointer, any overlap of q or y with the evals or
 * points ranges, or of q with y. */
#define BLSGPU_FR_ORDER_NATURAL 0
#define BLSGPU_FR_ORDER_BITREV  1
int blsgpu_fr_bary_eval_many(blsgpu_ctx* ctx, const uint64_t* evals, int log_n, size_t k, const uint64_t* points, int order, uint64_t* y);
int blsgpu_fr_bary_eval_many_device(blsgpu_ctx* ctx, const void* d_evals, int log_n, size_t k, const void* d_points, int order, void* d_y);
int blsgpu_fr_bary_open_many(blsgpu_ctx* ctx, const uint64_t* evals, int log_n, size_t k, const uint64_t* points, int order, uint64_t* y, uint64_t* q);
int blsgpu_fr_bary_open_many_device(blsgpu_ctx* ctx, const void* d_evals, int log_n, size_t k, const void* d_points, int order, void* d_y, void* d_q);
/* Sparse matrix-vector products over Fr: the step a = A z, b = B z, c = C z in front of a Groth16 / Marlin / PLONK-style prover's
 * transforms -- each output a short linear combination of gathered witness entries with fixed per-circuit coefficients.  The matrix is
 * fixed per circuit and reused for every proof, exactly as an SRS is, so it is a resident handle like blsgpu_bases: upload, validate
 * and plan once, multiply many times.  To apply A, B and C in one call, stack their rows into ONE matrix of 3n rows.
 * Format: CSR.  row_ptr has n_rows + 1 entries, row_ptr[0] = 0, non-decreasing; row_ptr[n_rows] IS the number of non-zeros nnz, and
 * col / val hold that many entries (the caller's promise, as every array length is): col[p] < n_cols, val[p] = the four canonical
 * Montgomery limbs of a `Scalar`.  Columns inside a row may come in any order and may repeat (repeats add); rows may be empty.
 * n_rows, n_cols, nnz <= 2^28.  The handle keeps its own device copy: the caller's arrays are free again when the call returns.
 * Validation happens here, once, before a handle exists (the products gather on trust and never re-validate): row_ptr's first entry and
 * order, nnz's range, every col, every val below r -- on the host for the host form, by a kernel for the device form (upload is a setup
 * call and synchronises the context's stream).  A bad matrix is BLSGPU_ERR_ARG, *out stays NULL, and blsgpu_last_error names the first
 * offending row or position.  d_val must be 16-byte aligned.  blsgpu_fr_matrix_free follows the rules of blsgpu_bases_free (it waits for
 * the device; NULL is allowed). */
typedef struct blsgpu_fr_matrix blsgpu_fr_matrix;
int blsgpu_fr_matrix_upload(blsgpu_ctx* ctx, size_t n_rows, size_t n_cols, const uint32_t* row_ptr, const uint32_t* col, const uint64_t* val, blsgpu_fr_matrix** out);
int blsgpu_fr_matrix_from_device(blsgpu_ctx* ctx, size_t n_rows, size_t n_cols, const void* d_row_ptr, const void* d_col, const void* d_val, blsgpu_fr_matrix** out);
size_t blsgpu_fr_matrix_rows(const blsgpu_fr_matrix* m);
size_t blsgpu_fr_matrix_cols(const blsgpu_fr_matrix* m);
size_t blsgpu_fr_matrix_nnz(const blsgpu_fr_matrix* m);
void blsgpu_fr_matrix_free(blsgpu_fr_matrix* m);
/* out[v][i] = sum_{p in [row_ptr[i], row_ptr[i+1])} val[p] * x[v][col[p]]  for k right-hand sides laid end to end: x is k x n_cols and
 * out is k x n_rows scalars (the layout of blsgpu_fr_ntt_many), built on `Scalar`'s mul / add (scalar.rs:452-503, :435-449; the
 * reference crate has no such operation).  x canonical is a precondition; out is canonical, an empty row gives 0, nnz == 0 writes
 * zeros.  The non-zeros, not the rows, are tiled, so a few rows of 10^5 entries among millions of short ones cost nothing extra; the
 * matrix is read once for all k vectors; results are limb-identical from run to run (no atomics).  k * max(n_rows, n_cols) <= 2^28;
 * k == 0 and n_rows == 0 are no-ops.  Device pointers must be 16-byte aligned.  The device form is asynchronous on the context's
 * stream; its scratch (64 bytes per 2048 non-zeros and vector) is its own and is not shared with pipelined *_msm_device calls in
 * flight.  BLSGPU_ERR_ARG (nothing staged or launched): a NULL matrix, NULL x / out with work to do, k * n out of range (64-bit
 * overflow included), a misaligned device pointer, ANY overlap of the out range with the x range (the gather would race). */
int blsgpu_fr_spmv(blsgpu_ctx* ctx, const blsgpu_fr_matrix* m, const uint64_t* x, size_t k, uint64_t* out);
int blsgpu_fr_spmv_device(blsgpu_ctx* ctx, const blsgpu_fr_matrix* m, const void* d_x, size_t k, void* d_out);
/* Multilinear polynomials: a table of 2^m scalars is the values of a multilinear polynomial f on the hypercube, entry i the value at the
 * point whose coordinate x_b is bit b of i -- what a Spartan / HyperPlonk / GKR-style prover holds after blsgpu_fr_spmv_device where a
 * univariate prover would transform.  k tables are addressed as table j at j * pitch scalars behind the base pointer, pitch >= 2^m (the
 * host forms are packed: pitch = 2^m).  With h = 2^(m-1):
 *   fold      out[j][i] = f_j[i] + r * (f_j[i + h] - f_j[i]),  i < h:  f_j with the TOP variable bound, x_(m-1) = r (m - 1 variables left)
 *   eq table  out[i] = prod_{b<m} (bit b of i ? p_b : 1 - p_b),  so that  f(p) = sum_i f[i] * eq(p)[i]
 *   eval      out[j] = f_j(point), point[b] the value of x_b: m folds, the first into the context's scratch; the tables are not written
 * built on `Scalar`'s mul / add / sub (scalar.rs:452-503, :435-449, :414-432; the reference crate has none of these operations).
 * Canonical inputs are a precondition (not validated); outputs are canonical, and limb-identical from run to run (no atomics, no
 * workgroup waits for another one).  fold: m in [1, 28]; d_r is ONE scalar in device memory; d_out == d_in with pitch_out == pitch_in is
 * the in-place form (row j's result lies in the first half of row j's slot), any other overlap of the two footprints
 * (k - 1) * pitch + length is refused; the host form returns packed k x 2^(m-1).  eq table: m in [0, 28], m == 0 writes the Scalar one.
 * eval: m in [0, 28], m == 0 copies.  (k - 1) * pitch + 2^m <= 2^28 (64-bit overflow checked); k == 0 is a no-op.  Device pointers
 * must be 16-byte aligned.  The device forms are asynchronous on the context's stream; scratch is the context's own and is not shared
 * with pipelined *_msm_device calls in flight.  BLSGPU_ERR_ARG (nothing staged or launched): a NULL pointer with work to do, m, k or a
 * pitch out of range, a misaligned device pointer, an overlap. */
int blsgpu_fr_mle_fold(blsgpu_ctx* ctx, const uint64_t* tables, int m, size_t k, const uint64_t r[4], uint64_t* out);
int blsgpu_fr_mle_fold_device(blsgpu_ctx* ctx, const void* d_in, size_t pitch_in, int m, size_t k, const void* d_r, void* d_out, size_t pitch_out);
int blsgpu_fr_eq_table(blsgpu_ctx* ctx, const uint64_t* point, int m, uint64_t* out);
int blsgpu_fr_eq_table_device(blsgpu_ctx* ctx, const void* d_point, int m, void* d_out);
int blsgpu_fr_mle_eval(blsgpu_ctx* ctx, const uint64_t* tables, int m, size_t k, const uint64_t* point, uint64_t* out);
int blsgpu_fr_mle_eval_device(blsgpu_ctx* ctx, const void* d_tables, size_t pitch, int m, size_t k, const void* d_point, void* d_out);
/* One round polynomial of a sumcheck over  P(x) = sum_t coef_t * prod_{e in term t} f_{term_tab[e]}(x)  (Scalar mul / add / sub as above).
 * The term program is a parameter in HOST memory in both forms, as `coset` is: n_terms in [1, 8]; term_ptr holds n_terms + 1 words,
 * term_ptr[0] = 0, strictly increasing, 1 to 6 factors per term; term_tab holds table indices < k (a repeated index is a square); coef
 * holds n_terms x 4 canonical Montgomery limbs (zero allowed); k in [1, 8].  D = the longest term.  For t = 0 .. D
 *   evals[t] = sum_{i<h} sum_t' coef_t' * prod_e ((1 - t) * f_e[i] + t * f_e[i + h])
 * i.e. the values at 0 .. D of the polynomial the prover sends when it binds x_(m-1); a term shorter than D is evaluated as it is.
 * d_r_prev == NULL: the tables as they are, m in [1, 28], nothing is written but d_evals (D + 1 scalars).  d_r_prev != NULL (one scalar
 * in device memory): FIRST every table is folded at *d_r_prev in place, pitch kept (row j's 2^(m-1) results in the first half of its
 * slot, the second half is left as it was), and the evaluations are those of the folded tables of m - 1 variables; m in [2, 28].  This
 * is the form a prover runs in rounds 2 .. m: one pass reads every table once, writes half of it and leaves the next round's
 * polynomial.  Round s = 1 .. m binds x_(m-s); with challenges r_1 .. r_m the tables end at the point p_b = r_(m-b).
 * Asynchronous on the context's stream; pitch, footprint, alignment, canonical inputs, determinism and refusals as above, and
 * BLSGPU_ERR_ARG for k == 0, a bad program, d_evals or d_r_prev inside the tables. */
int blsgpu_fr_sumcheck_round_device(blsgpu_ctx* ctx, void* d_tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab,
                                    const uint64_t* coef, const void* d_r_prev, void* d_evals);
/* A whole sumcheck as a resident handle, like blsgpu_fr_matrix and blsgpu_bases: begin copies the k tables of m in [1, 28] variables into
 * device memory of its own (the rounds consume them; the caller's are free again on return; k * 2^m <= 2^28) and validates the program
 * once.  round and finish are thin host code over blsgpu_fr_sumcheck_round_device and blsgpu_fr_mle_fold_device that also copy the
 * D + 1 evaluations (finish: the k values f_j(point)) back to HOST memory and synchronise the context's stream: an interactive prover
 * derives its next challenge from them.  Order: round(NULL), then round(r_1) .. round(r_(m-1)) while vars_left > 1, then finish(r_m);
 * for m = 1 round(NULL), finish(r_1).  Challenges are four canonical Montgomery limbs in host memory.  Any other order -- a NULL
 * challenge after the first round, a challenge in the first round, round when one variable is left, finish before that, anything after
 * finish -- is BLSGPU_ERR_ARG and leaves the handle as it was.  vars_left counts the unbound variables (m after begin, 0 after finish);
 * degree is D.  blsgpu_fr_sumcheck_free follows the rules of blsgpu_fr_matrix_free (it waits for the device; NULL is allowed). */
typedef struct blsgpu_fr_sumcheck blsgpu_fr_sumcheck;
int blsgpu_fr_sumcheck_begin(blsgpu_ctx* ctx, const uint64_t* tables, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef,
                             blsgpu_fr_sumcheck** out);
int blsgpu_fr_sumcheck_begin_device(blsgpu_ctx* ctx, const void* d_tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab,
                                    const uint64_t* coef, blsgpu_fr_sumcheck** out);
int blsgpu_fr_sumcheck_vars_left(const blsgpu_fr_sumcheck* s);
int blsgpu_fr_sumcheck_degree(const blsgpu_fr_sumcheck* s);
int blsgpu_fr_sumcheck_round(blsgpu_ctx* ctx, blsgpu_fr_sumcheck* s, const uint64_t* r_prev, uint64_t* evals);
int blsgpu_fr_sumcheck_finish(blsgpu_ctx* ctx, blsgpu_fr_sumcheck* s, const uint64_t* r_last, uint64_t* values);
void blsgpu_fr_sumcheck_free(blsgpu_fr_sumcheck* s);
/* Poseidon over Fr: permutations, fixed-length hashes and Merkle trees, the field-native hash a prover commits to tables with and derives
 * challenges from -- with the data where the transforms and sumcheck rounds left it.  An instance is width t, R_F full rounds (even: half
 * before and half after the partial ones), R_P partial rounds, round constants C[r][i] (r < R_F + R_P, i < t) and a t x t matrix M:
 *   for r = 0 .. R_F + R_P - 1:   s[i] += C[r][i];   s[i] = s[i]^5 (a full round: every i; a partial round: i = 0);   s'[i] = sum_j M[i][j] s[j]
 * built on `Scalar`'s mul / add (scalar.rs:452-503, :435-449; the reference crate has no hash over Scalar).  x^5 permutes Fr:
 * gcd(5, r - 1) = 1.  Fr values are unique, so the result is limb-identical to this definition whatever route the kernels take.
 * THE LIBRARY SHIPS NO STANDARD PARAMETER SET: the constants of a published instance come out of the Poseidon paper's Grain LFSR, which
 * cannot be pinned against published vectors here, and unverifiable constants have no place in a bit-exact library.  The caller passes the
 * constants and the matrix of the instance it uses (security is the instance's: the round numbers and M are not judged here).
 * create: the handle is resident like blsgpu_fr_matrix -- parameters validated and planned once, the constant image uploaded once (a setup
 * call: it synchronises).  t in {2, 3, 4, 5, 9, 12}, r_full even in [2, 16], r_partial in [0, 128]; round_constants holds
 * (r_full + r_partial) * t and mds t * t (row-major) scalars as four canonical Montgomery limbs each, in HOST memory.  form AUTO derives
 * the sparse form of the partial rounds (2t + 2 products each instead of 3 + t^2, and (t-1)^2 once) when the lower-right (t-1) x (t-1)
 * block of M is regular and falls back to the dense rounds otherwise; form DENSE asks for the dense rounds; blsgpu_fr_poseidon_form
 * reports DENSE or SPARSE.  Anything else is BLSGPU_ERR_ARG, *out stays NULL and blsgpu_last_error names the argument or the first
 * constant that is not below r.  blsgpu_fr_poseidon_free follows the rules of blsgpu_fr_matrix_free (it waits for the device; NULL is
 * allowed).
 *   permute    n states of t scalars laid end to end; out == states exactly is the in-place form, any other overlap is refused
 *   hash_many  n preimages of t - 1 scalars; the state is (tag, x_1 .. x_(t-1)) and the digest is element 1 after the permutation; out
 *              holds n scalars and must not overlap the inputs.  tag is four canonical Montgomery limbs in HOST memory in both forms (a
 *              parameter, like `coset`): a domain separator, a level or a round number
 *   merkle     arity a = t - 1: k trees of a^height leaves each, tree after tree; a node is the hash_many digest of its a children under
 *              tag.  roots holds k scalars (required).  nodes (may be NULL) holds every inner level, level-major: level 1 (k a^(height-1)
 *              nodes, tree-major) first, level `height` (the k roots) last, k (a^height - 1) / (a - 1) scalars (k * height for a = 1);
 *              with NULL the inner levels live in the context's scratch.  height 0 copies the leaves to roots.  The leaves are never
 *              written; every overlap between leaves, nodes and roots is refused.
 * n * t, k * a^height and the node count are at most 2^28 (64-bit overflow checked); height in [0, 28]; n == 0 and k == 0 are no-ops.
 * Device pointers must be 16-byte aligned.  Canonical inputs are a precondition (not validated); outputs are canonical and limb-identical
 * from run to run (no atomics, no workgroup waits for another one).  One launch per permute / hash_many; merkle is one launch per level
 * (a level of all k trees is a hash_many over the level below).  The device forms are asynchronous
 * on the context's stream and never synchronise; their scratch is the context's own and is not shared with pipelined *_msm_device calls
 * in flight.  BLSGPU_ERR_ARG (nothing staged or launched): a NULL pointer with work to do, a handle of another device, a tag that is not
 * below r, a size out of range, a misaligned device pointer, an overlap. */
typedef struct blsgpu_fr_poseidon blsgpu_fr_poseidon;
#define BLSGPU_FR_POSEIDON_AUTO   0   /* sparse partial rounds when derivable, else dense */
#define BLSGPU_FR_POSEIDON_DENSE  1   /* the textbook partial rounds */
#define BLSGPU_FR_POSEIDON_SPARSE 2   /* reported by blsgpu_fr_poseidon_form only */
int blsgpu_fr_poseidon_create(blsgpu_ctx* ctx, int t, int r_full, int r_partial, const uint64_t* round_constants, const uint64_t* mds, int form, blsgpu_fr_poseidon** out);
int blsgpu_fr_poseidon_width(const blsgpu_fr_poseidon* p);
int blsgpu_fr_poseidon_rounds_full(const blsgpu_fr_poseidon* p);
int blsgpu_fr_poseidon_rounds_partial(const blsgpu_fr_poseidon* p);
int blsgpu_fr_poseidon_form(const blsgpu_fr_poseidon* p);
size_t blsgpu_fr_poseidon_products(const blsgpu_fr_poseidon* p);      /* field products of one permutation in the form the handle uses */
void blsgpu_fr_poseidon_free(blsgpu_fr_poseidon* p);
int blsgpu_fr_poseidon_permute(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const uint64_t* states, size_t n, uint64_t* out);
int blsgpu_fr_poseidon_permute_device(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const void* d_states, size_t n, void* d_out);
int blsgpu_fr_poseidon_hash_many(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const uint64_t* inputs, size_t n, uint64_t* out);
int blsgpu_fr_poseidon_hash_many_device(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const void* d_inputs, size_t n, void* d_out);
int blsgpu_fr_poseidon_merkle(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const uint64_t* leaves, int height, size_t k, uint64_t* nodes, uint64_t* roots);
int blsgpu_fr_poseidon_merkle_device(blsgpu_ctx* ctx, const blsgpu_fr_poseidon* p, const uint64_t tag[4], const void* d_leaves, int height, size_t k, void* d_nodes, void* d_roots);
/* TWISTED EDWARDS GROUPS OVER Fr: the curves  a x^2 + y^2 = 1 + d x^2 y^2  whose coordinates are `Scalar`s -- Jubjub (Pedersen hashes, note
 * commitments, RedJubjub keys) and Bandersnatch (256-wide Pedersen vector commitments) are two of them.  The group law is the unified addition
 *   (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 - a x1 x2) / (1 - d x1 x2 y1 y2)),
 * the identity is (0, 1) and -(x, y) = (-x, y), built on `Scalar`'s mul / add / sub (scalar.rs:452-503, :435-449, :420-432; the reference
 * crate has no such group).  THE LIBRARY SHIPS NO PARAMETER SET: a and d are the caller's, as the constants of a Poseidon instance are.
 * Formats.  An Fr element is four canonical Montgomery u64 limbs, as everywhere in the Fr entry points.  An AFFINE point is (x, y), 8 u64;
 * there is no infinity byte.  A RESULT point is (X : Y : Z), 12 u64, x = X / Z, y = Y / Z: the representative is unspecified, compare after
 * normalize (as for `*_mul_batch`).  A SCALAR is a plain 256-bit little-endian integer of 32 bytes -- NOT an Fr element (the order of such
 * a group is not r): it is never compared with r and does not depend on blsgpu_set_scalar_form.  `bits` in [1, 256] says how many low bits of
 * every scalar are read; a scalar with a bit set at or above `bits` is reported as a scalar >= r is elsewhere (BLSGPU_ERR_ARG from a host
 * form; the sticky status word and the next blsgpu_synchronize for a device form) and the value of that ONE output is unspecified.
 * Completeness.  blsgpu_fr_edwards_complete returns 1 exactly when a is a square and d is a non-square (two Euler-criterion powers on the
 * host).  On such a curve every operation below is exact for EVERY pair of curve points: the points of order 2 and 4, P + P, P + (-P).  On a
 * curve that is NOT complete (Bandersnatch: a = -5 is a non-square) results are exact when every input point has ODD order and are
 * unspecified otherwise -- a promise of the caller's like blsgpu_set_assume_subgroup, not checked.  Points off the curve: unspecified values,
 * never an access outside the arrays.
 *   create        refuses a = 0, d = 0, a = d (a singular curve) and limbs >= r: BLSGPU_ERR_ARG, *out stays NULL, blsgpu_last_error names
 *                 the argument.  The handle holds no device memory; blsgpu_fr_edwards_free follows blsgpu_fr_matrix_free.
 *   check         ok[i] = 1 iff point i has limbs below r and satisfies the curve equation.
 *   normalize     (X : Y : Z) -> (X / Z, Y / Z) with ONE inversion per 256 points; where Z = 0, (0, 1) is written and ok[i] = 0 (ok may be
 *                 NULL).  There is no in-place form (the strides differ): any overlap of xy with xyz is refused.
 *   mul_batch     out[i] = s_i * P_i for n independent pairs in one launch: signed 3-bit windows, 3 (ceil((bits + 1) / 3) - 1) doublings
 *                 whatever the scalars hold, so bits = 64 does a quarter of the work of 256.
 *   bases_create / bases_from_device   a fixed-base table for n bases: for every base B and each of W = ceil((bits + 1) / window) signed
 *                 windows the 2^(window-1) multiples k 2^(window w) B, affine with d x y beside them (96 bytes an entry), built and
 *                 normalised on the device.  window in [2, 8], n in [1, 2^24], and n * W * 2^(window-1) * 96 bytes at most 2 GiB.  A setup
 *                 call: it synchronises.  A base that fails `check` is refused: the host form names it, the device form reads a flag back.
 *                 blsgpu_fr_edwards_bases_free follows blsgpu_fr_matrix_free.  A table keeps its own copy of a and d.
 *   msm_segments  out[j] = sum_{i < len_j} scalars[offsets[j] + i] * B[base_first[j] + i]: the contract of blsgpu_g1_msm_segments (k + 1
 *                 non-decreasing u32 offsets with offsets[0] = 0 and offsets[k] = total, base_first == NULL means base_first[j] =
 *                 offsets[j], overlapping slices -- a shared generator set -- allowed) with segments of ANY length: total <= 2^26, k <= 2^26.
 *                 The scalars are read with the table's `bits`.  No doublings: a term is W table additions.  The term list is cut into
 *                 chunks as blsgpu_g1_sum_segments cuts its own; an empty segment gives (0 : 1 : 1); k = 0 does nothing.  No atomics touch
 *                 a result and no workgroup waits for another: results are limb-identical from run to run after normalize.
 *                 Host form: offsets, base ranges and sizes are checked before anything is staged.  Device form: `total` = offsets[k] as
 *                 the caller knows it; a segment that breaks the rules (offsets[0] != 0, decreasing offsets, offsets[j + 1] > total,
 *                 offsets[k] != total, bases outside the table) is reported by the next blsgpu_synchronize (BLSGPU_ERR_ARG), its value and
 *                 that of its neighbours in the same chunks are unspecified, and nothing outside the caller's arrays is read or written.
 * Limits: n <= 2^26 points per check / normalize / mul_batch call.  Device pointers must be 16-byte aligned (d_offsets / d_base_first: 4).
 * The device forms are asynchronous on the context's stream and never synchronise (the table builds excepted); the MSM's scratch is the
 * context's own.  BLSGPU_ERR_ARG (nothing staged or launched): a NULL pointer with work to do, a handle of another device, bits or window
 * out of range, a size above its limit, a misaligned device pointer, an output that overlaps an input.  What a device form CANNOT refuse:
 * limbs >= r and points off the curve in check's sense (unspecified values), a scalar above `bits` and a broken segment (both reported by
 * the next synchronise). */
typedef struct blsgpu_fr_edwards blsgpu_fr_edwards;
typedef struct blsgpu_fr_edwards_bases blsgpu_fr_edwards_bases;
#define BLSGPU_FR_EDWARDS_MAX_POINTS ((size_t)1 << 26)      /* check / normalize / mul_batch: points of one call */
#define BLSGPU_FR_EDWARDS_MAX_TOTAL  ((size_t)1 << 26)      /* msm_segments: terms, and segments, of one call */
#define BLSGPU_FR_EDWARDS_MAX_BASES  ((size_t)1 << 24)      /* bases of one table */
#define BLSGPU_FR_EDWARDS_TABLE_MAX_BYTES ((size_t)1 << 31) /* bytes of one table */
#define BLSGPU_FR_EDWARDS_WINDOW_MIN 2
#define BLSGPU_FR_EDWARDS_WINDOW_MAX 8
int blsgpu_fr_edwards_create(blsgpu_ctx* ctx, const uint64_t a[4], const uint64_t d[4], blsgpu_fr_edwards** out);
int blsgpu_fr_edwards_complete(const blsgpu_fr_edwards* e);
void blsgpu_fr_edwards_free(blsgpu_fr_edwards* e);
int blsgpu_fr_edwards_check(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const uint64_t* xy, size_t n, uint8_t* ok);
int blsgpu_fr_edwards_check_device(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const void* d_xy, size_t n, void* d_ok);
int blsgpu_fr_edwards_normalize(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const uint64_t* xyz, size_t n, uint64_t* xy, uint8_t* ok);
int blsgpu_fr_edwards_normalize_device(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const void* d_xyz, size_t n, void* d_xy, void* d_ok);
int blsgpu_fr_edwards_mul_batch(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const uint64_t* xy, const uint8_t* scalars, int bits, size_t n, uint64_t* out_xyz);
int blsgpu_fr_edwards_mul_batch_device(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const void* d_xy, const void* d_scalars, int bits, size_t n, void* d_out_xyz);
int blsgpu_fr_edwards_bases_create(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const uint64_t* xy, size_t n, int bits, int window, blsgpu_fr_edwards_bases** out);
int blsgpu_fr_edwards_bases_from_device(blsgpu_ctx* ctx, const blsgpu_fr_edwards* e, const void* d_xy, size_t n, int bits, int window, blsgpu_fr_edwards_bases** out);
size_t blsgpu_fr_edwards_bases_len(const blsgpu_fr_edwards_bases* t);
void blsgpu_fr_edwards_bases_free(blsgpu_fr_edwards_bases* t);
int blsgpu_fr_edwards_msm_segments(blsgpu_ctx* ctx, const blsgpu_fr_edwards_bases* t, const uint32_t* base_first, const uint32_t* offsets, const uint8_t* scalars, size_t k,
                                   uint64_t* out_xyz);
int blsgpu_fr_edwards_msm_segments_device(blsgpu_ctx* ctx, const blsgpu_fr_edwards_bases* t, const void* d_base_first, const void* d_offsets, const void* d_scalars, size_t k,
                                          size_t total, void* d_out_xyz);
/* Fr EXPRESSION PROGRAMS: the row-wise evaluation of a constraint expression -- gates, a permutation term with its next-row operand,
 * boundary terms, all times 1 / Z_H -- over columns resident on the device, in ONE pass: the quotient numerator of a PLONK / halo2-style
 * prover on the extended coset domain between blsgpu_fr_ntt_many (onto the coset) and blsgpu_fr_ntt_many (back).  The expression is a
 * small straight-line program over a register file, fixed per circuit: validated once, when the handle is created, and interpreted per
 * row by one precompiled kernel (there is no runtime compilation).  Every column is read where it is used, every intermediate stays on
 * the chip, only the result of a row is written.
 *   program   n_instr instructions of three words in HOST memory, {op | dst << 8, a, b}: BLSGPU_FR_EXPR_INSTR(op, dst), then two operand
 *             words.  ADD dst = a + b; SUB dst = a - b; MUL dst = a * b; MAD dst = dst + a * b; MOV dst = a (b must be 0).
 *             An operand is BLSGPU_FR_EXPR_REG(i), i < n_regs; BLSGPU_FR_EXPR_COL(j, rot), j < n_cols, rot a signed 16-bit rotation;
 *             or BLSGPU_FR_EXPR_CONST(i), i < n_consts (kind in bits 31..30, index in bits 7..0, rot in bits 23..8, every other bit 0).
 *             The result of a row is the dst of the LAST instruction.
 *   limits    n_cols in [1, 32], n_regs in [1, 8], n_consts in [0, 32] (canonical Montgomery limbs, four u64 each; consts is NULL
 *             exactly when there are none), n_instr in [1, 256].
 *   refused   at create, BLSGPU_ERR_ARG with *out left NULL and blsgpu_last_error naming the instruction index and the rule: an
 *             unknown op or operand kind, an index out of range, a stray bit, a constant not below r, and a register READ -- as an
 *             operand or as MAD's dst -- before any instruction wrote it (results never depend on what a register held before).
 * blsgpu_fr_expr_create uploads the program image (about 4 KB, owned by the handle) and synchronises: a setup call.  The accessors
 * report the handle's shape; _products is the number of MUL + MAD instructions (field products per row), _cols_read has bit j set when
 * some instruction reads column j.  blsgpu_fr_expr_free follows the rules of blsgpu_fr_matrix_free (it waits for the device; NULL is
 * allowed).
 *
 * Evaluation: N = 2^log_n rows, log_n in [0, 28].  cols is a HOST array of n_cols pointers (device pointers in the device form, host
 * pointers in the host form): a parameter like `coset`, the columns come from different allocations.  Column j holds
 * 2^col_log_len[j] scalars, col_log_len[j] <= log_n (col_log_len == NULL: every column has N), and is read MODULO ITS OWN LENGTH:
 *   for row i, COL(j, rot) = col_j[(i + rot * 2^log_stride) mod 2^col_log_len[j]]        (64-bit signed arithmetic; log_stride in [0, log_n])
 * which is three things at once.  Rotations on an extended domain: on N = n * 2^e points the next row of the trace is
 * w_n = w_N^(2^e), so log_stride = e.  Periodic columns: 1 / Z_H on the coset g <w_N> depends on i mod 2^e only -- a column of length
 * 2^e (blsgpu_fr_batch_invert of the 2^e values g^n w_N^(n i) - 1).  Challenges on the device: a column of length 1 is one scalar in
 * device memory (d_challenges of the fraction scans), so a transcript on the device needs no synchronisation.
 * The domain point X is NOT an operand kind: it is a column, the coset transform (blsgpu_fr_ntt_many, forward, coset = g) of the
 * coefficient vector (0, 1, 0, ...).  Likewise L_1: the coset transform of the coefficients (1/n, 1/n, ..., 1/n, 0, ..., 0) (n of them,
 * then zeros up to N), i.e. of the inverse transform of (1, 0, ..., 0) on the trace domain, zero-padded.
 * The arithmetic is `Scalar`'s add / sub / mul (scalar.rs:414-503).  Inputs are canonical Montgomery limbs (a precondition, not
 * validated); outputs are canonical, so they are limb-identical to the same expression composed from blsgpu_fr_op, and identical from
 * run to run.  out is N scalars and must not overlap any column the program reads (checked on the 64-bit ranges: a rotated read would
 * race); columns may alias each other freely; there is no in-place form.  Pointers and lengths of columns no instruction reads are
 * ignored (the pointers may be NULL).  Device pointers must be 16-byte aligned.  The device form is asynchronous on the context's
 * stream, never synchronises and uses no scratch, so it shares nothing with pipelined *_msm_device calls in flight.
 * BLSGPU_ERR_ARG (nothing staged or launched): a NULL context or handle, a handle created on another device, NULL cols / out or a NULL
 * pointer of a column that is read, log_n, log_stride or a read column's col_log_len out of range, a misaligned device pointer, out
 * overlapping a column that is read. */
typedef struct blsgpu_fr_expr blsgpu_fr_expr;
#define BLSGPU_FR_EXPR_ADD 0
#define BLSGPU_FR_EXPR_SUB 1
#define BLSGPU_FR_EXPR_MUL 2
#define BLSGPU_FR_EXPR_MAD 3
#define BLSGPU_FR_EXPR_MOV 4
#define BLSGPU_FR_EXPR_MAX_COLS   32
#define BLSGPU_FR_EXPR_MAX_REGS   8
#define BLSGPU_FR_EXPR_MAX_CONSTS 32
#define BLSGPU_FR_EXPR_MAX_INSTR  256
#define BLSGPU_FR_EXPR_REG(i)       ((uint32_t)(i) & 0xffu)
#define BLSGPU_FR_EXPR_COL(j, rot)  (0x40000000u | (((uint32_t)(rot) & 0xffffu) << 8) | ((uint32_t)(j) & 0xffu))
#define BLSGPU_FR_EXPR_CONST(i)     (0x80000000u | ((uint32_t)(i) & 0xffu))
#define BLSGPU_FR_EXPR_INSTR(op, dst) (((uint32_t)(op) & 0xffu) | (((uint32_t)(dst) & 0xffu) << 8))
int blsgpu_fr_expr_create(blsgpu_ctx* ctx, int n_cols, int n_regs, int n_consts, const uint64_t* consts, size_t n_instr, const uint32_t* code, blsgpu_fr_expr** out);
int blsgpu_fr_expr_cols(const blsgpu_fr_expr* e);
int blsgpu_fr_expr_regs(const blsgpu_fr_expr* e);
size_t blsgpu_fr_expr_instructions(const blsgpu_fr_expr* e);
size_t blsgpu_fr_expr_products(const blsgpu_fr_expr* e);
uint32_t blsgpu_fr_expr_cols_read(const blsgpu_fr_expr* e);
void blsgpu_fr_expr_free(blsgpu_fr_expr* e);
int blsgpu_fr_expr_eval(blsgpu_ctx* ctx, const blsgpu_fr_expr* e, const uint64_t* const* cols, const uint8_t* col_log_len, int log_n, int log_stride, uint64_t* out);
int blsgpu_fr_expr_eval_device(blsgpu_ctx* ctx, const blsgpu_fr_expr* e, const void* const* d_cols, const uint8_t* col_log_len, int log_n, int log_stride, void* d_out);
/* Lookup tables: the multiplicity column of a log-derivative lookup argument (the `mult` of blsgpu_fr_frac_sum) and the table row
 * every looked-up row hit, in ONE call on data that is already in device memory.  A prover commits to the multiplicities before it
 * draws beta and gamma, so this is the first step of the lookup argument and cannot be folded into a challenge-dependent pass.
 * A KEY is a row of c scalars, c in [1, BLSGPU_FR_FRAC_MAX_COLS].  The table t (`rows` keys) and the looked-up rows f (n keys) are
 * column sets addressed exactly as blsgpu_fr_frac_sum's: column j starts j * pitch scalars behind the base pointer, pitch >= rows
 * (>= n for f); the host forms are packed (pitch = rows, pitch = n).
 * CONTRACT: two keys are equal when all 8 c 32-bit words of their limbs are equal.  Inputs are canonical Montgomery limbs, as
 * everywhere in this library, so limb equality is field equality; a non-canonical limb pattern is a different key.
 * blsgpu_fr_lookup_create / _from_device build the handle once per circuit: its own row-major copy of the keys (the caller's buffer may
 * be freed or overwritten once the call returns), an open-addressed index of `slots` = the power of two >= 2 * rows 32-bit words, and
 * `rows` 32-bit counters.  Both are setup calls and synchronise.  The accessors report c, rows, the number of distinct keys and slots.
 * blsgpu_fr_lookup_free follows the rules of blsgpu_fr_matrix_free (it waits for the device; NULL is allowed).
 * A count call writes any of three outputs (each may be NULL):
 *   d_mult     `rows` scalars, canonical Montgomery: m[j] = #{i : f[i] == t[j]} if j is the FIRST row of t with that key, else 0 -- so
 *              sum_j m[j] / (gamma + t[j]) is right for a table with repeated rows.  With negate = 1 the value is r - m[j] (0 stays 0):
 *              the column goes straight into blsgpu_fr_frac_sum's mult.
 *   d_index    n uint32: the first row of t equal to f[i], or BLSGPU_FR_LOOKUP_MISS.
 *   d_missing  one uint64 in device memory: the number of looked-up rows that are in no table row, written by the call on the stream.
 * The host form takes host pointers (mult: rows * 4 uint64; index: n uint32; missing: one uint64) and synchronises.
 * rows in [1, 2^24]; n <= 2^28 and (c - 1) * pitch + n <= 2^28; n == 0 is valid (mult all zero, missing 0).  Counts stay below 2^32.
 * Tables of at most BLSGPU_FR_LOOKUP_LDS_ROWS rows count in per-workgroup on-chip counters; larger ones behind a per-workgroup cache.
 * The device forms are asynchronous on the context's stream and never synchronise.  The counters are the HANDLE's scratch, zeroed at
 * the start of each count call: calls on one handle are ordered by the stream, and a handle serves ONE stream at a time.  Results are
 * identical from run to run (integer sums only).  Device pointers must be 16-byte aligned (d_index: 4, d_missing: 8).
 * BLSGPU_ERR_ARG (nothing staged or launched): c or rows out of range, negate not 0 or 1, a NULL context, handle, t, or f with n > 0,
 * a handle created on another device, pitch < n (pitch < rows when building from device), a size out of range (64-bit overflow
 * included), a misaligned device pointer, an output overlapping f or another output. */
typedef struct blsgpu_fr_lookup blsgpu_fr_lookup;
#define BLSGPU_FR_LOOKUP_LDS_ROWS 4096
#define BLSGPU_FR_LOOKUP_MISS     0xFFFFFFFFu
int blsgpu_fr_lookup_create(blsgpu_ctx* ctx, int c, const uint64_t* t, size_t rows, blsgpu_fr_lookup** out);
int blsgpu_fr_lookup_from_device(blsgpu_ctx* ctx, int c, const void* d_t, size_t pitch, size_t rows, blsgpu_fr_lookup** out);
int blsgpu_fr_lookup_cols(const blsgpu_fr_lookup* h);
size_t blsgpu_fr_lookup_rows(const blsgpu_fr_lookup* h);
size_t blsgpu_fr_lookup_distinct(const blsgpu_fr_lookup* h);
size_t blsgpu_fr_lookup_slots(const blsgpu_fr_lookup* h);
void blsgpu_fr_lookup_free(blsgpu_fr_lookup* h);
int blsgpu_fr_lookup_count(blsgpu_ctx* ctx, const blsgpu_fr_lookup* h, const uint64_t* f, size_t n, int negate, uint64_t* mult, uint32_t* index, uint64_t* missing);
int blsgpu_fr_lookup_count_device(blsgpu_ctx* ctx, const blsgpu_fr_lookup* h, const void* d_f, size_t pitch, size_t n, int negate, void* d_mult, void* d_index, void* d_missing);
/* The same radix-2 transform over GROUP elements: k vectors of 2^log_n G1 (G2) points each, laid end to end, in place, natural order in
 * and out:
 *   forward  Y[m] = sum_j [w^(jm)] P[j],   inverse  P[j] = [n^-1] sum_m [w^(-jm)] Y[m],   w as for blsgpu_fr_ntt
 * so the transform of [s_j] G is [fr_ntt(s)_m] G, and inverse after forward is the identity on group elements.  Uses: a monomial SRS
 * [tau^j] G into its Lagrange form (the inverse transform), the Toeplitz products of amortised KZG openings, key derivation over G2.
 * Points are projective wire points X | Y | Z (18 u64 for G1, 36 for G2; an affine point is one with Z = 1, any record with Z = 0 is
 * the identity): what blsgpu_g{1,2}_mul_batch writes and blsgpu_g{1,2}_batch_normalize reads, so mul_batch_device -> ntt_many_device
 * -> batch_normalize_device -> bases_from_device is a chain without a host copy.  Results are group elements: the projective
 * representative is not pinned, compare after affine conversion (as for mul_batch).
 * PRECONDITION: every point lies in the prime-order subgroup -- outputs of the checked decoders, of mul_batch / MSM on such points, an
 * SRS; the identity is allowed anywhere.  w^(jm) is a residue mod r, so the transform is only defined there, and the endomorphism
 * splits are always used, whatever blsgpu_set_assume_subgroup says.  Results for points outside the subgroup are unspecified (as for
 * the MSM under blsgpu_set_assume_subgroup).
 * log_n in [0, 24], k * 2^log_n <= 2^24; k == 0 and log_n == 0 are no-ops (the records are left exactly as they are: a record with
 * Z = 0 stays the identity it was).  d_xyz must be 16-byte aligned.  The device form is
 * asynchronous on the context's stream and works in place: it shares no scratch with pipelined *_msm_device calls in flight.  The
 * twiddle tables are the Fr transform's, built on the device and cached per (log_n, direction).  BLSGPU_ERR_ARG (nothing staged or
 * launched): NULL points with k > 0, log_n or k * 2^log_n out of range, a misaligned d_xyz.  There is no coset form. */
int blsgpu_g1_ntt_many(blsgpu_ctx* ctx, uint64_t* xyz, int log_n, size_t k, int inverse);
int blsgpu_g2_ntt_many(blsgpu_ctx* ctx, uint64_t* xyz, int log_n, size_t k, int inverse);
int blsgpu_g1_ntt_many_device(blsgpu_ctx* ctx, void* d_xyz, int log_n, size_t k, int inverse);
int blsgpu_g2_ntt_many_device(blsgpu_ctx* ctx, void* d_xyz, int log_n, size_t k, int inverse);
/* Amortised KZG openings: ALL 2c coset openings ("cell proofs") of many polynomials in one call, and the cells themselves -- with
 * n = 4096 and l = 64 the 128 cells and 128 cell proofs of a data-availability blob.  The circulant route (Feist-Khovratovich) turns
 * the 2c quotient MSMs of about n points per polynomial into one segmented MSM of 2n terms and two G1 transforms of 2c points.
 * Notation: n = 2^log_n coefficients, l = 2^log_l points per cell, c = n / l; w the root blsgpu_fr_ntt uses for log_n + 1 (order 2n; w^2
 * is the root for log_n, the domain of blsgpu_fr_bary_*); the SRS is the first n points S[0..n) of a resident G1 base set, S[m] meant as
 * [tau^m] G1.  Cell i of 2c is a coset h_i <w^(2c)> of l points, numbered by `order` (BLSGPU_FR_ORDER_*):
 *   NATURAL  h_i = w^i, entry t of cell i is the point w^(i + 2c t)
 *   BITREV   entry t of cell i is the point w^bitrev(i l + t, log_n + 1): the coset of h_i = w^bitrev(i, log_n + 1 - log_l) walked in
 *            bit-reversed order, the cell numbering of blob formats
 *   cells[v][i][t]  = p_v at that point
 *   proofs[v][i]    = sum_{u < n - l} q_i[u] S[u],  q_i = floor(p_v / (X^l - h_i^l)),  i.e.  q_i[u] = p[u + l] + h_i^l q_i[u + l]
 * The definition is linear in S and holds for ANY subgroup points S[m], not only powers of one tau.  Proofs are group elements: count x 2c
 * projective wire points of 18 u64 (the input form of blsgpu_g1_batch_normalize / _to_bytes_batch), the representative is not pinned,
 * compare after batch_normalize.  A polynomial of degree < l gives 2c identities; c = 1 gives two identities without any MSM.
 *   polys   count x n scalars, canonical Montgomery limbs (a precondition, as for the other Fr calls).  BLSGPU_KZG_FORM_COEFFS: the
 *           coefficients, X^0 first.  BLSGPU_KZG_FORM_EVALS: the n values on <w^2> in `order`, exactly as blsgpu_fr_bary_* reads them.
 *   order   the numbering of the outputs (cells and proofs) and, for FORM_EVALS, of the input.
 *   cells   count x 2c x l scalars.
 * blsgpu_kzg_multiproof_create is a setup call, as blsgpu_fr_matrix_upload is, and synchronises: it builds the transforms of the reversed
 * SRS strides (2n points: a gather, blsgpu_g1_ntt_many of l vectors of 2c, batch_normalize) as a resident base set of its own with its
 * endomorphism images, and keeps no reference to srs_g1.  _log_n / _log_l / _cells (= 2c) report the handle's shape;
 * blsgpu_kzg_multiproof_free follows the rules of blsgpu_fr_matrix_free (it waits for the device; NULL is allowed).
 * Limits: log_n in [0, 23], log_l in [0, min(log_n, 12)] (l <= BLSGPU_SEG_LEN_MAX), count * 2n <= 2^27 (the total of msm_segments),
 * count * 2c <= 2^24 (the group transform's limit); for blsgpu_kzg_cells* alone log_n in [0, 27] and count * 2n <= 2^28.  count == 0 is a
 * no-op.  Device pointers must be 16-byte aligned.  There is no in-place form: any overlap of an output with an input is refused.
 * The device forms are asynchronous on the context's stream and never synchronise; their launches depend on the shape alone; their
 * scratch (about 2 x 64 n + 288 c bytes per polynomial) is the context's own and is not shared with pipelined *_msm_device calls in
 * flight.  The caller's polynomials are never written.  The internal MSM reads Montgomery limbs whatever blsgpu_set_scalar_form says
 * (as the Lagrange combines do) and uses the endomorphism split: the handle's points are in the subgroup by construction.
 * BLSGPU_ERR_ARG with nothing staged or launched: a NULL pointer with work to do; a G2 or too-short SRS (blsgpu_bases_len < n); an SRS
 * whose subgroup state is 0 (a point outside the subgroup); log_n, log_l, count, form or order out of range, 64-bit overflow of the
 * products included; a misaligned device pointer; an overlap.
 * Calls of their own: verification of cells (blsgpu_kzg_verify_cells below) and recovery from half the cells (blsgpu_kzg_recover below).
 * Not in scope: G2, a Lagrange-form SRS, window-table precomputation for the Toeplitz MSM. */
typedef struct blsgpu_kzg_multiproof blsgpu_kzg_multiproof;
#define BLSGPU_KZG_FORM_COEFFS 0   /* n coefficients, X^0 first */
#define BLSGPU_KZG_FORM_EVALS  1   /* n values on <w^2> in `order` (BLSGPU_FR_ORDER_*), as fr_bary_* reads them */
int blsgpu_kzg_multiproof_create(blsgpu_ctx* ctx, const blsgpu_bases* srs_g1, int log_n, int log_l, blsgpu_kzg_multiproof** out);
int blsgpu_kzg_multiproof_log_n(const blsgpu_kzg_multiproof* h);
int blsgpu_kzg_multiproof_log_l(const blsgpu_kzg_multiproof* h);
size_t blsgpu_kzg_multiproof_cells(const blsgpu_kzg_multiproof* h);
void blsgpu_kzg_multiproof_free(blsgpu_kzg_multiproof* h);
int blsgpu_kzg_multiproof_proofs(blsgpu_ctx* ctx, const blsgpu_kzg_multiproof* h, const uint64_t* polys, size_t count, int form, int order, uint64_t* out_xyz);
int blsgpu_kzg_multiproof_proofs_device(blsgpu_ctx* ctx, const blsgpu_kzg_multiproof* h, const void* d_polys, size_t count, int form, int order, void* d_out_xyz);
int blsgpu_kzg_cells(blsgpu_ctx* ctx, const uint64_t* polys, int log_n, int log_l, size_t count, int form, int order, uint64_t* cells);
int blsgpu_kzg_cells_device(blsgpu_ctx* ctx, const void* d_polys, int log_n, int log_l, size_t count, int form, int order, void* d_cells);
/* Batched verification of KZG cell proofs: many (commitment, cell index, cell, proof) tuples decided by ONE two-term pairing product per
 * batch -- the consumer's half of data-availability sampling, blsgpu_kzg_multiproof_proofs / blsgpu_kzg_cells being the producer's.
 * Notation is that of the comment above: n = 2^log_n, l = 2^log_l, c = n / l, w the root blsgpu_fr_ntt uses for log_n + 1; cell j < 2c is
 * the coset h_j <w^(2c)>, numbered by `order` (BLSGPU_FR_ORDER_*) exactly as blsgpu_kzg_cells writes it; S[u] are the first l points of a
 * resident G1 base set, meant as [tau^u] G1.
 * blsgpu_kzg_cell_verifier_create(ctx, srs_g1, log_n, log_l, q_xy, q_inf, &out): q is ONE affine G2 wire point (24 u64, a HOST pointer;
 * q_inf NULL or one infinity byte), meant as [tau^l] G2; the caller vouches that it is in the subgroup, as for the key sets of
 * blsgpu_bls_fast_aggregate_verify_batch.  A setup call that synchronises, like blsgpu_kzg_multiproof_create: the handle keeps no
 * reference to srs_g1; it holds S[0..l) as a resident base set of its own with its endomorphism images, a two-entry `G2Prepared` table
 * {q, -G2 generator} and log_n + 1 powers of w.  _log_n / _log_l / _cells (= 2c) and _free follow the rules of the multiproof handle.
 * Refused (BLSGPU_ERR_ARG): a NULL argument; a G2 SRS or one shorter than l; an SRS with subgroup state 0; another device; log_n outside
 * [0, 23]; log_l outside [0, min(log_n, 12)].
 * blsgpu_kzg_verify_cells takes host pointers; blsgpu_kzg_verify_cells_device takes device pointers, is asynchronous on the context's
 * stream and never synchronises.
 *   commit_xy, commit_inf, ncommit   decoded affine G1 wire points + infinity bytes, as *_from_bytes_batch_device writes them
 *   row, col      m u32 each: cell k belongs to commitment row[k] and is cell number col[k] < 2c
 *   cells         m x l scalars, canonical Montgomery limbs, entry t of cell k as blsgpu_kzg_cells numbers it in `order`
 *   proof_xy, proof_inf              m decoded affine G1 wire points
 *   offsets, nseg [, m]              nseg + 1 u32, the CSR array of *_msm_segments: batch s owns the cells offsets[s] .. offsets[s + 1];
 *                 m = offsets[nseg] is passed by value in the device form
 *   r             nseg scalars (Montgomery limbs; a DEVICE pointer in the device form): the challenge of batch s
 *   verdict       nseg bytes;    out_ab   NULL, or nseg x 2 projective G1 wire points (18 u64 each): A_s, B_s
 * For batch s and its cells k, with rho_k = r_s^(k - offsets[s]) (rho = 1 for the first cell whatever r_s is), a_k = h_col[k]^l and I_k the
 * polynomial of degree < l that takes the values cells[k][*] on the points of cell col[k], the results are DEFINED by
 *   A_s = sum_k rho_k proof_k
 *   B_s = sum_k rho_k commit[row_k] + sum_k rho_k a_k proof_k - sum_{u<l} (sum_k rho_k I_k[u]) S[u]
 *   verdict[s] = 1 if multi_miller_loop([(A_s, q), (B_s, -G2)]).final_exponentiation() == Gt::identity()  (e(A_s, q) == e(B_s, G2)), else 0
 * and by nothing else: for honest inputs over a powers-of-tau SRS every batch holds, and the definition is meaningful for ANY points.
 * An empty batch has verdict 1; identities among commitments and proofs are ordinary terms (a polynomial of degree < l has identity
 * proofs); a pairing term with an identity on either side is skipped, as the reference's multi_miller_loop skips it; c = 1 is legal.
 * out_ab makes the call usable inside a larger pairing product; its projective representative is unspecified (compare after
 * batch_normalize).  (I_k[u] = h^(-u) INTT_l(v)[u], v the cell in natural coset order, INTT_l the inverse blsgpu_fr_ntt of size l.)
 * THE CHALLENGE IS THE CALLER'S, for example from blsgpu_hash_to_scalar_device over a transcript of the batch: soundness needs r_s to be
 * unpredictable from the inputs -- with a known r a wrong cell can be offset by another.  Batches of ONE cell give a per-cell verdict
 * after a failed batch, at the cost of one pairing product per cell.
 * Limits: m <= 2^24, nseg <= 2^24, m * l <= 2^27, nseg * l <= 2^27 (the total of msm_segments).  Device scalar arrays are 16-byte
 * aligned, point arrays 8-byte, u32 arrays 4-byte.  BLSGPU_ERR_ARG with nothing staged or launched: a NULL required pointer with work to
 * do; a range or product overflow, 64-bit wrap included; a bad `order`; a misaligned device pointer; an output that overlaps an input or
 * the other output; a handle of another device.  The host form also refuses offsets that do not start at 0 or that decrease,
 * row[k] >= ncommit and col[k] >= 2c.  The device form cannot see offsets or indices: a bad index or a broken batch (an offset that is
 * not the running maximum of the offsets before it, or beyond m; offsets[0] != 0; offsets[nseg] != m) is never used as an address, its
 * batch gets verdict 0 and an identity pair in out_ab, the context's sticky flag is set (the next blsgpu_synchronize returns
 * BLSGPU_ERR_ARG), and every other batch is right.  nseg == 0 is a no-op.  The caller's arrays are never written.  Scalars are read as
 * Montgomery limbs whatever blsgpu_set_scalar_form says.  The products are exact for every curve point; the endomorphism split of the
 * 3 m scalar multiplications applies only under blsgpu_set_assume_subgroup, as for the Lagrange combines.  The chain -- weights and
 * gather, ONE mul_batch, segment sums, inverse fr_ntt_many of the cells, the fold, msm_segments over S[0..l), batch_normalize,
 * multi_miller_loop_prepared_many with final exponentiation, gt_is_identity -- runs on the context's stream with scratch of its own (about
 * 820 + 32 l bytes per cell), not shared with pipelined *_msm_device calls in flight.
 * Not in scope: byte-level inputs, big-endian scalars, Fiat-Shamir derivation of r, a Pippenger MSM over the fresh proofs (it would need
 * *_bases_from_device and its synchronisation), multi-GPU.  A call of its own: recovery from half the cells (blsgpu_kzg_recover below). */
typedef struct blsgpu_kzg_cell_verifier blsgpu_kzg_cell_verifier;
int blsgpu_kzg_cell_verifier_create(blsgpu_ctx* ctx, const blsgpu_bases* srs_g1, int log_n, int log_l, const uint64_t* q_xy, const uint8_t* q_inf, blsgpu_kzg_cell_verifier** out);
int blsgpu_kzg_cell_verifier_log_n(const blsgpu_kzg_cell_verifier* h);
int blsgpu_kzg_cell_verifier_log_l(const blsgpu_kzg_cell_verifier* h);
size_t blsgpu_kzg_cell_verifier_cells(const blsgpu_kzg_cell_verifier* h);
void blsgpu_kzg_cell_verifier_free(blsgpu_kzg_cell_verifier* h);
int blsgpu_kzg_verify_cells(blsgpu_ctx* ctx, const blsgpu_kzg_cell_verifier* h, const uint64_t* commit_xy, const uint8_t* commit_inf, size_t ncommit, const uint32_t* row,
                            const uint32_t* col, const uint64_t* cells, const uint64_t* proof_xy, const uint8_t* proof_inf, const uint32_t* offsets, size_t nseg, const uint64_t* r,
                            int order, uint8_t* verdict, uint64_t* out_ab);
int blsgpu_kzg_verify_cells_device(blsgpu_ctx* ctx, const blsgpu_kzg_cell_verifier* h, const void* d_commit_xy, const void* d_commit_inf, size_t ncommit, const void* d_row,
                                   const void* d_col, const void* d_cells, const void* d_proof_xy, const void* d_proof_inf, const void* d_offsets, size_t nseg, size_t m,
                                   const void* d_r, int order, void* d_verdict, void* d_out_ab);
/* KZG cell recovery: a polynomial rebuilt from ANY c of its 2c cells, and from it all 2c cells again -- the third operation of
 * data-availability sampling: blsgpu_kzg_verify_cells on what was received -> blsgpu_kzg_recover -> blsgpu_kzg_multiproof_proofs on the
 * recovered coefficients -> serve the full set, all on the device.  Notation is that of the two comments above: n = 2^log_n, l = 2^log_l,
 * c = n / l, w the root blsgpu_fr_ntt uses for log_n + 1; cell i < 2c is the coset h_i <w^(2c)>, numbered by `order` (BLSGPU_FR_ORDER_*)
 * exactly as blsgpu_kzg_cells writes it; g = 7, the reference's GENERATOR.
 *   offsets, count [, m]   count + 1 u32, the CSR array of *_msm_segments: polynomial v owns the received cells offsets[v] .. offsets[v + 1],
 *                 in any order; m = offsets[count] is passed by value in the device form
 *   col           m u32: received cell k is cell number col[k] < 2c in `order`
 *   cells         m x l scalars, canonical Montgomery limbs, entry t of cell k as blsgpu_kzg_cells numbers it in `order`
 *   polys         NULL, or count x n coefficients, X^0 first: BLSGPU_KZG_FORM_COEFFS, ready for blsgpu_kzg_multiproof_proofs_device
 *   out_cells     NULL, or count x 2c x l scalars: ALL cells in `order`, exactly what blsgpu_kzg_cells writes for the recovered polynomial;
 *                 the received cells come back limb-identical when ok[v] = 1.  With ORDER_BITREV the first c cells are the n values of
 *                 the polynomial on <w^2> in bit-reversed order: the blob in evaluation form.  One of polys / out_cells must be given.
 *   ok            count bytes, required.  ok[v] = 1: recovered, and every received cell lies on the polynomial written.  ok[v] = 0: the
 *                 cells are inconsistent (no polynomial of degree < n takes them all), or the polynomial's input is malformed (below);
 *                 its rows of polys / out_cells are then all zero.  Inconsistent data is an ordinary outcome and does NOT set the
 *                 context's sticky flag.  With exactly c cells any values are consistent.
 * For polynomial v with M its missing cells (|M| <= c) and a_i = h_i^l the result is DEFINED by
 *   Z(X) = prod_{i in M} (X^l - a_i);   EZ[j] = the received value at w^j times Z(w^j), 0 at the points of missing cells   (j < 2n)
 *   Q = the 2n coefficients of (P Z) / Z, P Z interpolated from EZ on <w> and divided by Z pointwise on the coset g <w>
 *   ok[v] = Q[n .. 2n) is all zero;   polys[v] = Q[0 .. n)
 * Z(w^j) and Z(g w^j) depend on j mod 2c alone: two tables of 2c scalars per polynomial, built by direct products (O(c^2) per polynomial),
 * the second inverted by ONE batch inversion (it has no zero: g^(2n) != 1).  The chain -- effective offsets, slot table, roots, tables,
 * blsgpu_fr_batch_invert_device, the tiled scatter, inverse blsgpu_fr_ntt_many_device, the forward and the inverse one on the coset g with
 * the scaling between them, the check of the upper half, and blsgpu_kzg_cells_device when out_cells is given -- runs on the context's
 * stream; the device form is asynchronous and never synchronises; its launches depend on (log_n, log_l, count, m) alone (and on whether the root tables of (log_n, log_l) are the ones the context holds); its scratch
 * (about 64 n + 136 c bytes per polynomial, 32 n more without polys, next to that of the calls it chains) is the context's own and is not
 * shared with pipelined *_msm_device calls in flight.  Scalars are Montgomery limbs whatever blsgpu_set_scalar_form says.  The
 * caller's arrays are never written.
 * Limits: log_n in [0, 27], log_l in [0, min(log_n, 12)], log_n - log_l + 1 <= 12 (2c <= 4096), count * 2n <= 2^28, m <= 2^24,
 * m * l <= 2^28.  Scalar arrays are 16-byte aligned, u32 arrays 4-byte.  count == 0 is a no-op.
 * BLSGPU_ERR_ARG with nothing staged or launched: a NULL required pointer; both outputs NULL; a range or product overflow, 64-bit wrap
 * included; a bad `order`; a misaligned device pointer; any overlap of an output with an input or with another output.  The host form
 * also refuses offsets that do not start at 0 or that decrease, col[k] >= 2c, a cell listed twice for one polynomial and fewer than c
 * cells for a polynomial.  The device form cannot see any of that: a polynomial with a bad or duplicate cell number, with fewer than c
 * cells, or with a broken offset (one that is not the running maximum of the offsets before it, or beyond m; offsets[0] != 0;
 * offsets[count] != m -- the rule of blsgpu_kzg_verify_cells_device) gets ok[v] = 0 and zero rows, the context's sticky flag is set (the
 * next blsgpu_synchronize returns BLSGPU_ERR_ARG), every other polynomial is right, and no bad value is ever used as an address.
 * Not in scope: recomputing the proofs inside the call (chain blsgpu_kzg_multiproof_proofs_device on polys), byte-level cells, sharing the
 * tables between polynomials with equal patterns, 2c > 4096. */
int blsgpu_kzg_recover(blsgpu_ctx* ctx, const uint32_t* col, const uint32_t* offsets, size_t count, const uint64_t* cells, int log_n, int log_l, int order, uint64_t* polys,
                       uint64_t* out_cells, uint8_t* ok);
int blsgpu_kzg_recover_device(blsgpu_ctx* ctx, const void* d_col, const void* d_offsets, size_t count, size_t m, const void* d_cells, int log_n, int log_l, int order, void* d_polys,
                              void* d_out_cells, void* d_ok);

/* ---- hash-to-curve (the step in front of multi_miller_loop in bulk signature checks) ---- */
/* `<G as HashToCurve<ExpandMsgXmd<Sha256>>>::hash_to_curve(msg, dst)` / `encode_to_curve` (encode_only != 0) for n
 * messages (src/hash_to_curve/mod.rs:86-108; expand_msg.rs:230-328; map_g1.rs:513-638; map_g2.rs:374-504;
 * g1.rs:800-802, g2.rs:938-947).  `msgs` holds the messages back to back, message i = bytes offsets[i] ..
 * offsets[i+1] (n + 1 offsets).  `dst` of any length (longer than 255 bytes: reduced as expand_msg.rs:74-95 does).
 * out_xyz: n projective points (X : Y : Z), 18 (G1) / 36 (G2) u64 each -- the reference's own coordinates. */
int blsgpu_g1_hash_to_curve_batch(blsgpu_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                  int encode_only, uint64_t* out_xyz);
int blsgpu_g2_hash_to_curve_batch(blsgpu_ctx* ctx, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                  int encode_only, uint64_t* out_xyz);
/* Same with messages, offsets and DST (<= 255 bytes) already in device memory; group = 1 | 2. */
int blsgpu_hash_to_curve_device(blsgpu_ctx* ctx, int group, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len,
                                int encode_only, void* d_out_xyz);
/* The reference's hash-to-curve is generic in the expander: `hash_to_curve::<X>` with X = ExpandMsgXmd<H> for a fixed-output digest H
 * (src/hash_to_curve/expand_msg.rs:230-328) or ExpandMsgXof<H> for an extendable-output function (:167-228); its tests run Sha256, Sha512,
 * Shake128 and Shake256 (tests/expand_msg.rs).  The entry points above are X = ExpandMsgXmd<Sha256>, fused into the hashing kernels (the
 * BLS-signature suites); the `_expander` forms take the choice as an argument, expand into uniform bytes and map from those -- for
 * BLSGPU_EXPAND_XMD_SHA256 with results limb-identical to the fused kernels.  A DST longer than 255 bytes is reduced as
 * expand_msg.rs:47-95 does (XMD: the digest of the salted tag; XOF: its first 32 output bytes) by the host-pointer forms; the
 * device-pointer forms take a DST of at most 255 bytes.  group = 1 | 2. */
#define BLSGPU_EXPAND_XMD_SHA256 0
#define BLSGPU_EXPAND_XMD_SHA512 1
#define BLSGPU_EXPAND_XOF_SHAKE128 2
#define BLSGPU_EXPAND_XOF_SHAKE256 3
int blsgpu_hash_to_curve_expander_batch(blsgpu_ctx* ctx, int group, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst,
                                        size_t dst_len, int encode_only, uint64_t* out_xyz);
int blsgpu_hash_to_curve_expander_device(blsgpu_ctx* ctx, int group, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst,
                                         size_t dst_len, int encode_only, void* d_out_xyz);
/* The part of `hash_to_curve` / `encode_to_curve` BEHIND the expander (hash_to_curve/mod.rs:86-108 after `hash_to_field`'s
 * `expand_message` call): per message count x M x 64 uniform bytes (count = 1 for encode_only, else 2; M = 1 for G1, 2 for G2) are reduced
 * as `from_okm` does (map_g1.rs:512-531, map_g2.rs:362-380), mapped (`map_to_curve`: simplified SWU + isogeny), added and cleared of the
 * cofactor.  For callers with an expander of their own; with the bytes of blsgpu_expand_message_* it gives the limbs of
 * blsgpu_hash_to_curve_expander_*.  uniform = n x count x M x 64 bytes, out_xyz = n projective points in wire limbs -- the reference's own
 * coordinates, except that an identity result (the two field elements of a message negatives of each other) is (0 : Y : 0) with a Y of the
 * formulas' making where the reference's `double` substitutes the literal (0 : 1 : 0) (g1.rs:666, g2.rs:737). */
int blsgpu_hash_to_curve_from_uniform_batch(blsgpu_ctx* ctx, int group, const uint8_t* uniform, size_t n, int encode_only, uint64_t* out_xyz);
int blsgpu_hash_to_curve_from_uniform_device(blsgpu_ctx* ctx, int group, const void* d_uniform, size_t n, int encode_only, void* d_out_xyz);
/* `ExpandMessage::init_expand(msg, dst, len_in_bytes)` followed by reading all `len_in_bytes` bytes, for n messages: out = n x len_in_bytes
 * uniform bytes.  len_in_bytes <= 65535, and at most 255 digest blocks for the XMD expanders (the reference panics beyond, :181-183, :263-268). */
int blsgpu_expand_message_batch(blsgpu_ctx* ctx, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                size_t len_in_bytes, uint8_t* out);
int blsgpu_expand_message_device(blsgpu_ctx* ctx, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len,
                                 size_t len_in_bytes, void* d_out);
/* `hash_to_field::<X, Scalar>` (src/hash_to_curve/mod.rs:32-49 with `HashToField for Scalar`, map_scalar.rs:10-25: 48 uniform bytes per
 * element, zero-extended to 64 and read as `Scalar::from_bytes_wide`): `count` scalars per message, as the reference's `Scalar` (four u64
 * Montgomery limbs): out = n x count x 4 u64 -- ready for blsgpu_g{1,2}_msm_mont* / blsgpu_fr_*. */
int blsgpu_hash_to_scalar_batch(blsgpu_ctx* ctx, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                size_t count, uint64_t* out);
int blsgpu_hash_to_scalar_device(blsgpu_ctx* ctx, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len,
                                 size_t count, void* d_out);


/* ---- the widened rows with inputs and outputs in device memory: a chain that stays on the GPU ---------------- */
/* Device-pointer twins of blsgpu_g{1,2}_batch_normalize, *_from_bytes_batch, *_to_bytes_batch and blsgpu_gt_mul_scalar_batch:
 * same kernels, same formats, asynchronous on the context's stream, nothing crosses PCIe.  With them the stages of bulk
 * verification -- decode + subgroup check (src/g1.rs:273-416, src/g2.rs:330-489), hash-to-curve (map_g2.rs:374-504), normalise
 * (g2.rs:951-984), multi_miller_loop (pairings.rs:554-603), compare with the identity -- hand their results to one another in
 * HBM: blsgpu_hash_to_curve_device writes PROJECTIVE points, *_batch_normalize_device turns them into the AFFINE + infinity
 * form the Miller entry points take.  `d_infinity` of *_batch_normalize_device and `d_ok` / `d_infinity` of *_from_bytes_batch_device
 * are outputs (n bytes each, required). */
int blsgpu_g1_batch_normalize_device(blsgpu_ctx* ctx, const void* d_xyz, size_t n, void* d_xy, void* d_infinity);
int blsgpu_g2_batch_normalize_device(blsgpu_ctx* ctx, const void* d_xyz, size_t n, void* d_xy, void* d_infinity);
int blsgpu_g1_from_bytes_batch_device(blsgpu_ctx* ctx, const void* d_bytes, size_t n, int compressed, int checked, void* d_xy, void* d_infinity, void* d_ok);
int blsgpu_g2_from_bytes_batch_device(blsgpu_ctx* ctx, const void* d_bytes, size_t n, int compressed, int checked, void* d_xy, void* d_infinity, void* d_ok);
int blsgpu_g1_to_bytes_batch_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t n, int compressed, void* d_out);
int blsgpu_g2_to_bytes_batch_device(blsgpu_ctx* ctx, const void* d_xy, const void* d_infinity, size_t n, int compressed, void* d_out);
/* (d_scalars must be 16-byte aligned, as device allocations are: the kernel reads each 32-byte scalar as two 16-byte loads.  A scalar
 * >= r, as bytes or as limbs, is reported by the next blsgpu_synchronize.) */
int blsgpu_gt_mul_scalar_batch_device(blsgpu_ctx* ctx, const void* d_gt, const void* d_scalars, size_t n, void* d_out);
/* d_flags[i] = 1 if gt[i] == Gt::identity() (= Fp12::one(), src/pairings.rs:211-218), else 0: the verdict of an equation
 * prod e(P_j, Q_j) == 1 without bringing 576 B per equation to the host.  (d_gt must be 16-byte aligned, as device allocations are.) */
int blsgpu_gt_is_identity_device(blsgpu_ctx* ctx, const void* d_gt, size_t n, void* d_flags);
/* Bulk BLS signature verification, bytes in -> verdict bytes out, every stage on the device (one upload, one download in the
 * host-pointer form): checked decoding of the compressed public keys and signatures, hash_to_curve of the messages (message i =
 * bytes offsets[i] .. offsets[i+1] of `msgs`; `dst` <= 255 bytes in the device form), normalisation, ONE multi_miller_loop +
 * final exponentiation per signature, comparison with Gt::identity().
 *   mode 0 (public keys in G1, 48 B; signatures in G2, 96 B):  e(pk, H(m)) * e(-G1, sig) == 1   <=>  e(pk, H(m)) == e(G1, sig)
 *   mode 1 (signatures in G1, 48 B; public keys in G2, 96 B):  e(sig, -G2) * e(H(m), pk) == 1   <=>  e(sig, G2) == e(H(m), pk),
 *           with -G2 a `G2Prepared` resident in the context (built at first use).
 * verdict[i]: 1 = the equation holds, 0 = it does not, 2 = the public key is not a valid encoding of a subgroup point
 * (`from_compressed` -> None), 3 = the signature is not.  Identity points decode successfully and take part as the reference's
 * `pairing` treats them (an identity on either side contributes Gt::identity()); rejecting an identity public key is the caller's
 * policy (`KeyValidate`).  This is the reference's own operations composed, not a new scheme: src/g1.rs:336-390, src/g2.rs:390-489,
 * src/hash_to_curve/map_g2.rs:374-504 (map_g1.rs:513-638), src/g2.rs:951-984, src/pairings.rs:554-603, :48-176. */
int blsgpu_bls_verify_batch(blsgpu_ctx* ctx, int mode, const uint8_t* pk_bytes, const uint8_t* sig_bytes, const uint8_t* msgs, const uint64_t* offsets, size_t n,
                            const uint8_t* dst, size_t dst_len, uint8_t* verdict);
int blsgpu_bls_verify_batch_device(blsgpu_ctx* ctx, int mode, const void* d_pk_bytes, const void* d_sig_bytes, const void* d_msgs, const void* d_offsets, size_t n,
                                   const void* d_dst, size_t dst_len, void* d_verdict);
/* Aggregate verification: signature i is ONE signature over ONE message by a SUBSET of a long-lived key set (the shape of
 * FastAggregateVerify: consensus attestations, threshold committees).  Equation i is that of blsgpu_bls_verify_batch with
 * apk_i = sum of the keys idx[t], t in [key_offsets[i], key_offsets[i + 1]), in place of pk_i:
 *   mode 0:  e(apk_i, H(m_i)) == e(G1, sig_i)          mode 1:  e(sig_i, G2) == e(H(m_i), apk_i)
 * The keys are DECODED affine points resident in device memory (d_keys_xy, d_keys_infinity: nkeys points of G1 in mode 0, of G2 in
 * mode 1, as blsgpu_g{1,2}_from_bytes_batch_device writes them): the caller decodes and subgroup-checks a registry ONCE with
 * checked = 1, keeps it, and vouches for it -- nothing about a key is re-checked per call.  idx / key_offsets / total_keys are those of
 * blsgpu_g{1,2}_sum_segments (`impl Sum`, src/g1.rs:161-171), with the same refusals and, in the device form, the same sticky flag for an
 * index outside the set (the key arrays, d_idx and d_key_offsets are aligned as there; d_verdict is n bytes at any address); signatures,
 * messages, dst and the rest of the chain are those of blsgpu_bls_verify_batch (the two share every
 * stage behind the decoding).  In the host form the key set STAYS a pair of device pointers; every other argument is a host pointer.
 * verdict[i]: 1 = the equation holds, 0 = it does not, 3 = the signature is not a valid encoding of a subgroup point; 2 is never
 * produced.  An EMPTY subset, or one whose keys sum to the identity, takes part as an identity public key does in
 * blsgpu_bls_verify_batch: its pairing is Gt::identity(), so the equation holds exactly for the identity signature.  Rejecting such an
 * aggregate is the caller's policy (`KeyValidate`), as is proof of possession against rogue keys. */
int blsgpu_bls_fast_aggregate_verify_batch(blsgpu_ctx* ctx, int mode, const void* d_keys_xy, const void* d_keys_infinity, size_t nkeys, const uint32_t* idx,
                                           const uint64_t* key_offsets, size_t total_keys, const uint8_t* sig_bytes, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                                           const uint8_t* dst, size_t dst_len, uint8_t* verdict);
int blsgpu_bls_fast_aggregate_verify_batch_device(blsgpu_ctx* ctx, int mode, const void* d_keys_xy, const void* d_keys_infinity, size_t nkeys, const void* d_idx,
                                                  const void* d_key_offsets, size_t total_keys, const void* d_sig_bytes, const void* d_msgs, const void* d_msg_offsets, size_t n,
                                                  const void* d_dst, size_t dst_len, void* d_verdict);

#ifdef __cplusplus
}
#endif
#endif /* BLS12_381_HIP_H */
