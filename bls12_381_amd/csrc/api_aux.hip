// api_aux.hip -- the rows either side of the hot path: hash-to-curve, expanders and hash-to-scalar, point codecs, bulk BLS verification.
#define BLS_TU_NAME "api_aux.hip"
#include "host.h"
#include "h2c.hip.h"
#include "expand_kernels.hip.h"
#include "codec.hip.h"
#include "generators.hip.h"

using namespace bls;

// ---------------------------------------------------------------------------------------------------
// hash-to-curve (h2c.hip.h)
// ---------------------------------------------------------------------------------------------------
// one launch of the batched hash: group 1 = one lane per message, group 2 = one lane pair; batches that leave the chip under-filled take
// the split form (two lane groups per message, h2c.hip.h) -- up to 2^15 messages to G1 (<= 1 024 wavefronts of 64 lanes at one per SIMD),
// up to 2^14 to G2 (4 lanes each: 1 024 wavefronts).  Measured on MI355X, 2^14 32-byte messages: see DESIGN.md 4.8.
// uniform bytes of n messages into c->h2c_uniform (any expander; k_expand_message)
static int expand_launch(blsgpu_ctx* c, int expander, const uint8_t* msgs, const unsigned long long* offs, size_t n, const uint8_t* dst, u32 dlen, u32 len_in_bytes, uint8_t* out) {
  KLAUNCH(k_expand_message, dim3(nblk(n, 64)), dim3(64), 0, c->stream, expander, msgs, offs, n, dst, dlen, len_in_bytes, out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
// uniform bytes -> from_okm -> map_to_curve -> (sum) -> clear_h
static int uniform_launch(blsgpu_ctx* c, int group, const uint8_t* uniform, size_t n, int encode_only, u32* out) {
  if (group == 1) KLAUNCH(k_hash_to_curve_uniform<FpPolicy>, dim3(nblk(n, 64)), dim3(64), 0, c->stream, uniform, n, encode_only ? 1 : 0, out);
  else KLAUNCH(k_hash_to_curve_uniform<Fp2PairPolicy>, dim3(nblk(n * 2, 256)), dim3(256), 0, c->stream, uniform, n, encode_only ? 1 : 0, out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
static int h2c_launch(blsgpu_ctx* c, int group, int expander, const uint8_t* msgs, const unsigned long long* offs, size_t n, const uint8_t* dst, u32 dlen, int encode_only, u32* out) {
  if (expander != EXPAND_XMD_SHA256) {
    // the reference's other expanders (expand_msg.rs:167-328 over SHA-512 / SHAKE128 / SHAKE256): expand, then map from the uniform bytes
    const u32 len = (u32)((encode_only ? 1 : 2) * (group == 1 ? 1 : 2) * 64);
    if (c->h2c_uniform.reserve(n * (size_t)len)) { g_err = "hipMalloc(uniform bytes) failed"; return BLSGPU_ERR_HIP; }
    if (int rc = expand_launch(c, expander, msgs, offs, n, dst, dlen, len, c->h2c_uniform.as<uint8_t>())) return rc;
    return uniform_launch(c, group, c->h2c_uniform.as<uint8_t>(), n, encode_only, out);
  }
  const int forced = c->h2c_split;
  const bool split = !encode_only && (forced >= 0 ? forced == 1 : n <= (group == 1 ? (size_t)1 << 15 : (size_t)1 << 14));
  if (group == 1) {
    if (split) KLAUNCH(k_hash_to_curve_split<FpPolicy>, dim3(nblk(n * 2, 64)), dim3(64), 0, c->stream, msgs, offs, n, dst, dlen, out);
    else KLAUNCH(k_hash_to_curve<FpPolicy>, dim3(nblk(n, 64)), dim3(64), 0, c->stream, msgs, offs, n, dst, dlen, encode_only ? 1 : 0, out);
  } else {
    if (split) KLAUNCH(k_hash_to_curve_split<Fp2PairPolicy>, dim3(nblk(n * 4, 256)), dim3(256), 0, c->stream, msgs, offs, n, dst, dlen, out);
    else KLAUNCH(k_hash_to_curve<Fp2PairPolicy>, dim3(nblk(n * 2, 256)), dim3(256), 0, c->stream, msgs, offs, n, dst, dlen, encode_only ? 1 : 0, out);
  }
  LAUNCHCHK();
  return BLSGPU_OK;
}
// Messages (offsets[0..n] into msgs), offsets and DST of the host forms: the offsets are scanned, then the three are staged into io_a / io_b /
// io_f (a DST longer than 255 bytes reduced to H("H2C-OVERSIZE-DST-" || DST) first, expand_msg.rs:47-95).  The device pointers come back
// through d_msgs / d_offs / d_dst, the length of the staged DST through *dlen.
static int stage_messages(HostCall& h, const char* offsets_msg, const char* msgs_msg, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n,
                          const uint8_t* dst, size_t dst_len, void** d_msgs, void** d_offs, void** d_dst, u32* dlen) {
  if (!scan_offsets(offsets, n)) return bad(offsets_msg);
  const size_t total = (size_t)offsets[n];
  if (total && !msgs) return bad(msgs_msg);
  blsgpu_ctx* c = h.c;
  *dlen = h2c_reduce_dst(expander, dst, dst_len, h.keep);
  *d_msgs = h.in(c->io_a, msgs, total);
  *d_offs = h.in(c->io_b, offsets, (n + 1) * 8);
  *d_dst = h.in(c->io_f, h.keep, *dlen);
  return h.rc;
}
// the arguments of every hash-to-curve form (dst_max: 255 for the device forms, which take a reduced DST; no bound on the host)
static int h2c_check(blsgpu_ctx* c, int group, int expander, const void* offsets, size_t n, const void* dst, size_t dst_len, size_t dst_max, const void* out) {
  if (!c || (n && (!offsets || !out)) || (dst_len && !dst)) return bad("hash_to_curve: NULL argument");
  if (dst_len > dst_max) return bad("hash_to_curve_device: reduce a DST longer than 255 bytes on the host first");
  if (group != 1 && group != 2) return bad("hash_to_curve: group must be 1 or 2");
  if (expander < EXPAND_XMD_SHA256 || expander > EXPAND_XOF_SHAKE256) return bad("hash_to_curve: unknown expander");
  return BLSGPU_OK;
}
// device-resident variant: messages, offsets (n + 1 u64) and the DST (<= 255 bytes) already in device memory
static int h2c_device(blsgpu_ctx* c, int group, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, int encode_only, void* d_out_xyz) {
  if (int rc = h2c_check(c, group, expander, d_offsets, n, d_dst, dst_len, 255, d_out_xyz)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  return h2c_launch(c, group, expander, (const uint8_t*)d_msgs, (const unsigned long long*)d_offsets, n, (const uint8_t*)d_dst, (u32)dst_len, encode_only, (u32*)d_out_xyz);
}
static int h2c_host(blsgpu_ctx* c, int group, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, int encode_only,
                    uint64_t* out) {
  if (int rc = h2c_check(c, group, expander, offsets, n, dst, dst_len, (size_t)-1, out)) return rc;
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void *m, *o, *d; u32 dlen;
  if (int rc = stage_messages(h, "hash_to_curve: offsets must be non-decreasing", "hash_to_curve: NULL argument", expander, msgs, offsets, n, dst, dst_len, &m, &o, &d, &dlen)) return rc;
  void* x = h.out(c->io_out, out, n * 3 * (group == 1 ? 12 : 24) * 4);
  if (h.rc) return h.rc;
  return h.finish(h2c_device(c, group, expander, m, o, n, d, dlen, encode_only, x));
}
extern "C" int blsgpu_g1_hash_to_curve_batch(blsgpu_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                             int encode_only, uint64_t* out_xyz) { CTX_CLAIM(c);
  return h2c_host(c, 1, EXPAND_XMD_SHA256, msgs, offsets, n, dst, dst_len, encode_only, out_xyz);
}
extern "C" int blsgpu_g2_hash_to_curve_batch(blsgpu_ctx* c, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                             int encode_only, uint64_t* out_xyz) { CTX_CLAIM(c);
  return h2c_host(c, 2, EXPAND_XMD_SHA256, msgs, offsets, n, dst, dst_len, encode_only, out_xyz);
}
extern "C" int blsgpu_hash_to_curve_device(blsgpu_ctx* c, int group, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len,
                                           int encode_only, void* d_out_xyz) { CTX_CLAIM(c);
  return h2c_device(c, group, EXPAND_XMD_SHA256, d_msgs, d_offsets, n, d_dst, dst_len, encode_only, d_out_xyz);
}
// ---- the reference's other expanders, uniform bytes, and `HashToField for Scalar` (expand.hip.h) ---------------------------------------
// `G1Projective::hash_to_curve::<X>` / `encode_to_curve::<X>` (hash_to_curve/mod.rs:86-108) for X = ExpandMsgXmd<Sha256 | Sha512> or
// ExpandMsgXof<Shake128 | Shake256> (expand_msg.rs:167-328)
extern "C" int blsgpu_hash_to_curve_expander_batch(blsgpu_ctx* c, int group, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len,
                                                   int encode_only, uint64_t* out_xyz) { CTX_CLAIM(c);
  return h2c_host(c, group, expander, msgs, offsets, n, dst, dst_len, encode_only, out_xyz);
}
extern "C" int blsgpu_hash_to_curve_expander_device(blsgpu_ctx* c, int group, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len,
                                                    int encode_only, void* d_out_xyz) { CTX_CLAIM(c);
  return h2c_device(c, group, expander, d_msgs, d_offsets, n, d_dst, dst_len, encode_only, d_out_xyz);
}
// the part behind the expander: caller-supplied uniform bytes -> from_okm -> map_to_curve -> (sum) -> clear_h
static int from_uniform_check(blsgpu_ctx* c, int group, const void* uniform, size_t n, const void* out) {
  if (!c || (n && (!uniform || !out))) return bad("hash_to_curve_from_uniform: NULL argument");
  if (group != 1 && group != 2) return bad("hash_to_curve: group must be 1 or 2");
  return BLSGPU_OK;
}
extern "C" int blsgpu_hash_to_curve_from_uniform_device(blsgpu_ctx* c, int group, const void* d_uniform, size_t n, int encode_only, void* d_out_xyz) { CTX_CLAIM(c);
  if (int rc = from_uniform_check(c, group, d_uniform, n, d_out_xyz)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  return uniform_launch(c, group, (const uint8_t*)d_uniform, n, encode_only, (u32*)d_out_xyz);
}
extern "C" int blsgpu_hash_to_curve_from_uniform_batch(blsgpu_ctx* c, int group, const uint8_t* uniform, size_t n, int encode_only, uint64_t* out_xyz) { CTX_CLAIM(c);
  if (int rc = from_uniform_check(c, group, uniform, n, out_xyz)) return rc;
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  const size_t per = (size_t)(encode_only ? 1 : 2) * (group == 1 ? 1 : 2) * 64;
  void* u = h.in(c->io_a, uniform, n * per);
  void* o = h.out(c->io_out, out_xyz, n * 3 * (group == 1 ? 12 : 24) * 4);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_hash_to_curve_from_uniform_device(c, group, u, n, encode_only, o));
}
// `ExpandMessage::init_expand` + reading all `len_in_bytes` bytes, per message (out: n x len_in_bytes); dst_max as for h2c_check
static int expand_check(blsgpu_ctx* c, int expander, const void* offsets, size_t n, const void* dst, size_t dst_len, size_t dst_max, size_t len_in_bytes, const void* out) {
  if (!c || (n && (!offsets || !out)) || (dst_len && !dst)) return bad("expand_message: NULL argument");
  if (expander < EXPAND_XMD_SHA256 || expander > EXPAND_XOF_SHAKE256) return bad("expand_message: unknown expander");
  if (dst_len > dst_max) return bad("expand_message_device: reduce a DST longer than 255 bytes on the host first");
  // expand_msg.rs:181-183, :263-268: the reference panics beyond these
  if (len_in_bytes > 65535) return bad("expand_message: len_in_bytes must not exceed 65535");
  if (expander <= EXPAND_XMD_SHA512 && (len_in_bytes + (expander == EXPAND_XMD_SHA256 ? 31 : 63)) / (expander == EXPAND_XMD_SHA256 ? 32 : 64) > 255) return bad("expand_message: more than 255 digest blocks");
  return BLSGPU_OK;
}
extern "C" int blsgpu_expand_message_device(blsgpu_ctx* c, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, size_t len_in_bytes,
                                            void* d_out) { CTX_CLAIM(c);
  if (int rc = expand_check(c, expander, d_offsets, n, d_dst, dst_len, 255, len_in_bytes, d_out)) return rc;
  if (!n || !len_in_bytes) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  return expand_launch(c, expander, (const uint8_t*)d_msgs, (const unsigned long long*)d_offsets, n, (const uint8_t*)d_dst, (u32)dst_len, (u32)len_in_bytes, (uint8_t*)d_out);
}
extern "C" int blsgpu_expand_message_batch(blsgpu_ctx* c, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, size_t len_in_bytes,
                                           uint8_t* out) { CTX_CLAIM(c);
  if (int rc = expand_check(c, expander, offsets, n, dst, dst_len, (size_t)-1, len_in_bytes, out)) return rc;
  if (!n || !len_in_bytes) return BLSGPU_OK;
  HostCall h(c);
  void *m, *o, *d; u32 dlen;
  if (int rc = stage_messages(h, "offsets must be non-decreasing", "NULL messages", expander, msgs, offsets, n, dst, dst_len, &m, &o, &d, &dlen)) return rc;
  void* x = h.out(c->io_out, out, n * len_in_bytes);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_expand_message_device(c, expander, m, o, n, d, dlen, len_in_bytes, x));
}
// `hash_to_field::<X, Scalar>` (mod.rs:32-49 with map_scalar.rs:10-25): `count` scalars per message as Montgomery limbs (out: n x count x 4 u64)
static int hash_to_scalar_check(blsgpu_ctx* c, const void* offsets, size_t n, const void* dst, size_t dst_len, size_t count, const void* out) {
  if (!c || (n && count && (!offsets || !out)) || (dst_len && !dst)) return bad("hash_to_scalar: NULL argument");
  if (count > 65535 / 48) return bad("hash_to_scalar: count * 48 must not exceed 65535 (expand_msg.rs:181-183)");
  return BLSGPU_OK;
}
extern "C" int blsgpu_hash_to_scalar_device(blsgpu_ctx* c, int expander, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst, size_t dst_len, size_t count,
                                            void* d_out) { CTX_CLAIM(c);
  if (int rc = hash_to_scalar_check(c, d_offsets, n, d_dst, dst_len, count, d_out)) return rc;
  if (!n || !count) return BLSGPU_OK;
  if (int rc = expand_check(c, expander, d_offsets, n, d_dst, dst_len, 255, count * 48, d_out)) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (c->h2c_uniform.reserve(n * count * 48)) { g_err = "hipMalloc(uniform bytes) failed"; return BLSGPU_ERR_HIP; }
  if (int rc = expand_launch(c, expander, (const uint8_t*)d_msgs, (const unsigned long long*)d_offsets, n, (const uint8_t*)d_dst, (u32)dst_len, (u32)(count * 48),
                             c->h2c_uniform.as<uint8_t>())) return rc;
  KLAUNCH(k_hash_to_scalar, dim3(nblk(n * count, 256)), dim3(256), 0, c->stream, c->h2c_uniform.as<uint8_t>(), n * count, (u32*)d_out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_hash_to_scalar_batch(blsgpu_ctx* c, int expander, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst, size_t dst_len, size_t count,
                                           uint64_t* out) { CTX_CLAIM(c);
  if (int rc = hash_to_scalar_check(c, offsets, n, dst, dst_len, count, out)) return rc;
  if (!n || !count) return BLSGPU_OK;
  if (int rc = expand_check(c, expander, offsets, n, dst, dst_len, (size_t)-1, count * 48, out)) return rc;
  HostCall h(c);
  void *m, *o, *d; u32 dlen;
  if (int rc = stage_messages(h, "offsets must be non-decreasing", "NULL messages", expander, msgs, offsets, n, dst, dst_len, &m, &o, &d, &dlen)) return rc;
  void* x = h.out(c->io_out, out, n * count * 32);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_hash_to_scalar_device(c, expander, m, o, n, d, dlen, count, x));
}

// ---------------------------------------------------------------------------------------------------
// batched point (de)serialisation + validation  (codec.hip.h)
// ---------------------------------------------------------------------------------------------------
template <class F>
static int point_decode_device(blsgpu_ctx* c, const void* d_bytes, size_t n, int compressed, int checked, void* d_xy, void* d_inf, void* d_ok) {
  if (!c || (n && (!d_bytes || !d_xy || !d_inf || !d_ok))) return bad("decode: NULL argument");
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  KLAUNCH(k_point_decode<F>, dim3(nblk(n, 128)), dim3(128), 0, c->stream, (const uint8_t*)d_bytes, n, (compressed ? 1 : 0) | (checked ? 2 : 0), (u32*)d_xy, (uint8_t*)d_inf,
                     (uint8_t*)d_ok);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int point_encode_device(blsgpu_ctx* c, const void* d_xy, const void* d_inf, size_t n, int compressed, void* d_out) {
  if (!c || (n && (!d_xy || !d_out))) return bad("encode: NULL argument");
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  KLAUNCH(k_point_encode<F>, dim3(nblk(n, 128)), dim3(128), 0, c->stream, (const u32*)d_xy, (const uint8_t*)d_inf, n, compressed, (uint8_t*)d_out);
  LAUNCHCHK();
  return BLSGPU_OK;
}
template <class F>
static int point_decode(blsgpu_ctx* c, const uint8_t* bytes, size_t n, int compressed, int checked, uint64_t* xy, uint8_t* inf, uint8_t* ok) {
  if (!c || (n && (!bytes || !xy || !inf || !ok))) return bad("decode: NULL argument");
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  constexpr int CB = Codec<F>::COORD_BYTES, WW = Wire<F>::WORDS;
  void* b = h.in(c->io_a, bytes, n * (compressed ? CB : 2 * CB));
  void* x = h.out(c->io_out, xy, n * 2 * WW * 4);
  void* i = h.out(c->flags_a, inf, n);
  void* o = h.out(c->flags_b, ok, n);
  if (h.rc) return h.rc;
  return h.finish(point_decode_device<F>(c, b, n, compressed, checked, x, i, o));
}
template <class F>
static int point_encode(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, int compressed, uint8_t* out) {
  if (!c || (n && (!xy || !out))) return bad("encode: NULL argument");
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  constexpr int CB = Codec<F>::COORD_BYTES, WW = Wire<F>::WORDS;
  void* x = h.in(c->io_a, xy, n * 2 * WW * 4);
  void* i = h.in(c->flags_a, inf, n);
  void* o = h.out(c->io_out, out, n * (compressed ? CB : 2 * CB));
  if (h.rc) return h.rc;
  return h.finish(point_encode_device<F>(c, x, i, n, compressed, o));
}
extern "C" int blsgpu_g1_from_bytes_batch_device(blsgpu_ctx* c, const void* b, size_t n, int compressed, int checked, void* xy, void* inf, void* ok) { CTX_CLAIM(c);
  return point_decode_device<FpPolicy>(c, b, n, compressed, checked, xy, inf, ok);
}
extern "C" int blsgpu_g2_from_bytes_batch_device(blsgpu_ctx* c, const void* b, size_t n, int compressed, int checked, void* xy, void* inf, void* ok) { CTX_CLAIM(c);
  return point_decode_device<Fp2Policy>(c, b, n, compressed, checked, xy, inf, ok);
}
extern "C" int blsgpu_g1_to_bytes_batch_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t n, int compressed, void* out) { CTX_CLAIM(c);
  return point_encode_device<FpPolicy>(c, xy, inf, n, compressed, out);
}
extern "C" int blsgpu_g2_to_bytes_batch_device(blsgpu_ctx* c, const void* xy, const void* inf, size_t n, int compressed, void* out) { CTX_CLAIM(c);
  return point_encode_device<Fp2Policy>(c, xy, inf, n, compressed, out);
}
extern "C" int blsgpu_g1_from_bytes_batch(blsgpu_ctx* c, const uint8_t* b, size_t n, int compressed, int checked, uint64_t* xy, uint8_t* inf, uint8_t* ok) { CTX_CLAIM(c);
  return point_decode<FpPolicy>(c, b, n, compressed, checked, xy, inf, ok);
}
extern "C" int blsgpu_g2_from_bytes_batch(blsgpu_ctx* c, const uint8_t* b, size_t n, int compressed, int checked, uint64_t* xy, uint8_t* inf, uint8_t* ok) { CTX_CLAIM(c);
  return point_decode<Fp2Policy>(c, b, n, compressed, checked, xy, inf, ok);
}
extern "C" int blsgpu_g1_to_bytes_batch(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, int compressed, uint8_t* out) { CTX_CLAIM(c);
  return point_encode<FpPolicy>(c, xy, inf, n, compressed, out);
}
extern "C" int blsgpu_g2_to_bytes_batch(blsgpu_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, int compressed, uint8_t* out) { CTX_CLAIM(c);
  return point_encode<Fp2Policy>(c, xy, inf, n, compressed, out);
}

// ---------------------------------------------------------------------------------------------------
// bulk BLS signature verification: compressed bytes in -> verdict bytes out, every stage on the device
// ---------------------------------------------------------------------------------------------------
// consts[0..24): the affine wire coordinates of -G1 (g1.rs:86-104 negated, :126-134); consts[24..72): of -G2 (g2.rs:103-140)
__global__ void k_bls_consts(u32* __restrict__ consts) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Aff<FpPolicy> g = generator<FpPolicy>();
  Wire<FpPolicy>::save(g.x, consts); Wire<FpPolicy>::save(neg(g.y), consts + 12);
  const Aff<Fp2Policy> h = generator<Fp2Policy>();
  Wire<Fp2Policy>::save(h.x, consts + 24); Wire<Fp2Policy>::save(neg(h.y), consts + 48);
}
// the two terms of equation i (segment i = terms 2 i, 2 i + 1).  A point whose decoding failed is flagged as the identity so that
// the Miller kernels never see unvalidated limbs; its verdict comes from the ok flags.
//   mode 0:  (pk_i, H_i), (-G1, sig_i)                       mode 1:  (sig_i, table[0] = -G2), (H_i, pk_i)
__global__ void __launch_bounds__(256) k_bls_assemble(int mode, const u32* __restrict__ pk, const uint8_t* __restrict__ pk_inf, const uint8_t* __restrict__ pk_ok,
                                                      const u32* __restrict__ sig, const uint8_t* __restrict__ sig_inf, const uint8_t* __restrict__ sig_ok,
                                                      const u32* __restrict__ h, const uint8_t* __restrict__ h_inf, const u32* __restrict__ consts, size_t n,
                                                      u32* __restrict__ g1t, uint8_t* __restrict__ g1f, u32* __restrict__ g2t, uint8_t* __restrict__ g2f,
                                                      u32* __restrict__ qidx, unsigned long long* __restrict__ off) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  off[i] = 2ull * i;
  if (i == n) return;
  const bool pbad = !pk_ok[i], sbad = !sig_ok[i];
  u32* a0 = g1t + (2 * i) * 24; u32* a1 = a0 + 24;
  u32* b0 = g2t + (2 * i) * 48; u32* b1 = b0 + 48;
  if (mode == 0) {
    for (int k = 0; k < 24; k++) { a0[k] = pk[i * 24 + k]; a1[k] = consts[k]; }
    for (int k = 0; k < 48; k++) { b0[k] = h[i * 48 + k]; b1[k] = sig[i * 48 + k]; }
    g1f[2 * i] = (pk_inf[i] || pbad) ? 1 : 0; g1f[2 * i + 1] = 0;
    g2f[2 * i] = h_inf[i]; g2f[2 * i + 1] = (sig_inf[i] || sbad) ? 1 : 0;
    qidx[2 * i] = PREP_NONE; qidx[2 * i + 1] = PREP_NONE;
  } else {
    for (int k = 0; k < 24; k++) { a0[k] = sig[i * 24 + k]; a1[k] = h[i * 24 + k]; }
    for (int k = 0; k < 48; k++) { b0[k] = 0; b1[k] = pk[i * 48 + k]; }
    g1f[2 * i] = (sig_inf[i] || sbad) ? 1 : 0; g1f[2 * i + 1] = h_inf[i];
    g2f[2 * i] = 0; g2f[2 * i + 1] = (pk_inf[i] || pbad) ? 1 : 0;
    qidx[2 * i] = 0; qidx[2 * i + 1] = PREP_NONE;
  }
}
// n G2 encodings and n G1 encodings in ONE launch (bulk verification: its two decodings are independent, each is one lane per point and fills a
// quarter of the chip at 2^14 points -- one after the other on a stream they cost 3.3 + 1.9 ms, side by side 3.3 ms; a second side STREAM is not
// an answer: the runtime had put two side streams on one hardware queue).  Blocks [0, ceil(n / 128)) decode the G2 array, the rest the G1 array.
__global__ void __launch_bounds__(128) k_point_decode_both(const uint8_t* __restrict__ in2, u32* __restrict__ xy2, uint8_t* __restrict__ inf2, uint8_t* __restrict__ ok2,
                                                           const uint8_t* __restrict__ in1, u32* __restrict__ xy1, uint8_t* __restrict__ inf1, uint8_t* __restrict__ ok1,
                                                           size_t n, int mode) {
  const u32 nb = (u32)((n + blockDim.x - 1) / blockDim.x);
  if (blockIdx.x < nb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) point_decode_one<Fp2Policy>(i, in2, mode, xy2, inf2, ok2);
  } else {
    const size_t i = (size_t)(blockIdx.x - nb) * blockDim.x + threadIdx.x;
    if (i < n) point_decode_one<FpPolicy>(i, in1, mode, xy1, inf1, ok1);
  }
}

__global__ void __launch_bounds__(256) k_bls_verdict(const uint8_t* __restrict__ is_one, const uint8_t* __restrict__ pk_ok, const uint8_t* __restrict__ sig_ok, size_t n,
                                                     uint8_t* __restrict__ verdict) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  verdict[i] = !pk_ok[i] ? 2 : !sig_ok[i] ? 3 : is_one[i] ? 1 : 0;
}
// dst_max as for h2c_check
static int verify_check(blsgpu_ctx* c, int mode, const void* pk, const void* sig, const void* offsets, size_t n, const void* dst, size_t dst_len, size_t dst_max,
                        const void* verdict) {
  if (!c || (n && (!pk || !sig || !offsets || !verdict)) || (dst_len && !dst)) return bad("bls_verify_batch: NULL argument");
  if (mode != 0 && mode != 1) return bad("bls_verify_batch: mode must be 0 (public keys in G1) or 1 (public keys in G2)");
  if (dst_len > dst_max) return bad("bls_verify_batch_device: reduce a DST longer than 255 bytes on the host first");
  return BLSGPU_OK;
}
// where every intermediate of the chain lives in c->ver (the aggregate form appends the summed keys: the plain form's block is unchanged)
struct VerifyLayout { size_t consts, a, b, hp, h, fl, g1t, g2t, tf, qi, off, gt, apk, bytes; };
static VerifyLayout verify_layout(int mode, size_t n, bool aggregate) {
  // G1-side and G2-side points of the equation: mode 0 = (pk, sig), mode 1 = (sig, pk); the hash goes to the signature's group
  const size_t a_xy = n * 96, b_xy = n * 192, h_xyz = n * (mode == 0 ? 288 : 144), h_xy = n * (mode == 0 ? 192 : 96);
  const size_t al = 256;
  auto up = [&](size_t x) { return (x + al - 1) / al * al; };
  VerifyLayout L;
  size_t o = 0;
  L.consts = o; o += up(288);
  L.a = o; o += up(a_xy);
  L.b = o; o += up(b_xy);
  L.hp = o; o += up(h_xyz);
  L.h = o; o += up(h_xy);
  L.fl = o; o += up(6 * n);                // a_inf a_ok b_inf b_ok h_inf is_one
  L.g1t = o; o += up(2 * n * 96);
  L.g2t = o; o += up(2 * n * 192);
  L.tf = o; o += up(4 * n);                // g1f (2n) g2f (2n)
  L.qi = o; o += up(2 * n * 4);
  L.off = o; o += up((n + 1) * 8);
  L.gt = o; o += up(n * 576);
  L.apk = o; if (aggregate) o += up(n * (mode == 0 ? 144 : 288));       // the n summed keys, projective
  L.bytes = o;
  return L;
}
// What both verifiers do before their keys and signatures are decoded: the scratch block, the constants, the resident -G2, and the
// hash of the messages queued on the side stream.  Returns with c->stream the caller's stream again.
static int verify_begin(blsgpu_ctx* c, int mode, size_t n, const VerifyLayout& L, const void* d_msgs, const void* d_offsets, const void* d_dst, size_t dst_len) {
  const bool fresh = c->ver.cap < L.bytes;
  if (c->ver.reserve(L.bytes)) { g_err = "hipMalloc(bulk verification) failed"; return BLSGPU_ERR_HIP; }
  uint8_t* base = c->ver.as<uint8_t>();
  if (fresh || !c->ver_consts_ready) {
    KLAUNCH(k_bls_consts, dim3(1), dim3(64), 0, c->stream, (u32*)(base + L.consts));
    LAUNCHCHK();
    HIPCHK(hipEventRecord(c->ev_ver, c->stream));
    c->ver_consts_ready = true;
  }
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ver, 0));
  if (mode == 1 && !c->ver_table) {
    // `G2Prepared::from(-G2Affine::generator())`, once per context (its own allocation: it outlives a regrown scratch block)
    int rc = blsgpu_g2_prepare_device(c, base + L.consts + 96, nullptr, 1, &c->ver_table);
    if (rc) return rc;
  }
  uint8_t* h_inf = base + L.fl + 4 * n;
  // 1.-3. independent, latency-shaped stages (one lane or lane pair per point, a few thousand field multiplications each): the two
  // checked decodings run on the context's stream, hash-to-curve + normalisation beside them on a side stream (ONE side stream: the
  // runtime multiplexes streams onto a few hardware queues, and two side streams created back to back shared one -- kernel trace of
  // round 5 -- which serialised exactly the two longest stages), and they meet again before the terms are assembled
  if (!c->ver_stream[0]) {
    for (auto& q : c->ver_stream) HIPCHK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    for (auto& e : c->ev_ver_side) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  hipStream_t main_stream = c->stream;
  HIPCHK(hipEventRecord(c->ev_ver_side[0], main_stream));
  int rc = BLSGPU_OK;
  {
    // hash the messages to the signature's group and normalise, on the side stream
    c->stream = c->ver_stream[0];
    hipError_t e = hipStreamWaitEvent(c->stream, c->ev_ver_side[0], 0);
    // (the plain form of the hash even for a small batch: the split form buys latency with 45 % more lane-time, which only pays while the chip
    // has nothing else to do -- here the decoders run beside it; measured 2^14 signatures: 15.5 ms plain, 18.7-18.9 ms split (16.6 / 21.7 ms with the
    // slower G2 decoder of before); BLSGPU_VERIFY_H2C_SPLIT=1 lets the batch-size rule apply here too, for re-measuring)
    const int keep_split = c->h2c_split;
    c->h2c_split = c->diag.verify_h2c_split ? keep_split : 0;
    if (e == hipSuccess) rc = blsgpu_hash_to_curve_device(c, mode == 0 ? 2 : 1, d_msgs, d_offsets, n, d_dst, dst_len, 0, base + L.hp);
    c->h2c_split = keep_split;
    if (e == hipSuccess && !rc)
      rc = mode == 0 ? blsgpu_g2_batch_normalize_device(c, base + L.hp, n, base + L.h, h_inf) : blsgpu_g1_batch_normalize_device(c, base + L.hp, n, base + L.h, h_inf);
    if (e == hipSuccess && !rc) e = hipEventRecord(c->ev_ver_side[1], c->stream);
    c->stream = main_stream;
    if (e != hipSuccess) return fail("bls_verify_batch: side stream", e, __LINE__);
    if (rc) return rc;
  }
  return BLSGPU_OK;
}
// What both verifiers do once their keys and signatures are decoded (xy, infinity and ok flags of both in the block): wait for the hashes,
// assemble the terms, one multi_miller_loop + final exponentiation per equation, the verdicts.
static int verify_finish(blsgpu_ctx* c, int mode, size_t n, const VerifyLayout& L, void* d_verdict) {
  uint8_t* base = c->ver.as<uint8_t>();
  uint8_t* fl = base + L.fl;
  uint8_t *a_inf = fl, *a_ok = fl + n, *b_inf = fl + 2 * n, *b_ok = fl + 3 * n, *h_inf = fl + 4 * n, *is_one = fl + 5 * n;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ver_side[1], 0));
  // 4. the two terms of every equation
  const uint8_t *pk_inf = mode == 0 ? a_inf : b_inf, *pk_ok = mode == 0 ? a_ok : b_ok, *sig_inf = mode == 0 ? b_inf : a_inf, *sig_ok = mode == 0 ? b_ok : a_ok;
  KLAUNCH(k_bls_assemble, dim3(nblk(n + 1, 256)), dim3(256), 0, c->stream, mode, (const u32*)(base + (mode == 0 ? L.a : L.b)), pk_inf, pk_ok,
                     (const u32*)(base + (mode == 0 ? L.b : L.a)), sig_inf, sig_ok, (const u32*)(base + L.h), h_inf, (const u32*)(base + L.consts), n, (u32*)(base + L.g1t),
                     base + L.tf, (u32*)(base + L.g2t), base + L.tf + 2 * n, (u32*)(base + L.qi), (unsigned long long*)(base + L.off));
  LAUNCHCHK();
  // 5. one multi_miller_loop + final exponentiation per equation
  int rc;
  if (mode == 0)
    rc = blsgpu_multi_miller_loop_many_device(c, base + L.g1t, base + L.tf, base + L.g2t, base + L.tf + 2 * n, base + L.off, n, 2 * n, 2, 1, base + L.gt);
  else
    rc = blsgpu_multi_miller_loop_prepared_many_device(c, base + L.g1t, base + L.tf, base + L.g2t, base + L.tf + 2 * n, base + L.qi, c->ver_table, base + L.off, n, 2 * n, 2, 1,
                                                       base + L.gt);
  if (rc) return rc;
  // 6. == Gt::identity()?
  rc = blsgpu_gt_is_identity_device(c, base + L.gt, n, is_one);
  if (rc) return rc;
  KLAUNCH(k_bls_verdict, dim3(nblk(n, 256)), dim3(256), 0, c->stream, is_one, pk_ok, sig_ok, n, (uint8_t*)d_verdict);
  LAUNCHCHK();
  return BLSGPU_OK;
}
extern "C" int blsgpu_bls_verify_batch_device(blsgpu_ctx* c, int mode, const void* d_pk, const void* d_sig, const void* d_msgs, const void* d_offsets, size_t n, const void* d_dst,
                                              size_t dst_len, void* d_verdict) { CTX_CLAIM(c);
  if (int rc = verify_check(c, mode, d_pk, d_sig, d_offsets, n, d_dst, dst_len, 255, d_verdict)) return rc;
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const VerifyLayout L = verify_layout(mode, n, false);
  if (int rc = verify_begin(c, mode, n, L, d_msgs, d_offsets, d_dst, dst_len)) return rc;
  uint8_t* base = c->ver.as<uint8_t>();
  uint8_t* fl = base + L.fl;
  uint8_t *a_inf = fl, *a_ok = fl + n, *b_inf = fl + 2 * n, *b_ok = fl + 3 * n;
  // checked decoding (`from_compressed`: on the curve, in the subgroup) of both point arrays on the context's stream, which then waits for the side stream
  // (ONE launch for both arrays: k_point_decode_both)
  KLAUNCH(k_point_decode_both, dim3(2 * nblk(n, 128)), dim3(128), 0, c->stream, (const uint8_t*)(mode == 0 ? d_sig : d_pk), (u32*)(base + L.b), b_inf, b_ok,
                     (const uint8_t*)(mode == 0 ? d_pk : d_sig), (u32*)(base + L.a), a_inf, a_ok, n, 3);
  LAUNCHCHK();
  return verify_finish(c, mode, n, L, d_verdict);
}
// Aggregate verification (blsgpu_bls_fast_aggregate_verify_batch): equation i takes the SUM of the keys of subset i where the plain form decodes one key.
// The keys are decoded affine points the caller vouches for, so only the signatures are decoded here: on the second side stream, beside
// the segmented sum on the context's stream (neither uses scratch of the other, nor of the hash).  The normalisation of the n sums shares
// io_c / io_d with the normalisation of the hashes: it is queued behind the side stream's event.
static int aggregate_check(blsgpu_ctx* c, int mode, const void* sig, const void* msg_offsets, size_t n, const void* dst, size_t dst_len, size_t dst_max, const void* verdict) {
  if (!c || (n && (!sig || !msg_offsets || !verdict)) || (dst_len && !dst)) return bad("bls_fast_aggregate_verify_batch: NULL argument");
  if (mode != 0 && mode != 1) return bad("bls_fast_aggregate_verify_batch: mode must be 0 (public keys in G1) or 1 (public keys in G2)");
  if (dst_len > dst_max) return bad("bls_fast_aggregate_verify_batch_device: reduce a DST longer than 255 bytes on the host first");
  return BLSGPU_OK;
}
extern "C" int blsgpu_bls_fast_aggregate_verify_batch_device(blsgpu_ctx* c, int mode, const void* d_keys_xy, const void* d_keys_inf, size_t nkeys, const void* d_idx,
                                                             const void* d_key_offsets, size_t total_keys, const void* d_sig, const void* d_msgs, const void* d_msg_offsets, size_t n,
                                                             const void* d_dst, size_t dst_len, void* d_verdict) { CTX_CLAIM(c);
  if (int rc = aggregate_check(c, mode, d_sig, d_msg_offsets, n, d_dst, dst_len, 255, d_verdict)) return rc;
  {
    GsumArgs a;
    a.group = mode == 0 ? 1 : 2; a.xy = d_keys_xy; a.inf = d_keys_inf; a.npoints = nkeys; a.idx = d_idx; a.offsets = d_key_offsets; a.nseg = n; a.total = total_keys;
    // (the sums go to the context's block, which is aligned: `out` is a stand-in here.  d_verdict is n bytes with no alignment rule, as in
    // blsgpu_bls_verify_batch_device; aggregate_check has seen that it is not NULL.)
    alignas(16) static const unsigned char aligned_stand_in[16] = {};
    a.out = aligned_stand_in; a.device = true;
    if (const char* why = gsum_check(a)) return bad(why);     // before anything is queued: the sum itself would refuse too late
  }
  if (!n) return BLSGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  const VerifyLayout L = verify_layout(mode, n, true);
  if (int rc = verify_begin(c, mode, n, L, d_msgs, d_msg_offsets, d_dst, dst_len)) return rc;
  uint8_t* base = c->ver.as<uint8_t>();
  uint8_t* fl = base + L.fl;
  uint8_t *a_inf = fl, *a_ok = fl + n, *b_inf = fl + 2 * n, *b_ok = fl + 3 * n;
  uint8_t *pk_inf = mode == 0 ? a_inf : b_inf, *pk_ok = mode == 0 ? a_ok : b_ok, *sig_inf = mode == 0 ? b_inf : a_inf, *sig_ok = mode == 0 ? b_ok : a_ok;
  void* pk_xy = base + (mode == 0 ? L.a : L.b);
  void* sig_xy = base + (mode == 0 ? L.b : L.a);
  hipStream_t main_stream = c->stream;
  int rc;
  {
    // the signatures: `from_compressed` on the second side stream
    c->stream = c->ver_stream[1];
    hipError_t e = hipStreamWaitEvent(c->stream, c->ev_ver_side[0], 0);
    rc = BLSGPU_OK;
    if (e == hipSuccess) rc = mode == 0 ? point_decode_device<Fp2Policy>(c, d_sig, n, 1, 1, sig_xy, sig_inf, sig_ok) : point_decode_device<FpPolicy>(c, d_sig, n, 1, 1, sig_xy, sig_inf, sig_ok);
    if (e == hipSuccess && !rc) e = hipEventRecord(c->ev_ver_side[2], c->stream);
    c->stream = main_stream;
    if (e != hipSuccess) return fail("bls_fast_aggregate_verify_batch: side stream", e, __LINE__);
    if (rc) return rc;
  }
  // the aggregate keys: segmented sum, then (behind the hashes' normalisation) theirs; a summed key is always a valid key
  rc = mode == 0 ? blsgpu_g1_sum_segments_device(c, d_keys_xy, d_keys_inf, nkeys, d_idx, d_key_offsets, n, total_keys, base + L.apk)
                 : blsgpu_g2_sum_segments_device(c, d_keys_xy, d_keys_inf, nkeys, d_idx, d_key_offsets, n, total_keys, base + L.apk);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(pk_ok, 1, n, c->stream));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ver_side[1], 0));
  rc = mode == 0 ? blsgpu_g1_batch_normalize_device(c, base + L.apk, n, pk_xy, pk_inf) : blsgpu_g2_batch_normalize_device(c, base + L.apk, n, pk_xy, pk_inf);
  if (rc) return rc;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_ver_side[2], 0));
  return verify_finish(c, mode, n, L, d_verdict);
}
// host form: the key set stays where it is -- d_keys_xy / d_keys_inf are DEVICE pointers (a resident registry is the point of the call) --
// and everything that changes from call to call comes from the host
extern "C" int blsgpu_bls_fast_aggregate_verify_batch(blsgpu_ctx* c, int mode, const void* d_keys_xy, const void* d_keys_inf, size_t nkeys, const uint32_t* idx,
                                                      const uint64_t* key_offsets, size_t total_keys, const uint8_t* sig, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                                                      const uint8_t* dst, size_t dst_len, uint8_t* verdict) { CTX_CLAIM(c);
  if (int rc = aggregate_check(c, mode, sig, msg_offsets, n, dst, dst_len, (size_t)-1, verdict)) return rc;
  {
    GsumArgs a;
    a.group = mode == 0 ? 1 : 2; a.xy = d_keys_xy; a.inf = d_keys_inf; a.npoints = nkeys; a.idx = idx; a.offsets = key_offsets; a.nseg = n; a.total = total_keys; a.out = verdict;
    if (const char* why = gsum_check(a)) return bad(why);
    if (const char* why = gsum_check_host(key_offsets, n, total_keys, idx, nkeys)) return bad(why);
  }
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void *m, *o, *d; u32 dlen;
  if (int rc = stage_messages(h, "bls_fast_aggregate_verify_batch: message offsets must be non-decreasing", "bls_fast_aggregate_verify_batch: NULL argument", EXPAND_XMD_SHA256,
                              msgs, msg_offsets, n, dst, dst_len, &m, &o, &d, &dlen)) return rc;
  void* s = h.in(c->flags_b, sig, n * (mode == 0 ? 96 : 48));
  void* ix = total_keys ? h.in(c->io_e, idx, total_keys * 4) : nullptr;
  void* ko = h.in(c->io_out, key_offsets, (n + 1) * 8);
  void* v = h.out(c->flags_a, verdict, n);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_bls_fast_aggregate_verify_batch_device(c, mode, d_keys_xy, d_keys_inf, nkeys, ix, ko, total_keys, s, m, o, n, d, dlen, v));
}
extern "C" int blsgpu_bls_verify_batch(blsgpu_ctx* c, int mode, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offsets, size_t n, const uint8_t* dst,
                                       size_t dst_len, uint8_t* verdict) { CTX_CLAIM(c);
  if (int rc = verify_check(c, mode, pk, sig, offsets, n, dst, dst_len, (size_t)-1, verdict)) return rc;
  if (!n) return BLSGPU_OK;
  HostCall h(c);
  void *m, *o, *d; u32 dlen;
  if (int rc = stage_messages(h, "bls_verify_batch: offsets must be non-decreasing", "bls_verify_batch: NULL argument", EXPAND_XMD_SHA256, msgs, offsets, n, dst, dst_len,
                              &m, &o, &d, &dlen)) return rc;
  void* p = h.in(c->io_e, pk, n * (mode == 0 ? 48 : 96));
  void* s = h.in(c->flags_b, sig, n * (mode == 0 ? 96 : 48));
  void* v = h.out(c->flags_a, verdict, n);
  if (h.rc) return h.rc;
  return h.finish(blsgpu_bls_verify_batch_device(c, mode, p, s, m, o, n, d, dlen, v));
}
