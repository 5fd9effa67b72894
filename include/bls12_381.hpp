// bls12_381.hpp -- header-only C++ mirror of the zkcrypto/bls12_381 hot-path API over libblsgpu.so.
//
// Same names and semantics as the reference's Rust surface (/root/reference/src/lib.rs:49-83): Scalar, G1Affine,
// G1Projective, G2Affine, G2Projective, Gt, MillerLoopResult, G2Prepared, pairing(), multi_miller_loop().  Every
// group / pairing operation is executed by the HIP kernels through the C ABI (bls12_381_hip.h); values are the
// reference's in-memory limbs (canonical Montgomery form, R = 2^384), so they can be memcpy'd to/from a Rust caller.
// Errors from the ABI are thrown as std::runtime_error (the reference's functions are infallible; there is no
// CPU fallback here).
#pragma once
#include <array>
#include <memory>
#include <optional>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <initializer_list>
#include <utility>
#include <vector>

#include "bls12_381_hip.h"

namespace bls {

inline void check(int rc, const char* what) {
  if (rc != BLSGPU_OK) throw std::runtime_error(std::string(what) + ": " + blsgpu_last_error());
}

class Context {
 public:
  explicit Context(int device = 0) { check(blsgpu_create(device, &h_), "blsgpu_create"); }
  ~Context() { blsgpu_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  blsgpu_ctx* handle() const { return h_; }
  static Context& instance() { static Context c(0); return c; }
 private:
  blsgpu_ctx* h_ = nullptr;
};

// src/scalar.rs: only the byte form is on the hot path (Scalar::to_bytes, :284-296)
struct Scalar {
  std::array<uint8_t, 32> bytes{};                       // little-endian canonical integer in [0, r)
  static Scalar from_u64(uint64_t v) { Scalar s; std::memcpy(s.bytes.data(), &v, 8); return s; }
  // scalar.rs:256-280: CtOption::none for a value >= r (here: std::nullopt)
  static std::optional<Scalar> from_bytes(const uint8_t b[32]) {
    static constexpr uint8_t kR[32] = {0x01, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0x02, 0xa4, 0xbd, 0x53,
                                       0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8, 0x39, 0x33, 0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73};
    for (int i = 31; i >= 0; i--) {
      if (b[i] < kR[i]) { Scalar s; std::memcpy(s.bytes.data(), b, 32); return s; }
      if (b[i] > kR[i]) return std::nullopt;
    }
    return std::nullopt;               // == r
  }
  const std::array<uint8_t, 32>& to_bytes() const { return bytes; }
};

namespace detail {
constexpr uint64_t kOne[6] = {0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull};
constexpr uint64_t kG1Gen[12] = {0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull, 0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull, 0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull, 0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull, 0x0bbc3efc5008a26aull};
constexpr uint64_t kG2Gen[24] = {0xf5f28fa202940a10ull, 0xb3f5fb2687b4961aull, 0xa1a893b53e2ae580ull, 0x9894999d1a3caee9ull, 0x6f67b7631863366bull, 0x058191924350bcd7ull, 0xa5a9c0759e23f606ull, 0xaaa0c59dbccd60c3ull, 0x3bb17e18e2867806ull, 0x1b1ab6cc8541b367ull, 0xc2b6ed0ef2158547ull, 0x11922a097360edf3ull, 0x4c730af860494c4aull, 0x597cfa1f5e369c5aull, 0xe7e6856caa0a635aull, 0xbbefb5e96e0d495full, 0x07d3a975f0ef25a2ull, 0x0083fd8e7e80dae5ull, 0xadc0fc92df64b05dull, 0x18aa270a2b1461dcull, 0x86adac6a3be4eba0ull, 0x79495c4ec93da33aull, 0xe7175850a43ccaedull, 0x0b2bc2a163de1bf2ull};
}  // namespace detail

template <int G> struct Projective;

// src/g1.rs:28-32 / src/g2.rs: affine point = x | y limbs + infinity flag
template <int G> struct Affine {
  static constexpr int W = G == 1 ? 12 : 24;
  std::array<uint64_t, W> xy{};
  bool infinity = false;
  static Affine identity() {                                 // (0, 1, infinity)   src/g1.rs:187-193
    Affine a; a.infinity = true; std::memcpy(a.xy.data() + W / 2, detail::kOne, 48); return a;
  }
  static Affine generator() {                                // src/g1.rs:197-217, src/g2.rs:210-250
    Affine a; std::memcpy(a.xy.data(), G == 1 ? detail::kG1Gen : detail::kG2Gen, W * 8); return a;
  }
  bool is_identity() const { return infinity; }
  bool operator==(const Affine& o) const { return (infinity && o.infinity) || (infinity == o.infinity && xy == o.xy); }
  Projective<G> operator*(const Scalar& s) const;            // `&G1Affine * &Scalar`, src/g1.rs:573-579
};

// src/g1.rs:442-446: homogeneous projective (X:Y:Z), identity (0:1:0)
template <int G> struct Projective {
  static constexpr int W = G == 1 ? 18 : 36;
  std::array<uint64_t, W> xyz{};
  static Projective identity() { Projective p; std::memcpy(p.xyz.data() + W / 3, detail::kOne, 48); return p; }
  static Projective generator() {
    Projective p; auto g = Affine<G>::generator();
    std::memcpy(p.xyz.data(), g.xy.data(), g.xy.size() * 8); std::memcpy(p.xyz.data() + 2 * W / 3, detail::kOne, 48); return p;
  }
  Affine<G> to_affine() const {                              // `G1Affine::from(&G1Projective)`, src/g1.rs:49-63
    Affine<G> a; uint8_t inf = 0;
    check((G == 1 ? blsgpu_g1_batch_normalize : blsgpu_g2_batch_normalize)(Context::instance().handle(), xyz.data(), 1, a.xy.data(), &inf), "batch_normalize");
    a.infinity = inf != 0; return a;
  }
  static std::vector<Affine<G>> batch_normalize(const std::vector<Projective>& p) {      // src/g1.rs:806-839
    std::vector<Affine<G>> out(p.size());
    if (p.empty()) return out;
    std::vector<uint64_t> in(p.size() * W), xy(p.size() * Affine<G>::W); std::vector<uint8_t> inf(p.size());
    for (size_t i = 0; i < p.size(); i++) std::memcpy(in.data() + i * W, p[i].xyz.data(), W * 8);
    check((G == 1 ? blsgpu_g1_batch_normalize : blsgpu_g2_batch_normalize)(Context::instance().handle(), in.data(), p.size(), xy.data(), inf.data()), "batch_normalize");
    for (size_t i = 0; i < p.size(); i++) { std::memcpy(out[i].xy.data(), xy.data() + i * Affine<G>::W, Affine<G>::W * 8); out[i].infinity = inf[i] != 0; }
    return out;
  }
  Projective operator+(const Projective& o) const {          // RCB15 Alg. 7, src/g1.rs:670-712
    Projective r; check(blsgpu_point_op(Context::instance().handle(), G, 0, xyz.data(), o.xyz.data(), nullptr, 1, r.xyz.data()), "point add"); return r;
  }
  Projective operator+(const Affine<G>& o) const {           // RCB15 Alg. 8, src/g1.rs:715-752
    Projective r; uint8_t inf = o.infinity;
    check(blsgpu_point_op(Context::instance().handle(), G, 2, xyz.data(), o.xy.data(), &inf, 1, r.xyz.data()), "point add_mixed"); return r;
  }
  Projective dbl() const {                                   // `double`, src/g1.rs:638-667
    Projective r; check(blsgpu_point_op(Context::instance().handle(), G, 1, xyz.data(), nullptr, nullptr, 1, r.xyz.data()), "point double"); return r;
  }
  Projective operator*(const Scalar& s) const { return to_affine() * s; }                // src/g1.rs:556-562
  bool operator==(const Projective& o) const { return to_affine() == o.to_affine(); }    // src/g1.rs:479-496
  static Projective sum(const std::vector<Projective>& p) {                              // `Sum`, src/g1.rs:161-171
    Projective r = identity();
    if (p.empty()) return r;
    std::vector<uint64_t> in(p.size() * W);
    for (size_t i = 0; i < p.size(); i++) std::memcpy(in.data() + i * W, p[i].xyz.data(), W * 8);
    check((G == 1 ? blsgpu_g1_sum : blsgpu_g2_sum)(Context::instance().handle(), in.data(), p.size(), r.xyz.data()), "sum"); return r;
  }
};

// subsets.iter().map(|s| s.iter().map(|&i| points[i]).sum()) in ONE call (blsgpu_g{1,2}_sum_segments; `Sum`, src/g1.rs:161-171): the
// aggregate public keys of many subsets of one key set.  An empty subset gives the identity; an index may repeat.
template <int G> std::vector<Projective<G>> sum_segments(const std::vector<Affine<G>>& points, const std::vector<std::vector<uint32_t>>& subsets) {
  const size_t n = points.size(), nseg = subsets.size();
  std::vector<Projective<G>> out(nseg);
  if (!nseg) return out;
  std::vector<uint64_t> xy(n * Affine<G>::W + 1), offs(nseg + 1, 0); std::vector<uint8_t> inf(n + 1); std::vector<uint32_t> idx;
  for (size_t i = 0; i < n; i++) { std::memcpy(xy.data() + i * Affine<G>::W, points[i].xy.data(), Affine<G>::W * 8); inf[i] = points[i].infinity; }
  for (size_t s = 0; s < nseg; s++) { idx.insert(idx.end(), subsets[s].begin(), subsets[s].end()); offs[s + 1] = idx.size(); }
  const size_t total = idx.size();
  idx.push_back(0);
  std::vector<uint64_t> o(nseg * Projective<G>::W);
  check((G == 1 ? blsgpu_g1_sum_segments : blsgpu_g2_sum_segments)(Context::instance().handle(), xy.data(), inf.data(), n, idx.data(), offs.data(), nseg, total, o.data()),
        "sum_segments");
  for (size_t s = 0; s < nseg; s++) std::memcpy(out[s].xyz.data(), o.data() + s * Projective<G>::W, Projective<G>::W * 8);
  return out;
}

// bases.iter().zip(scalars).map(|(p, s)| p * s).sum()
template <int G> Projective<G> msm(const std::vector<Affine<G>>& bases, const std::vector<Scalar>& scalars) {
  if (bases.size() != scalars.size()) throw std::invalid_argument("msm: bases and scalars differ in length");
  size_t n = bases.size();
  std::vector<uint64_t> xy(n * Affine<G>::W); std::vector<uint8_t> inf(n), s(n * 32);
  for (size_t i = 0; i < n; i++) {
    std::memcpy(xy.data() + i * Affine<G>::W, bases[i].xy.data(), Affine<G>::W * 8);
    inf[i] = bases[i].infinity; std::memcpy(s.data() + 32 * i, scalars[i].bytes.data(), 32);
  }
  Projective<G> r;
  check((G == 1 ? blsgpu_g1_msm_host : blsgpu_g2_msm_host)(Context::instance().handle(), xy.data(), inf.data(), s.data(), n, r.xyz.data()), "msm");
  return r;
}
// points.iter().zip(scalars).map(|(p, s)| p * s) collected: `Mul<&Scalar>` over slices (src/g1.rs:573-579, src/g2.rs:626-632)
template <int G> std::vector<Projective<G>> mul_batch(const std::vector<Affine<G>>& points, const std::vector<Scalar>& scalars) {
  if (points.size() != scalars.size()) throw std::invalid_argument("mul_batch: points and scalars differ in length");
  size_t n = points.size();
  std::vector<uint64_t> xy(n * Affine<G>::W), out(n * Projective<G>::W); std::vector<uint8_t> inf(n), s(n * 32);
  for (size_t i = 0; i < n; i++) {
    std::memcpy(xy.data() + i * Affine<G>::W, points[i].xy.data(), Affine<G>::W * 8);
    inf[i] = points[i].infinity; std::memcpy(s.data() + 32 * i, scalars[i].bytes.data(), 32);
  }
  check((G == 1 ? blsgpu_g1_mul_batch : blsgpu_g2_mul_batch)(Context::instance().handle(), xy.data(), inf.data(), s.data(), n, out.data()), "mul_batch");
  std::vector<Projective<G>> r(n);
  for (size_t i = 0; i < n; i++) std::memcpy(r[i].xyz.data(), out.data() + i * Projective<G>::W, Projective<G>::W * 8);
  return r;
}
template <int G> Projective<G> Affine<G>::operator*(const Scalar& s) const { return mul_batch<G>({*this}, {s})[0]; }

using G1Affine = Affine<1>;
using G2Affine = Affine<2>;
using G1Projective = Projective<1>;
using G2Projective = Projective<2>;
inline std::vector<G1Projective> g1_sum_segments(const std::vector<G1Affine>& points, const std::vector<std::vector<uint32_t>>& subsets) { return sum_segments<1>(points, subsets); }
inline std::vector<G2Projective> g2_sum_segments(const std::vector<G2Affine>& points, const std::vector<std::vector<uint32_t>>& subsets) { return sum_segments<2>(points, subsets); }

// src/pairings.rs:204-337 -- written additively like the reference: + is the Fp12 product, unary - the conjugate
struct Gt {
  std::array<uint64_t, 72> f{};
  static Gt identity() { Gt g; std::memcpy(g.f.data(), detail::kOne, 48); return g; }
  Gt operator+(const Gt& o) const { Gt r; check(blsgpu_fp12_op(Context::instance().handle(), 0, f.data(), o.f.data(), 1, r.f.data()), "Gt add"); return r; }
  Gt operator-() const { Gt r; check(blsgpu_fp12_op(Context::instance().handle(), 8, f.data(), nullptr, 1, r.f.data()), "Gt neg"); return r; }
  Gt dbl() const { Gt r; check(blsgpu_fp12_op(Context::instance().handle(), 3, f.data(), nullptr, 1, r.f.data()), "Gt double"); return r; }
  Gt operator*(const Scalar& s) const {                      // `&Gt * &Scalar`, src/pairings.rs:297-322
    Gt r; check(blsgpu_gt_mul_scalar_batch(Context::instance().handle(), f.data(), s.bytes.data(), 1, r.f.data()), "Gt mul"); return r;
  }
  bool operator==(const Gt& o) const { return f == o.f; }
  static Gt generator();
};

// src/pairings.rs:26 -- no equality on purpose (:21-26)
struct MillerLoopResult {
  std::array<uint64_t, 72> f{};
  static MillerLoopResult default_value() { MillerLoopResult m; std::memcpy(m.f.data(), detail::kOne, 48); return m; }
  Gt final_exponentiation() const {                          // src/pairings.rs:48-176
    Gt g; check(blsgpu_final_exponentiation_batch(Context::instance().handle(), f.data(), 1, g.f.data()), "final_exponentiation"); return g;
  }
  MillerLoopResult operator+(const MillerLoopResult& o) const {                          // src/pairings.rs:179-186
    MillerLoopResult r; check(blsgpu_fp12_op(Context::instance().handle(), 0, f.data(), o.f.data(), 1, r.f.data()), "MillerLoopResult add"); return r;
  }
};

// m `G2Prepared` values resident on the device (blsgpu_g2_prepared): shared by the G2Prepared objects built from it
class PreparedTable {
 public:
  explicit PreparedTable(const std::vector<G2Affine>& pts) {
    std::vector<uint64_t> xy(pts.size() * 24 + 1); std::vector<uint8_t> inf(pts.size() + 1);
    for (size_t i = 0; i < pts.size(); i++) { std::memcpy(xy.data() + 24 * i, pts[i].xy.data(), 192); inf[i] = pts[i].infinity; }
    check(blsgpu_g2_prepare(Context::instance().handle(), xy.data(), inf.data(), pts.size(), &h_), "g2_prepare");
  }
  ~PreparedTable() { blsgpu_g2_prepared_free(h_); }
  PreparedTable(const PreparedTable&) = delete;
  PreparedTable& operator=(const PreparedTable&) = delete;
  const blsgpu_g2_prepared* handle() const { return h_; }
  size_t size() const { return blsgpu_g2_prepared_len(h_); }
 private:
  blsgpu_g2_prepared* h_ = nullptr;
};
// src/pairings.rs:487-546: opaque in the reference.  G2Prepared(q) keeps the affine point (its lines are computed on the fly in every
// Miller loop); G2Prepared::resident(q) / resident_many(points) do what `From<G2Affine>` does in the reference: the 68 coefficient triples
// are computed ONCE, into a device-resident table, and every later multi_miller_loop only evaluates them.
struct G2Prepared {
  G2Affine q;
  std::shared_ptr<PreparedTable> table;                    // null: not resident
  uint32_t index = BLSGPU_UNPREPARED;
  explicit G2Prepared(const G2Affine& p) : q(p) {}
  static std::vector<G2Prepared> resident_many(const std::vector<G2Affine>& pts) {
    auto t = std::make_shared<PreparedTable>(pts);
    std::vector<G2Prepared> out;
    for (size_t i = 0; i < pts.size(); i++) { G2Prepared g(pts[i]); g.table = t; g.index = (uint32_t)i; out.push_back(g); }
    return out;
  }
  static G2Prepared resident(const G2Affine& p) { return resident_many({p})[0]; }
  // `coeffs: Vec<(Fp2, Fp2, Fp2)>` of a resident value: 68 x 3 x 12 u64 in the reference's value format
  std::vector<uint64_t> coeffs() const {
    if (!table) throw std::invalid_argument("G2Prepared::coeffs: not resident");
    std::vector<uint64_t> c(68 * 36); uint8_t inf = 0;
    check(blsgpu_g2_prepared_coeffs(Context::instance().handle(), table->handle(), index, c.data(), &inf), "g2_prepared_coeffs");
    return c;
  }
};
namespace detail {
// the table shared by the resident terms (the first one found) and the per-term indices; terms of another table stay unprepared
template <class It> const PreparedTable* resident_indices(It begin, It end, std::vector<uint32_t>& qi) {
  const PreparedTable* t = nullptr;
  for (It i = begin; i != end; ++i) if (i->second.table) { t = i->second.table.get(); break; }
  if (!t) return nullptr;
  for (It i = begin; i != end; ++i) qi.push_back(i->second.table.get() == t ? i->second.index : BLSGPU_UNPREPARED);
  return t;
}
}  // namespace detail

inline Gt pairing(const G1Affine& p, const G2Affine& q) {    // src/pairings.rs:607-653
  Gt g; uint8_t i1 = p.infinity, i2 = q.infinity;
  check(blsgpu_pairing_batch(Context::instance().handle(), p.xy.data(), &i1, q.xy.data(), &i2, 1, g.f.data()), "pairing"); return g;
}
inline std::vector<Gt> pairing_batch(const std::vector<G1Affine>& p, const std::vector<G2Affine>& q) {
  if (p.size() != q.size()) throw std::invalid_argument("pairing_batch: length mismatch");
  size_t n = p.size(); std::vector<Gt> out(n);
  if (!n) return out;
  std::vector<uint64_t> a(n * 12), b(n * 24), o(n * 72); std::vector<uint8_t> fa(n), fb(n);
  for (size_t i = 0; i < n; i++) { std::memcpy(a.data() + 12 * i, p[i].xy.data(), 96); std::memcpy(b.data() + 24 * i, q[i].xy.data(), 192); fa[i] = p[i].infinity; fb[i] = q[i].infinity; }
  check(blsgpu_pairing_batch(Context::instance().handle(), a.data(), fa.data(), b.data(), fb.data(), n, o.data()), "pairing_batch");
  for (size_t i = 0; i < n; i++) std::memcpy(out[i].f.data(), o.data() + 72 * i, 576);
  return out;
}
inline MillerLoopResult multi_miller_loop(const std::vector<std::pair<G1Affine, G2Prepared>>& terms) {   // src/pairings.rs:554-603
  size_t n = terms.size();
  std::vector<uint64_t> a(n * 12), b(n * 24); std::vector<uint8_t> fa(n), fb(n);
  for (size_t i = 0; i < n; i++) {
    std::memcpy(a.data() + 12 * i, terms[i].first.xy.data(), 96); std::memcpy(b.data() + 24 * i, terms[i].second.q.xy.data(), 192);
    fa[i] = terms[i].first.infinity; fb[i] = terms[i].second.q.infinity;
  }
  MillerLoopResult m;
  std::vector<uint32_t> qi;
  if (const PreparedTable* t = detail::resident_indices(terms.begin(), terms.end(), qi))
    check(blsgpu_multi_miller_loop_prepared(Context::instance().handle(), a.data(), fa.data(), b.data(), fb.data(), qi.data(), t->handle(), n, m.f.data()), "multi_miller_loop_prepared");
  else
    check(blsgpu_multi_miller_loop(Context::instance().handle(), a.data(), fa.data(), b.data(), fb.data(), n, m.f.data()), "multi_miller_loop");
  return m;
}
// N independent `multi_miller_loop(..).final_exponentiation()` in one device call: the bulk form of signature verification
// (src/pairings.rs:554-603, 817-824; blsgpu_multi_miller_loop_many)
inline std::vector<Gt> multi_miller_loop_many(const std::vector<std::vector<std::pair<G1Affine, G2Prepared>>>& equations) {
  size_t n = 0;
  std::vector<uint64_t> off(equations.size() + 1, 0);
  for (size_t s = 0; s < equations.size(); s++) { n += equations[s].size(); off[s + 1] = n; }
  std::vector<uint64_t> a(n * 12 + 1), b(n * 24 + 1), o(equations.size() * 72 + 1); std::vector<uint8_t> fa(n + 1), fb(n + 1);
  size_t i = 0;
  for (const auto& e : equations)
    for (const auto& t : e) {
      std::memcpy(a.data() + 12 * i, t.first.xy.data(), 96); std::memcpy(b.data() + 24 * i, t.second.q.xy.data(), 192);
      fa[i] = t.first.infinity; fb[i] = t.second.q.infinity; i++;
    }
  std::vector<std::pair<G1Affine, G2Prepared>> flat;
  for (const auto& e : equations) flat.insert(flat.end(), e.begin(), e.end());
  std::vector<uint32_t> qi;
  if (const PreparedTable* t = detail::resident_indices(flat.begin(), flat.end(), qi))
    check(blsgpu_multi_miller_loop_prepared_many(Context::instance().handle(), a.data(), fa.data(), b.data(), fb.data(), qi.data(), t->handle(), off.data(), equations.size(), 1,
                                                 o.data()), "multi_miller_loop_prepared_many");
  else
    check(blsgpu_multi_miller_loop_many(Context::instance().handle(), a.data(), fa.data(), b.data(), fb.data(), off.data(), equations.size(), 1, o.data()), "multi_miller_loop_many");
  std::vector<Gt> out(equations.size());
  for (size_t s = 0; s < equations.size(); s++) std::memcpy(out[s].f.data(), o.data() + 72 * s, 576);
  return out;
}
inline Gt Gt::generator() { return pairing(G1Affine::generator(), G2Affine::generator()); }            // src/pairings.rs:359-475

// Bulk signature verification from bytes (blsgpu_bls_verify_batch): compressed keys, signatures and messages in, one verdict byte each
// out (1 valid, 0 invalid, 2 bad key encoding, 3 bad signature encoding); keys_in_g1 = true: 48-byte keys / 96-byte signatures
inline std::vector<uint8_t> bls_verify_batch(bool keys_in_g1, const std::vector<uint8_t>& pk_bytes, const std::vector<uint8_t>& sig_bytes, const std::vector<std::string>& msgs,
                                             const std::string& dst) {
  const size_t n = msgs.size();
  if (pk_bytes.size() != n * (keys_in_g1 ? 48 : 96) || sig_bytes.size() != n * (keys_in_g1 ? 96 : 48)) throw std::invalid_argument("bls_verify_batch: byte lengths");
  std::vector<uint8_t> verdict(n);
  if (!n) return verdict;
  std::vector<uint64_t> offs(n + 1, 0); std::string blob;
  for (size_t i = 0; i < n; i++) { blob += msgs[i]; offs[i + 1] = blob.size(); }
  check(blsgpu_bls_verify_batch(Context::instance().handle(), keys_in_g1 ? 0 : 1, pk_bytes.data(), sig_bytes.data(), (const uint8_t*)blob.data(), offs.data(), n,
                                (const uint8_t*)dst.data(), dst.size(), verdict.data()), "bls_verify_batch");
  return verdict;
}

// Aggregate verification (blsgpu_bls_fast_aggregate_verify_batch): signature i over msgs[i] by the keys subsets[i] of a key set that is
// RESIDENT on the device -- d_keys_xy / d_keys_infinity are device pointers to nkeys decoded affine points (G1 if keys_in_g1), decoded and
// subgroup-checked once by the caller.  Verdicts: 1 valid, 0 invalid, 3 bad signature encoding.  An empty subset takes part as an identity key.
inline std::vector<uint8_t> bls_fast_aggregate_verify(bool keys_in_g1, const void* d_keys_xy, const void* d_keys_infinity, size_t nkeys,
                                                      const std::vector<std::vector<uint32_t>>& subsets, const std::vector<uint8_t>& sig_bytes,
                                                      const std::vector<std::string>& msgs, const std::string& dst) {
  const size_t n = msgs.size();
  if (subsets.size() != n || sig_bytes.size() != n * (keys_in_g1 ? 96 : 48)) throw std::invalid_argument("bls_fast_aggregate_verify: lengths");
  std::vector<uint8_t> verdict(n);
  if (!n) return verdict;
  std::vector<uint64_t> offs(n + 1, 0), koffs(n + 1, 0); std::string blob; std::vector<uint32_t> idx;
  for (size_t i = 0; i < n; i++) { blob += msgs[i]; offs[i + 1] = blob.size(); idx.insert(idx.end(), subsets[i].begin(), subsets[i].end()); koffs[i + 1] = idx.size(); }
  const size_t total = idx.size();
  idx.push_back(0);
  check(blsgpu_bls_fast_aggregate_verify_batch(Context::instance().handle(), keys_in_g1 ? 0 : 1, d_keys_xy, d_keys_infinity, nkeys, idx.data(), koffs.data(), total,
                                               sig_bytes.data(), (const uint8_t*)blob.data(), offs.data(), n, (const uint8_t*)dst.data(), dst.size(), verdict.data()),
        "bls_fast_aggregate_verify");
  return verdict;
}

// src/hash_to_curve/mod.rs:86-108 with ExpandMsgXmd<Sha256>: `G::hash_to_curve(msg, dst)` / `G::encode_to_curve(msg, dst)` for a batch
template <int G> std::vector<Projective<G>> hash_to_curve(const std::vector<std::string>& msgs, const std::string& dst, bool encode_only = false) {
  std::vector<Projective<G>> out(msgs.size());
  if (msgs.empty()) return out;
  std::vector<uint64_t> offs(msgs.size() + 1, 0); std::string blob;
  for (size_t i = 0; i < msgs.size(); i++) { blob += msgs[i]; offs[i + 1] = blob.size(); }
  std::vector<uint64_t> xyz(msgs.size() * Projective<G>::W);
  check((G == 1 ? blsgpu_g1_hash_to_curve_batch : blsgpu_g2_hash_to_curve_batch)(Context::instance().handle(), (const uint8_t*)blob.data(), offs.data(), msgs.size(),
                                                                                 (const uint8_t*)dst.data(), dst.size(), encode_only ? 1 : 0, xyz.data()), "hash_to_curve");
  for (size_t i = 0; i < msgs.size(); i++) std::memcpy(out[i].xyz.data(), xyz.data() + i * Projective<G>::W, Projective<G>::W * 8);
  return out;
}

// src/scalar.rs: vectors of `Scalar([u64; 4])` (Montgomery limbs) -- element-wise arithmetic and the radix-2 transform built on ROOT_OF_UNITY
using FrLimbs = std::array<uint64_t, 4>;
enum class FrOp { Mul = 0, Add = 1, Sub = 2, Square = 3, Invert = 4, Neg = 5, Double = 6 };
inline std::vector<FrLimbs> fr_op(FrOp op, const std::vector<FrLimbs>& a, const std::vector<FrLimbs>& b = {}) {
  std::vector<FrLimbs> out(a.size());
  if (a.empty()) return out;
  if ((int)op <= 2 && b.size() != a.size()) throw std::invalid_argument("fr_op: operands differ in length");
  check(blsgpu_fr_op(Context::instance().handle(), (int)op, a[0].data(), b.empty() ? nullptr : b[0].data(), a.size(), out[0].data(), nullptr), "fr_op");
  return out;
}
inline void fr_ntt(std::vector<FrLimbs>& v, bool inverse = false) {         // natural order in and out; v.size() a power of two
  if (v.empty() || (v.size() & (v.size() - 1))) throw std::invalid_argument("fr_ntt: length must be a power of two");
  int log_n = 0; while (((size_t)1 << log_n) < v.size()) log_n++;
  check(blsgpu_fr_ntt(Context::instance().handle(), v[0].data(), log_n, inverse ? 1 : 0), "fr_ntt");
}
// k transforms of v.size() / k scalars each in one call (vector i = elements [i n, (i+1) n)); coset: the Montgomery limbs of a non-zero
// shift g -- the values on g * <w> (forward) and back (inverse) -- or nullptr for the plain transform
inline void fr_ntt_many(std::vector<FrLimbs>& v, size_t k, bool inverse = false, const FrLimbs* coset = nullptr) {
  if (k == 0 && v.empty()) return;
  if (k == 0 || v.empty() || v.size() % k) throw std::invalid_argument("fr_ntt_many: the length must be k vectors of equal size");
  const size_t n = v.size() / k;
  if (n & (n - 1)) throw std::invalid_argument("fr_ntt_many: the vector length must be a power of two");
  int log_n = 0; while (((size_t)1 << log_n) < n) log_n++;
  check(blsgpu_fr_ntt_many(Context::instance().handle(), v[0].data(), log_n, k, inverse ? 1 : 0, coset ? coset->data() : nullptr), "fr_ntt_many");
}
// Recurrences along k rows of v.size() / k scalars each in one call (include/bls12_381_hip.h): running sums / products (inclusive, or
// exclusive), or Horner rows -- row i = the coefficients of p_i, points[i] = z: out row = p_i(z), then the quotient (p_i(X) - p_i(z)) / (X - z)
enum class FrScan { Sum = 0, Product = 1, Horner = 2 };
inline std::vector<FrLimbs> fr_scan(FrScan op, const std::vector<FrLimbs>& v, size_t k, const std::vector<FrLimbs>& points = {}, bool exclusive = false) {
  std::vector<FrLimbs> out(v.size());
  if (v.empty()) return out;
  if (k == 0 || v.size() % k) throw std::invalid_argument("fr_scan: the length must be k rows of equal size");
  if (op == FrScan::Horner && (points.size() != k || exclusive)) throw std::invalid_argument("fr_scan: HORNER takes one point per row and no exclusive form");
  check(blsgpu_fr_scan_many(Context::instance().handle(), (int)op, exclusive ? 1 : 0, v[0].data(), v.size() / k, k, points.empty() ? nullptr : points[0].data(), out[0].data()), "fr_scan");
  return out;
}
// element-wise inverses by Montgomery's trick: limb-identical to fr_op(FrOp::Invert, ...), 0 for a zero (nonzero, if given, gets the flags)
inline std::vector<FrLimbs> fr_batch_invert(const std::vector<FrLimbs>& v, std::vector<uint8_t>* nonzero = nullptr) {
  std::vector<FrLimbs> out(v.size());
  if (nonzero) nonzero->assign(v.size(), 1);
  if (v.empty()) return out;
  check(blsgpu_fr_batch_invert(Context::instance().handle(), v[0].data(), v.size(), out[0].data(), nonzero ? nonzero->data() : nullptr), "fr_batch_invert");
  return out;
}
// Lagrange coefficients at arbitrary nodes for many subsets in one call (include/bls12_381_hip.h: blsgpu_fr_lagrange_segments):
// lambda_i = prod_{j != i} (z - x_j) * inv0(prod_{j != i} (x_i - x_j)) for subset s = nodes[s] at the point points[s] (points empty:
// every z = 0).  values, if given, has the shape of nodes and y gets sum_i lambda_i values_i per subset; distinct gets 1 per subset whose
// nodes are pairwise distinct.  Returns the coefficients in the shape of nodes.
struct FrLagrange { std::vector<std::vector<FrLimbs>> lambda; std::vector<FrLimbs> y; std::vector<uint8_t> distinct; };
namespace detail {
inline size_t lagrange_flatten(const std::vector<std::vector<FrLimbs>>& nodes, std::vector<FrLimbs>& flat, std::vector<uint32_t>& offs) {
  offs.assign(nodes.size() + 1, 0);
  for (size_t s = 0; s < nodes.size(); s++) { flat.insert(flat.end(), nodes[s].begin(), nodes[s].end()); offs[s + 1] = (uint32_t)flat.size(); }
  const size_t total = flat.size();
  flat.push_back(FrLimbs{});
  return total;
}
}  // namespace detail
inline FrLagrange fr_lagrange_segments(const std::vector<std::vector<FrLimbs>>& nodes, const std::vector<FrLimbs>& points = {},
                                       const std::vector<std::vector<FrLimbs>>& values = {}) {
  const size_t nseg = nodes.size();
  FrLagrange r;
  r.lambda.resize(nseg); r.distinct.assign(nseg, 1);
  if (!nseg) return r;
  if (!points.empty() && points.size() != nseg) throw std::invalid_argument("fr_lagrange_segments: one point per subset");
  std::vector<FrLimbs> x, v; std::vector<uint32_t> offs, voffs;
  const size_t total = detail::lagrange_flatten(nodes, x, offs);
  if (!values.empty() && (detail::lagrange_flatten(values, v, voffs) != total || voffs != offs)) throw std::invalid_argument("fr_lagrange_segments: values must have the shape of nodes");
  std::vector<FrLimbs> lam(total + 1);
  if (!values.empty()) r.y.resize(nseg);
  check(blsgpu_fr_lagrange_segments(Context::instance().handle(), x[0].data(), offs.data(), nseg, points.empty() ? nullptr : points[0].data(), values.empty() ? nullptr : v[0].data(),
                                    lam[0].data(), values.empty() ? nullptr : r.y[0].data(), r.distinct.data()), "fr_lagrange_segments");
  for (size_t s = 0; s < nseg; s++) r.lambda[s].assign(lam.begin() + offs[s], lam.begin() + offs[s + 1]);
  return r;
}
// Interpolation in the exponent (blsgpu_g{1,2}_lagrange_combine): out[s] = sum_i lambda_i * shares[s][i], lambda as above -- t partial
// signatures into the group's.  shares has the shape of nodes; an empty subset gives the identity.
template <int G> std::vector<Projective<G>> lagrange_combine(const std::vector<std::vector<Affine<G>>>& shares, const std::vector<std::vector<FrLimbs>>& nodes,
                                                             const std::vector<FrLimbs>& points = {}, std::vector<uint8_t>* distinct = nullptr) {
  const size_t nseg = nodes.size();
  std::vector<Projective<G>> out(nseg);
  if (distinct) distinct->assign(nseg, 1);
  if (!nseg) return out;
  if (shares.size() != nseg || (!points.empty() && points.size() != nseg)) throw std::invalid_argument("lagrange_combine: one subset of shares and one point per subset of nodes");
  std::vector<FrLimbs> x; std::vector<uint32_t> offs;
  const size_t total = detail::lagrange_flatten(nodes, x, offs);
  std::vector<uint64_t> xy((total + 1) * Affine<G>::W), o(nseg * Projective<G>::W); std::vector<uint8_t> inf(total + 1);
  for (size_t s = 0, t = 0; s < nseg; s++) {
    if (shares[s].size() != nodes[s].size()) throw std::invalid_argument("lagrange_combine: shares must have the shape of nodes");
    for (const auto& p : shares[s]) { std::memcpy(xy.data() + t * Affine<G>::W, p.xy.data(), Affine<G>::W * 8); inf[t++] = p.infinity; }
  }
  check((G == 1 ? blsgpu_g1_lagrange_combine : blsgpu_g2_lagrange_combine)(Context::instance().handle(), xy.data(), inf.data(), x[0].data(), offs.data(), nseg,
                                                                          points.empty() ? nullptr : points[0].data(), o.data(), distinct ? distinct->data() : nullptr),
        "lagrange_combine");
  for (size_t s = 0; s < nseg; s++) std::memcpy(out[s].xyz.data(), o.data() + s * Projective<G>::W, Projective<G>::W * 8);
  return out;
}
inline std::vector<G1Projective> g1_lagrange_combine(const std::vector<std::vector<G1Affine>>& shares, const std::vector<std::vector<FrLimbs>>& nodes,
                                                     const std::vector<FrLimbs>& points = {}, std::vector<uint8_t>* distinct = nullptr) { return lagrange_combine<1>(shares, nodes, points, distinct); }
inline std::vector<G2Projective> g2_lagrange_combine(const std::vector<std::vector<G2Affine>>& shares, const std::vector<std::vector<FrLimbs>>& nodes,
                                                     const std::vector<FrLimbs>& points = {}, std::vector<uint8_t>* distinct = nullptr) { return lagrange_combine<2>(shares, nodes, points, distinct); }
// Fraction scans (include/bls12_381_hip.h: blsgpu_fr_grand_product / blsgpu_fr_frac_sum): a column set is c tables of k rows, packed --
// set.size() = c * k * len -- and an empty set stands for NULL (num_b, den_b: no beta term; mult: every multiplicity is 1).
// fr_grand_product: f[i] = prod_j (num_a_j + beta num_b_j + gamma)[i] * inv0(prod_j (den_a_j + beta den_b_j + gamma)[i]), the PRODUCT scan
// of f along each row; fr_frac_sum: f[i] = sum_j mult_j[i] * inv0(gamma + den_a_j[i] + beta den_b_j[i]), the SUM scan.  nonzero, if given,
// gets a byte per element: 0 where a denominator factor was zero.
namespace detail {
inline size_t fr_frac_len(const char* what, size_t set, size_t c, size_t k, std::initializer_list<size_t> others) {
  if (c == 0 || k == 0 || set % (c * k)) throw std::invalid_argument(std::string(what) + ": a set must be c tables of k rows of equal length");
  for (size_t o : others) if (o && o != set) throw std::invalid_argument(std::string(what) + ": the column sets differ in size");
  return set / (c * k);
}
}  // namespace detail
inline std::vector<FrLimbs> fr_grand_product(size_t c, size_t k, const std::vector<FrLimbs>& num_a, const std::vector<FrLimbs>& num_b, const std::vector<FrLimbs>& den_a,
                                             const std::vector<FrLimbs>& den_b, const FrLimbs& beta, const FrLimbs& gamma, bool exclusive = false, std::vector<uint8_t>* nonzero = nullptr) {
  if (den_a.size() != num_a.size()) throw std::invalid_argument("fr_grand_product: num_a and den_a differ in size");
  const size_t len = detail::fr_frac_len("fr_grand_product", num_a.size(), c, k, {num_b.size(), den_b.size()});
  std::vector<FrLimbs> out(k * len);
  if (nonzero) nonzero->assign(k * len, 1);
  if (out.empty()) return out;
  const FrLimbs chal[2] = {beta, gamma};
  check(blsgpu_fr_grand_product(Context::instance().handle(), exclusive ? 1 : 0, (int)c, num_a[0].data(), num_b.empty() ? nullptr : num_b[0].data(), den_a[0].data(),
                                den_b.empty() ? nullptr : den_b[0].data(), chal[0].data(), len, k, out[0].data(), nonzero ? nonzero->data() : nullptr), "fr_grand_product");
  return out;
}
inline std::vector<FrLimbs> fr_frac_sum(size_t c, size_t k, const std::vector<FrLimbs>& mult, const std::vector<FrLimbs>& den_a, const std::vector<FrLimbs>& den_b, const FrLimbs& beta,
                                        const FrLimbs& gamma, bool exclusive = false, std::vector<uint8_t>* nonzero = nullptr) {
  const size_t len = detail::fr_frac_len("fr_frac_sum", den_a.size(), c, k, {mult.size(), den_b.size()});
  std::vector<FrLimbs> out(k * len);
  if (nonzero) nonzero->assign(k * len, 1);
  if (out.empty()) return out;
  const FrLimbs chal[2] = {beta, gamma};
  check(blsgpu_fr_frac_sum(Context::instance().handle(), exclusive ? 1 : 0, (int)c, mult.empty() ? nullptr : mult[0].data(), den_a[0].data(), den_b.empty() ? nullptr : den_b[0].data(),
                           chal[0].data(), len, k, out[0].data(), nonzero ? nonzero->data() : nullptr), "fr_frac_sum");
  return out;
}
// Polynomials in evaluation form (include/bls12_381_hip.h: blsgpu_fr_bary_*): k rows of evals.size() / k = 2^log_n values on the roots of
// unity, in natural or bit-reversed order, points[i] = z of row i (inside the domain or not).  fr_bary_eval returns y[i] = p_i(z_i);
// fr_bary_open also the values of (p_i(X) - y[i]) / (X - z_i) on the same domain, in the same order.
enum class FrOrder { Natural = 0, BitReversed = 1 };
struct FrOpening { std::vector<FrLimbs> y, q; };
namespace detail {
inline int fr_bary_log_n(const char* what, size_t len, size_t k, size_t points) {
  if (k == 0 || len == 0 || len % k || points != k) throw std::invalid_argument(std::string(what) + ": k rows of equal size and one point per row");
  const size_t n = len / k;
  if (n & (n - 1)) throw std::invalid_argument(std::string(what) + ": the row length must be a power of two");
  int log_n = 0; while (((size_t)1 << log_n) < n) log_n++;
  return log_n;
}
}  // namespace detail
inline std::vector<FrLimbs> fr_bary_eval(const std::vector<FrLimbs>& evals, size_t k, const std::vector<FrLimbs>& points, FrOrder order = FrOrder::Natural) {
  const int log_n = detail::fr_bary_log_n("fr_bary_eval", evals.size(), k, points.size());
  std::vector<FrLimbs> y(k);
  check(blsgpu_fr_bary_eval_many(Context::instance().handle(), evals[0].data(), log_n, k, points[0].data(), (int)order, y[0].data()), "fr_bary_eval");
  return y;
}
inline FrOpening fr_bary_open(const std::vector<FrLimbs>& evals, size_t k, const std::vector<FrLimbs>& points, FrOrder order = FrOrder::Natural) {
  const int log_n = detail::fr_bary_log_n("fr_bary_open", evals.size(), k, points.size());
  FrOpening o{std::vector<FrLimbs>(k), std::vector<FrLimbs>(evals.size())};
  check(blsgpu_fr_bary_open_many(Context::instance().handle(), evals[0].data(), log_n, k, points[0].data(), (int)order, o.y[0].data(), o.q[0].data()), "fr_bary_open");
  return o;
}
// A CSR matrix over Fr resident on the device (blsgpu_fr_matrix): validated and planned once, multiplied many times.  row_ptr has
// n_rows + 1 entries from 0 to nnz = col.size() = val.size(); col[p] < n_cols; repeated columns inside a row add; rows may be empty.
class FrMatrix {
 public:
  FrMatrix(const std::vector<uint32_t>& row_ptr, const std::vector<uint32_t>& col, const std::vector<FrLimbs>& val, size_t n_cols) {
    if (row_ptr.empty() || col.size() != val.size() || row_ptr.back() != col.size()) throw std::invalid_argument("FrMatrix: row_ptr must run from 0 to col.size() == val.size()");
    check(blsgpu_fr_matrix_upload(Context::instance().handle(), row_ptr.size() - 1, n_cols, row_ptr.data(), col.data(), val.empty() ? nullptr : val[0].data(), &m_), "fr_matrix_upload");
  }
  ~FrMatrix() { blsgpu_fr_matrix_free(m_); }
  FrMatrix(const FrMatrix&) = delete;
  FrMatrix& operator=(const FrMatrix&) = delete;
  FrMatrix(FrMatrix&& o) noexcept : m_(o.m_) { o.m_ = nullptr; }
  size_t rows() const { return blsgpu_fr_matrix_rows(m_); }
  size_t cols() const { return blsgpu_fr_matrix_cols(m_); }
  size_t nnz() const { return blsgpu_fr_matrix_nnz(m_); }
  const blsgpu_fr_matrix* handle() const { return m_; }
 private:
  blsgpu_fr_matrix* m_ = nullptr;
};
// out[v][i] = sum over row i's entries of val[p] * x[v][col[p]] for k = x.size() / m.cols() right-hand sides laid end to end; stack A, B and
// C into one matrix of 3n rows to apply all three in one call
inline std::vector<FrLimbs> fr_spmv(const FrMatrix& m, const std::vector<FrLimbs>& x) {
  if (m.cols() == 0 || x.size() % m.cols()) throw std::invalid_argument("fr_spmv: x must be k vectors of m.cols() scalars");
  const size_t k = x.size() / m.cols();
  std::vector<FrLimbs> out(k * m.rows());
  if (out.empty()) return out;
  check(blsgpu_fr_spmv(Context::instance().handle(), m.handle(), x[0].data(), k, out[0].data()), "fr_spmv");
  return out;
}
// A Poseidon instance over Fr resident on the device (blsgpu_fr_poseidon): width t, r_full full and r_partial partial rounds, round
// constants (r_full + r_partial) x t and the t x t matrix (row-major) as canonical Montgomery limbs.  THE PARAMETERS ARE THE CALLER'S: the
// library ships no standard set.  Validated and planned once; Form::Auto takes the sparse partial rounds when they can be derived.
// permute: n states of t scalars end to end; hash_many: n preimages of t - 1 scalars, the digest is element 1 of the permutation of
// (tag, x_1 .. x_(t-1)); merkle: k trees of (t-1)^height leaves each, tree after tree -> the k roots, and every inner level (level 1
// first, the roots last) in *nodes when it is given.
class FrPoseidon {
 public:
  enum class Form { Auto = BLSGPU_FR_POSEIDON_AUTO, Dense = BLSGPU_FR_POSEIDON_DENSE, Sparse = BLSGPU_FR_POSEIDON_SPARSE };
  FrPoseidon(int t, int r_full, int r_partial, const std::vector<FrLimbs>& round_constants, const std::vector<FrLimbs>& mds, Form form = Form::Auto) {
    if (t < 1 || r_full < 0 || r_partial < 0 || round_constants.size() != (size_t)(r_full + r_partial) * t || mds.size() != (size_t)t * t)
      throw std::invalid_argument("FrPoseidon: (r_full + r_partial) * t round constants and t * t matrix entries");
    check(blsgpu_fr_poseidon_create(Context::instance().handle(), t, r_full, r_partial, round_constants.data()->data(), mds.data()->data(), (int)form, &p_), "fr_poseidon_create");
  }
  ~FrPoseidon() { blsgpu_fr_poseidon_free(p_); }
  FrPoseidon(const FrPoseidon&) = delete;
  FrPoseidon& operator=(const FrPoseidon&) = delete;
  FrPoseidon(FrPoseidon&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  int width() const { return blsgpu_fr_poseidon_width(p_); }
  int rounds_full() const { return blsgpu_fr_poseidon_rounds_full(p_); }
  int rounds_partial() const { return blsgpu_fr_poseidon_rounds_partial(p_); }
  Form form() const { return (Form)blsgpu_fr_poseidon_form(p_); }
  size_t products_per_permutation() const { return blsgpu_fr_poseidon_products(p_); }
  const blsgpu_fr_poseidon* handle() const { return p_; }
  std::vector<FrLimbs> permute(const std::vector<FrLimbs>& states) const {
    if (states.size() % (size_t)width()) throw std::invalid_argument("FrPoseidon::permute: n states of t scalars");
    std::vector<FrLimbs> out(states.size());
    if (out.empty()) return out;
    check(blsgpu_fr_poseidon_permute(Context::instance().handle(), p_, states[0].data(), states.size() / (size_t)width(), out[0].data()), "fr_poseidon_permute");
    return out;
  }
  std::vector<FrLimbs> hash_many(const FrLimbs& tag, const std::vector<FrLimbs>& inputs) const {
    const size_t a = (size_t)width() - 1;
    if (inputs.size() % a) throw std::invalid_argument("FrPoseidon::hash_many: n preimages of t - 1 scalars");
    std::vector<FrLimbs> out(inputs.size() / a);
    if (out.empty()) return out;
    check(blsgpu_fr_poseidon_hash_many(Context::instance().handle(), p_, tag.data(), inputs[0].data(), out.size(), out[0].data()), "fr_poseidon_hash_many");
    return out;
  }
  std::vector<FrLimbs> merkle(const FrLimbs& tag, const std::vector<FrLimbs>& leaves, int height, size_t k, std::vector<FrLimbs>* nodes = nullptr) const {
    const size_t a = (size_t)width() - 1;
    size_t per = 1;
    for (int i = 0; i < height; i++) per *= a;
    if (height < 0 || leaves.size() != k * per) throw std::invalid_argument("FrPoseidon::merkle: k trees of (t-1)^height leaves");
    std::vector<FrLimbs> roots(k);
    if (!k) return roots;
    if (nodes) nodes->assign(a == 1 ? k * (size_t)height : k * ((per - 1) / (a - 1)), FrLimbs{});
    check(blsgpu_fr_poseidon_merkle(Context::instance().handle(), p_, tag.data(), leaves[0].data(), height, k, nodes && !nodes->empty() ? (*nodes)[0].data() : nullptr, roots[0].data()),
          "fr_poseidon_merkle");
    return roots;
  }
 private:
  blsgpu_fr_poseidon* p_ = nullptr;
};
// An Fr expression program resident on the device (blsgpu_fr_expr; include/bls12_381_hip.h documents the format): straight-line code
// over columns, registers and constants, validated once by the constructor (a bad program throws with the instruction index and the
// rule), evaluated per row in one pass by eval().  Build the code with the static helpers:
//   FrExpr::Code code; code.mul(0, FrExpr::col(0), FrExpr::col(1)); code.mad(0, FrExpr::col(2, +1), FrExpr::constant(0)); ...
// The row's result is the dst of the last instruction.  eval: cols[j] holds 2^col_log_len[j] scalars (col_log_len empty: every column
// has N = 2^log_n), read modulo its own length at (row + rot * 2^log_stride); a column the program does not read may be left empty.
// The domain point X and L_1 are columns, not operands: the coset transforms of (0, 1, 0, ...) and of (1/n, ..., 1/n, 0, ..., 0).
class FrExpr {
 public:
  static uint32_t reg(unsigned i) { return BLSGPU_FR_EXPR_REG(i); }
  static uint32_t col(unsigned j, int rot = 0) { return BLSGPU_FR_EXPR_COL(j, rot); }
  static uint32_t constant(unsigned i) { return BLSGPU_FR_EXPR_CONST(i); }
  struct Code {
    std::vector<uint32_t> words;
    Code& add(unsigned dst, uint32_t a, uint32_t b) { return push(BLSGPU_FR_EXPR_ADD, dst, a, b); }
    Code& sub(unsigned dst, uint32_t a, uint32_t b) { return push(BLSGPU_FR_EXPR_SUB, dst, a, b); }
    Code& mul(unsigned dst, uint32_t a, uint32_t b) { return push(BLSGPU_FR_EXPR_MUL, dst, a, b); }
    Code& mad(unsigned dst, uint32_t a, uint32_t b) { return push(BLSGPU_FR_EXPR_MAD, dst, a, b); }
    Code& mov(unsigned dst, uint32_t a) { return push(BLSGPU_FR_EXPR_MOV, dst, a, 0); }
    Code& push(unsigned op, unsigned dst, uint32_t a, uint32_t b) { words.push_back(BLSGPU_FR_EXPR_INSTR(op, dst)); words.push_back(a); words.push_back(b); return *this; }
  };
  FrExpr(int n_cols, int n_regs, const std::vector<FrLimbs>& consts, const Code& code) {
    check(blsgpu_fr_expr_create(Context::instance().handle(), n_cols, n_regs, (int)consts.size(), consts.empty() ? nullptr : consts[0].data(), code.words.size() / 3,
                                code.words.data(), &e_), "fr_expr_create");
  }
  ~FrExpr() { blsgpu_fr_expr_free(e_); }
  FrExpr(const FrExpr&) = delete;
  FrExpr& operator=(const FrExpr&) = delete;
  FrExpr(FrExpr&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  int cols() const { return blsgpu_fr_expr_cols(e_); }
  int regs() const { return blsgpu_fr_expr_regs(e_); }
  size_t instructions() const { return blsgpu_fr_expr_instructions(e_); }
  size_t products_per_row() const { return blsgpu_fr_expr_products(e_); }
  uint32_t cols_read() const { return blsgpu_fr_expr_cols_read(e_); }
  const blsgpu_fr_expr* handle() const { return e_; }
  std::vector<FrLimbs> eval(const std::vector<std::vector<FrLimbs>>& columns, int log_n, int log_stride = 0, const std::vector<uint8_t>& col_log_len = {}) const {
    if (columns.size() != (size_t)cols() || (!col_log_len.empty() && col_log_len.size() != columns.size()))
      throw std::invalid_argument("FrExpr::eval: one column (and one col_log_len, if any) per column of the program");
    if (log_n < 0 || log_n > 28) throw std::invalid_argument("FrExpr::eval: log_n must be in [0, 28]");
    std::vector<const uint64_t*> ptr(columns.size(), nullptr);
    for (size_t j = 0; j < columns.size(); j++) {
      if (columns[j].empty()) continue;
      const int ll = col_log_len.empty() ? log_n : (int)col_log_len[j];
      if (ll > 28 || columns[j].size() != (size_t)1 << ll) throw std::invalid_argument("FrExpr::eval: a column does not have 2^col_log_len scalars");
      ptr[j] = columns[j][0].data();
    }
    std::vector<FrLimbs> out((size_t)1 << log_n);
    check(blsgpu_fr_expr_eval(Context::instance().handle(), e_, ptr.data(), col_log_len.empty() ? nullptr : col_log_len.data(), log_n, log_stride, out[0].data()), "fr_expr_eval");
    return out;
  }
 private:
  blsgpu_fr_expr* e_ = nullptr;
};
// A lookup table over Fr resident on the device (include/bls12_381_hip.h: blsgpu_fr_lookup_*): an index over rows of c scalars, built
// once by the constructor from c columns of equal length (a key is the tuple (columns[0][i], ..., columns[c - 1][i])).  count() gives
// the logUp multiplicity column for the looked-up rows f (m[j] = how often row j's key occurs in f if j is the FIRST row with that key,
// else 0; r - m with negate, ready for fr_frac_sum's mult), the first table row of every looked-up row (FrLookup::miss for none) and the
// number of looked-up rows that are in no table row.  Keys are compared limb for limb: inputs are canonical Montgomery limbs.
class FrLookup {
 public:
  static constexpr uint32_t miss = BLSGPU_FR_LOOKUP_MISS;
  struct Counts { std::vector<FrLimbs> mult; std::vector<uint32_t> index; uint64_t missing = 0; };
  explicit FrLookup(const std::vector<std::vector<FrLimbs>>& columns) {
    const std::vector<uint64_t> t = pack(columns, "FrLookup");
    check(blsgpu_fr_lookup_create(Context::instance().handle(), (int)columns.size(), t.data(), columns[0].size(), &h_), "fr_lookup_create");
  }
  ~FrLookup() { blsgpu_fr_lookup_free(h_); }
  FrLookup(const FrLookup&) = delete;
  FrLookup& operator=(const FrLookup&) = delete;
  FrLookup(FrLookup&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  int cols() const { return blsgpu_fr_lookup_cols(h_); }
  size_t rows() const { return blsgpu_fr_lookup_rows(h_); }
  size_t distinct() const { return blsgpu_fr_lookup_distinct(h_); }
  size_t slots() const { return blsgpu_fr_lookup_slots(h_); }
  const blsgpu_fr_lookup* handle() const { return h_; }
  Counts count(const std::vector<std::vector<FrLimbs>>& f, bool negate = false) const {
    if (f.size() != (size_t)cols()) throw std::invalid_argument("FrLookup::count: one column per column of the table");
    const std::vector<uint64_t> v = pack(f, "FrLookup::count");
    const size_t n = f[0].size();
    Counts r;
    r.mult.resize(rows());
    r.index.resize(n);
    check(blsgpu_fr_lookup_count(Context::instance().handle(), h_, n ? v.data() : nullptr, n, negate ? 1 : 0, r.mult[0].data(), n ? r.index.data() : nullptr, &r.missing), "fr_lookup_count");
    return r;
  }
 private:
  static std::vector<uint64_t> pack(const std::vector<std::vector<FrLimbs>>& columns, const char* what) {
    if (columns.empty()) throw std::invalid_argument(std::string(what) + ": at least one column");
    std::vector<uint64_t> out;
    out.reserve(columns.size() * columns[0].size() * 4);
    for (const auto& col : columns) {
      if (col.size() != columns[0].size()) throw std::invalid_argument(std::string(what) + ": the columns differ in length");
      for (const auto& e : col) out.insert(out.end(), e.begin(), e.end());
    }
    return out;
  }
  blsgpu_fr_lookup* h_ = nullptr;
};
// Multilinear tables (include/bls12_381_hip.h): k tables of t.size() / k = 2^m scalars each, laid end to end; entry i is the value at the
// point whose coordinate x_b is bit b of i.  fr_mle_fold binds the top variable at r (k x 2^(m-1) out), fr_eq_table is
// eq(point)[i] = prod_b (bit b of i ? point[b] : 1 - point[b]), fr_mle_eval gives f_j(point) with point[b] the value of x_b.
inline int fr_mle_log(size_t n, const char* what) {
  if (n == 0 || (n & (n - 1))) throw std::invalid_argument(std::string(what) + ": the table length must be a power of two");
  int m = 0; while (((size_t)1 << m) < n) m++;
  return m;
}
inline std::vector<FrLimbs> fr_mle_fold(const std::vector<FrLimbs>& t, size_t k, const FrLimbs& r) {
  if (t.empty()) return {};
  if (k == 0 || t.size() % k) throw std::invalid_argument("fr_mle_fold: the length must be k tables of equal size");
  const int m = fr_mle_log(t.size() / k, "fr_mle_fold");
  std::vector<FrLimbs> out(t.size() / 2);
  check(blsgpu_fr_mle_fold(Context::instance().handle(), t[0].data(), m, k, r.data(), out.empty() ? nullptr : out[0].data()), "fr_mle_fold");
  return out;
}
inline std::vector<FrLimbs> fr_eq_table(const std::vector<FrLimbs>& point) {
  std::vector<FrLimbs> out((size_t)1 << point.size());
  check(blsgpu_fr_eq_table(Context::instance().handle(), point.empty() ? nullptr : point[0].data(), (int)point.size(), out[0].data()), "fr_eq_table");
  return out;
}
inline std::vector<FrLimbs> fr_mle_eval(const std::vector<FrLimbs>& t, size_t k, const std::vector<FrLimbs>& point) {
  std::vector<FrLimbs> out(k);
  if (k == 0) return out;
  if (t.empty() || t.size() % k || fr_mle_log(t.size() / k, "fr_mle_eval") != (int)point.size()) throw std::invalid_argument("fr_mle_eval: k tables of 2^point.size() scalars");
  check(blsgpu_fr_mle_eval(Context::instance().handle(), t[0].data(), (int)point.size(), k, point.empty() ? nullptr : point[0].data(), out[0].data()), "fr_mle_eval");
  return out;
}
// One term of a sumcheck's summand: coef * prod_e f_{tables[e]} (1 to 6 factors; an index may repeat)
struct FrTerm { FrLimbs coef; std::vector<uint8_t> tables; };
// A sumcheck over sum_x sum_t coef_t prod_e f_e(x) as a resident handle (blsgpu_fr_sumcheck): the k tables are copied to the device
// and consumed by the rounds.  round() gives the round polynomial's values at 0 .. degree(); order: round(), round(&r_1), ... while
// vars_left() > 1, then finish(r_m), which returns f_j at the point p_b = r_(m-b).
class FrSumcheck {
 public:
  FrSumcheck(const std::vector<FrLimbs>& t, size_t k, const std::vector<FrTerm>& terms) : k_(k) {
    if (t.empty() || k == 0 || t.size() % k) throw std::invalid_argument("FrSumcheck: the length must be k tables of equal size");
    const int m = fr_mle_log(t.size() / k, "FrSumcheck");
    std::vector<uint32_t> ptr{0};
    std::vector<uint8_t> tab;
    std::vector<FrLimbs> coef;
    for (const FrTerm& term : terms) {
      tab.insert(tab.end(), term.tables.begin(), term.tables.end());
      ptr.push_back((uint32_t)tab.size());
      coef.push_back(term.coef);
    }
    check(blsgpu_fr_sumcheck_begin(Context::instance().handle(), t[0].data(), m, k, terms.size(), ptr.data(), tab.data(), coef.empty() ? nullptr : coef[0].data(), &s_), "fr_sumcheck_begin");
  }
  ~FrSumcheck() { blsgpu_fr_sumcheck_free(s_); }
  FrSumcheck(const FrSumcheck&) = delete;
  FrSumcheck& operator=(const FrSumcheck&) = delete;
  FrSumcheck(FrSumcheck&& o) noexcept : s_(o.s_), k_(o.k_) { o.s_ = nullptr; }
  int vars_left() const { return blsgpu_fr_sumcheck_vars_left(s_); }
  int degree() const { return blsgpu_fr_sumcheck_degree(s_); }
  std::vector<FrLimbs> round(const FrLimbs* r_prev = nullptr) {
    std::vector<FrLimbs> evals((size_t)degree() + 1);
    check(blsgpu_fr_sumcheck_round(Context::instance().handle(), s_, r_prev ? r_prev->data() : nullptr, evals[0].data()), "fr_sumcheck_round");
    return evals;
  }
  std::vector<FrLimbs> finish(const FrLimbs& r_last) {
    std::vector<FrLimbs> values(k_);
    check(blsgpu_fr_sumcheck_finish(Context::instance().handle(), s_, r_last.data(), values[0].data()), "fr_sumcheck_finish");
    return values;
  }
  blsgpu_fr_sumcheck* handle() const { return s_; }
 private:
  blsgpu_fr_sumcheck* s_ = nullptr;
  size_t k_ = 0;
};
// The same transform over group elements: k vectors of p.size() / k points each in one call, in place (vector i = elements
// [i n, (i+1) n)); Y[m] = sum_j [w^(jm)] P[j] with the w of fr_ntt, the inverse scaled by n^-1 (include/bls12_381_hip.h).  Every point
// must lie in the prime-order subgroup.  The overloads on affine points lift them (Z = 1, the identity (0 : 1 : 0)) and return the result.
template <int G> void g_ntt_many(std::vector<Projective<G>>& p, size_t k, bool inverse = false) {
  if (k == 0 && p.empty()) return;
  if (k == 0 || p.empty() || p.size() % k) throw std::invalid_argument("g_ntt_many: the length must be k vectors of equal size");
  const size_t n = p.size() / k;
  if (n & (n - 1)) throw std::invalid_argument("g_ntt_many: the vector length must be a power of two");
  int log_n = 0; while (((size_t)1 << log_n) < n) log_n++;
  constexpr int W = Projective<G>::W;
  std::vector<uint64_t> xyz(p.size() * W);
  for (size_t i = 0; i < p.size(); i++) std::memcpy(xyz.data() + i * W, p[i].xyz.data(), W * 8);
  check((G == 1 ? blsgpu_g1_ntt_many : blsgpu_g2_ntt_many)(Context::instance().handle(), xyz.data(), log_n, k, inverse ? 1 : 0), "g_ntt_many");
  for (size_t i = 0; i < p.size(); i++) std::memcpy(p[i].xyz.data(), xyz.data() + i * W, W * 8);
}
template <int G> std::vector<Projective<G>> g_ntt_many(const std::vector<Affine<G>>& a, size_t k, bool inverse = false) {
  std::vector<Projective<G>> p(a.size());
  for (size_t i = 0; i < a.size(); i++) {
    if (a[i].infinity) { p[i] = Projective<G>::identity(); continue; }
    std::memcpy(p[i].xyz.data(), a[i].xy.data(), Affine<G>::W * 8);
    std::memcpy(p[i].xyz.data() + 2 * Projective<G>::W / 3, detail::kOne, 48);
  }
  g_ntt_many<G>(p, k, inverse);
  return p;
}
inline void g1_ntt_many(std::vector<G1Projective>& p, size_t k, bool inverse = false) { g_ntt_many<1>(p, k, inverse); }
inline void g2_ntt_many(std::vector<G2Projective>& p, size_t k, bool inverse = false) { g_ntt_many<2>(p, k, inverse); }
inline std::vector<G1Projective> g1_ntt_many(const std::vector<G1Affine>& a, size_t k, bool inverse = false) { return g_ntt_many<1>(a, k, inverse); }
inline std::vector<G2Projective> g2_ntt_many(const std::vector<G2Affine>& a, size_t k, bool inverse = false) { return g_ntt_many<2>(a, k, inverse); }

// Amortised KZG openings (include/bls12_381_hip.h: blsgpu_kzg_multiproof_*): all 2c = 2n / l cell proofs of many polynomials in one call.
// The constructor uploads the first n = 2^log_n points of `srs` (S[m] meant as [tau^m] G1), builds the handle's own resident tables
// and lets the upload go; proofs() takes count polynomials of n scalars laid end to end -- coefficients, or (form = BLSGPU_KZG_FORM_EVALS)
// values on the domain of fr_bary_* in `order` -- and returns count x 2c points numbered by `order`.  kzg_cells gives the cells.
class KzgMultiproof {
 public:
  KzgMultiproof(const std::vector<G1Affine>& srs, int log_n, int log_l) {
    if (log_n < 0 || log_n > 23 || srs.size() < ((size_t)1 << log_n)) throw std::invalid_argument("KzgMultiproof: the SRS holds fewer than 2^log_n points");
    const size_t n = (size_t)1 << log_n;
    std::vector<uint64_t> xy(n * G1Affine::W);
    std::vector<uint8_t> inf(n);
    for (size_t i = 0; i < n; i++) { std::memcpy(xy.data() + i * G1Affine::W, srs[i].xy.data(), G1Affine::W * 8); inf[i] = srs[i].infinity ? 1 : 0; }
    blsgpu_bases* b = nullptr;
    check(blsgpu_g1_bases_upload(Context::instance().handle(), xy.data(), inf.data(), n, &b), "g1_bases_upload");
    const int rc = blsgpu_kzg_multiproof_create(Context::instance().handle(), b, log_n, log_l, &h_);
    blsgpu_bases_free(b);
    check(rc, "kzg_multiproof_create");
  }
  ~KzgMultiproof() { blsgpu_kzg_multiproof_free(h_); }
  KzgMultiproof(const KzgMultiproof&) = delete;
  KzgMultiproof& operator=(const KzgMultiproof&) = delete;
  KzgMultiproof(KzgMultiproof&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  int log_n() const { return blsgpu_kzg_multiproof_log_n(h_); }
  int log_l() const { return blsgpu_kzg_multiproof_log_l(h_); }
  size_t cells() const { return blsgpu_kzg_multiproof_cells(h_); }
  const blsgpu_kzg_multiproof* handle() const { return h_; }
  std::vector<G1Projective> proofs(const std::vector<FrLimbs>& polys, int form = BLSGPU_KZG_FORM_COEFFS, int order = BLSGPU_FR_ORDER_NATURAL) const {
    const size_t n = (size_t)1 << log_n();
    if (polys.size() % n) throw std::invalid_argument("KzgMultiproof::proofs: the length must be polynomials of 2^log_n scalars");
    const size_t count = polys.size() / n;
    std::vector<G1Projective> out(count * cells());
    if (!count) return out;
    std::vector<uint64_t> xyz(out.size() * G1Projective::W);
    check(blsgpu_kzg_multiproof_proofs(Context::instance().handle(), h_, polys[0].data(), count, form, order, xyz.data()), "kzg_multiproof_proofs");
    for (size_t i = 0; i < out.size(); i++) std::memcpy(out[i].xyz.data(), xyz.data() + i * G1Projective::W, G1Projective::W * 8);
    return out;
  }
 private:
  blsgpu_kzg_multiproof* h_ = nullptr;
};
// cells[v][i][t] of count = polys.size() / 2^log_n polynomials: count x 2c x l scalars laid end to end
inline std::vector<FrLimbs> kzg_cells(const std::vector<FrLimbs>& polys, int log_n, int log_l, int form = BLSGPU_KZG_FORM_COEFFS, int order = BLSGPU_FR_ORDER_NATURAL) {
  if (log_n < 0 || log_n > 27 || polys.size() % ((size_t)1 << log_n)) throw std::invalid_argument("kzg_cells: the length must be polynomials of 2^log_n scalars");
  const size_t count = polys.size() >> log_n;
  std::vector<FrLimbs> out(polys.size() * 2);
  if (!count) return out;
  check(blsgpu_kzg_cells(Context::instance().handle(), polys[0].data(), log_n, log_l, count, form, order, out[0].data()), "kzg_cells");
  return out;
}

// Batched verification of KZG cell proofs (include/bls12_381_hip.h: blsgpu_kzg_cell_verifier_*, blsgpu_kzg_verify_cells): every batch of
// (commitment, cell index, cell, proof) tuples decided by one two-term pairing product.  The constructor uploads the first l = 2^log_l
// points of `srs`, builds the handle (S[0..l), the `G2Prepared` table {q, -G2}, the powers of w) and lets the upload go; q is meant as
// [tau^l] G2 and the caller vouches that it is in the subgroup.  verify() takes m cells of l scalars laid end to end, numbered by `order` as
// kzg_cells writes them, with row[k] / col[k] naming the commitment and the cell number; offsets is the CSR array of the batches and r
// holds one challenge per batch -- the caller's, unpredictable from the inputs.  Returns the verdict bytes; `out_ab`, if given, receives
// (A_s, B_s) per batch.
class KzgCellVerifier {
 public:
  KzgCellVerifier(const std::vector<G1Affine>& srs, int log_n, int log_l, const G2Affine& q) {
    if (log_l < 0 || log_l > 12 || srs.size() < ((size_t)1 << log_l)) throw std::invalid_argument("KzgCellVerifier: the SRS holds fewer than 2^log_l points");
    const size_t l = (size_t)1 << log_l;
    std::vector<uint64_t> xy(l * G1Affine::W);
    std::vector<uint8_t> inf(l);
    for (size_t i = 0; i < l; i++) { std::memcpy(xy.data() + i * G1Affine::W, srs[i].xy.data(), G1Affine::W * 8); inf[i] = srs[i].infinity ? 1 : 0; }
    blsgpu_bases* b = nullptr;
    check(blsgpu_g1_bases_upload(Context::instance().handle(), xy.data(), inf.data(), l, &b), "g1_bases_upload");
    const uint8_t q_inf = q.infinity ? 1 : 0;
    const int rc = blsgpu_kzg_cell_verifier_create(Context::instance().handle(), b, log_n, log_l, q.xy.data(), &q_inf, &h_);
    blsgpu_bases_free(b);
    check(rc, "kzg_cell_verifier_create");
  }
  ~KzgCellVerifier() { blsgpu_kzg_cell_verifier_free(h_); }
  KzgCellVerifier(const KzgCellVerifier&) = delete;
  KzgCellVerifier& operator=(const KzgCellVerifier&) = delete;
  KzgCellVerifier(KzgCellVerifier&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  int log_n() const { return blsgpu_kzg_cell_verifier_log_n(h_); }
  int log_l() const { return blsgpu_kzg_cell_verifier_log_l(h_); }
  size_t cells() const { return blsgpu_kzg_cell_verifier_cells(h_); }
  const blsgpu_kzg_cell_verifier* handle() const { return h_; }
  std::vector<uint8_t> verify(const std::vector<G1Affine>& commitments, const std::vector<uint32_t>& row, const std::vector<uint32_t>& col, const std::vector<FrLimbs>& cell_values,
                              const std::vector<G1Affine>& proofs, const std::vector<uint32_t>& offsets, const std::vector<FrLimbs>& r, int order = BLSGPU_FR_ORDER_NATURAL,
                              std::vector<G1Projective>* out_ab = nullptr) const {
    const size_t nseg = offsets.empty() ? 0 : offsets.size() - 1, m = nseg ? offsets.back() : 0, l = (size_t)1 << log_l();
    if (row.size() != m || col.size() != m || proofs.size() != m || cell_values.size() != m * l || r.size() != nseg)
      throw std::invalid_argument("KzgCellVerifier::verify: row, col, proofs and cells must hold offsets.back() cells, r one challenge per batch");
    std::vector<uint8_t> verdict(nseg);
    if (!nseg) return verdict;
    auto wire = [](const std::vector<G1Affine>& p, std::vector<uint64_t>& xy, std::vector<uint8_t>& inf) {
      xy.resize(p.size() * G1Affine::W + 1); inf.resize(p.size() + 1);
      for (size_t i = 0; i < p.size(); i++) { std::memcpy(xy.data() + i * G1Affine::W, p[i].xy.data(), G1Affine::W * 8); inf[i] = p[i].infinity ? 1 : 0; }
    };
    std::vector<uint64_t> cxy, pxy, ab(out_ab ? nseg * 2 * G1Projective::W : 0);
    std::vector<uint8_t> cinf, pinf;
    wire(commitments, cxy, cinf); wire(proofs, pxy, pinf);
    check(blsgpu_kzg_verify_cells(Context::instance().handle(), h_, cxy.data(), cinf.data(), commitments.size(), row.data(), col.data(), m ? cell_values[0].data() : nullptr, pxy.data(),
                                  pinf.data(), offsets.data(), nseg, r[0].data(), order, verdict.data(), out_ab ? ab.data() : nullptr), "kzg_verify_cells");
    if (out_ab) {
      out_ab->assign(nseg * 2, G1Projective());
      for (size_t i = 0; i < out_ab->size(); i++) std::memcpy((*out_ab)[i].xyz.data(), ab.data() + i * G1Projective::W, G1Projective::W * 8);
    }
    return verdict;
  }
 private:
  blsgpu_kzg_cell_verifier* h_ = nullptr;
};

// The same operations sharded over several GPUs of one node from this process (blsgpu_group: one context + one host thread per
// listed device; partial results folded with `Sum` / `MillerLoopResult + MillerLoopResult`, src/g1.rs:161-171, src/pairings.rs:179-186)
class Group {
 public:
  explicit Group(const std::vector<int>& devices) { check(blsgpu_group_create(devices.data(), (int)devices.size(), &h_), "blsgpu_group_create"); }
  ~Group() { blsgpu_group_destroy(h_); }
  Group(const Group&) = delete;
  Group& operator=(const Group&) = delete;
  blsgpu_group* handle() const { return h_; }
  int size() const { return blsgpu_group_size(h_); }
  // sum_i scalars[i] * bases[i] with bases and scalars dealt to the members in contiguous slices
  template <int G> Projective<G> msm(const std::vector<Affine<G>>& bases, const std::vector<Scalar>& scalars) const {
    if (bases.size() != scalars.size()) throw std::invalid_argument("msm: length mismatch");
    const size_t n = bases.size();
    std::vector<uint64_t> xy(n * Affine<G>::W + 1); std::vector<uint8_t> inf(n + 1), sb(n * 32 + 1);
    for (size_t i = 0; i < n; i++) { std::memcpy(xy.data() + i * Affine<G>::W, bases[i].xy.data(), Affine<G>::W * 8); inf[i] = bases[i].infinity; std::memcpy(sb.data() + 32 * i, scalars[i].bytes.data(), 32); }
    blsgpu_group_bases* b = nullptr;
    check(blsgpu_group_bases_upload(h_, G, xy.data(), inf.data(), n, &b), "group_bases_upload");
    Projective<G> r;
    int rc = G == 1 ? blsgpu_g1_msm_sharded(h_, b, sb.data(), n, r.xyz.data()) : blsgpu_g2_msm_sharded(h_, b, sb.data(), n, r.xyz.data());
    blsgpu_group_bases_free(b);
    check(rc, "msm_sharded");
    return r;
  }
  // multi_miller_loop(terms).final_exponentiation() with the terms dealt to the members and ONE final exponentiation
  Gt multi_miller_loop_final_exp(const std::vector<std::pair<G1Affine, G2Prepared>>& terms) const {
    const size_t n = terms.size();
    std::vector<uint64_t> a(n * 12 + 1), b(n * 24 + 1); std::vector<uint8_t> fa(n + 1), fb(n + 1);
    for (size_t i = 0; i < n; i++) {
      std::memcpy(a.data() + 12 * i, terms[i].first.xy.data(), 96); std::memcpy(b.data() + 24 * i, terms[i].second.q.xy.data(), 192);
      fa[i] = terms[i].first.infinity; fb[i] = terms[i].second.q.infinity;
    }
    Gt g;
    check(blsgpu_multi_miller_loop_sharded(h_, a.data(), fa.data(), b.data(), fb.data(), n, 1, g.f.data()), "multi_miller_loop_sharded");
    return g;
  }
  std::vector<Gt> pairing_batch(const std::vector<G1Affine>& p, const std::vector<G2Affine>& q) const {
    if (p.size() != q.size()) throw std::invalid_argument("pairing_batch: length mismatch");
    const size_t n = p.size(); std::vector<Gt> out(n);
    if (!n) return out;
    std::vector<uint64_t> a(n * 12), b(n * 24), o(n * 72); std::vector<uint8_t> fa(n), fb(n);
    for (size_t i = 0; i < n; i++) { std::memcpy(a.data() + 12 * i, p[i].xy.data(), 96); std::memcpy(b.data() + 24 * i, q[i].xy.data(), 192); fa[i] = p[i].infinity; fb[i] = q[i].infinity; }
    check(blsgpu_pairing_batch_sharded(h_, a.data(), fa.data(), b.data(), fb.data(), n, o.data()), "pairing_batch_sharded");
    for (size_t i = 0; i < n; i++) std::memcpy(out[i].f.data(), o.data() + 72 * i, 576);
    return out;
  }
 private:
  blsgpu_group* h_ = nullptr;
};

struct Bls12 {                                              // `pairing::Engine` / `MultiMillerLoop`, src/pairings.rs:790-824
  static Gt pairing(const G1Affine& p, const G2Affine& q) { return bls::pairing(p, q); }
  static MillerLoopResult multi_miller_loop(const std::vector<std::pair<G1Affine, G2Prepared>>& t) { return bls::multi_miller_loop(t); }
};

}  // namespace bls
