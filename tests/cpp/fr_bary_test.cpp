// Exercises fr_bary_eval and fr_bary_open of include/bls12_381.hpp against the coefficient-form route of the same header: inverse
// fr_ntt_many, fr_scan(Horner) -- whose row is p(z) followed by the quotient's coefficients --, forward fr_ntt_many.  Rows of 4096 values
// (longer than a tile) and of 64, a point of the domain among the points, both orders for the short rows.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static uint64_t s = 0x9E3779B97F4A7C15ull;
static void next(FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } }      // top limb < 2^62: below r
static size_t bitrev(size_t i, int bits) { size_t r = 0; for (int b = 0; b < bits; b++) if (i >> b & 1) r |= (size_t)1 << (bits - 1 - b); return r; }
// (y, q) of k natural-order rows by way of the coefficients
static FrOpening composed(std::vector<FrLimbs> f, size_t k, const std::vector<FrLimbs>& z) {
  const size_t n = f.size() / k;
  fr_ntt_many(f, k, true);
  auto h = fr_scan(FrScan::Horner, f, k, z);
  FrOpening o{std::vector<FrLimbs>(k), std::vector<FrLimbs>(f.size())};
  for (size_t v = 0; v < k; v++) {
    o.y[v] = h[v * n];
    for (size_t i = 0; i + 1 < n; i++) o.q[v * n + i] = h[v * n + i + 1];
    o.q[v * n + n - 1] = FrLimbs({0, 0, 0, 0});
  }
  fr_ntt_many(o.q, k, false);
  return o;
}
int main() {
  for (size_t n : {(size_t)4096, (size_t)64}) {
    const size_t k = 3;
    int log_n = 0; while (((size_t)1 << log_n) < n) log_n++;
    std::vector<FrLimbs> f(k * n), z(k);
    for (auto& e : f) next(e);
    for (auto& e : z) next(e);
    // z[1] = D[n - 3] = w^(n - 3): the transform of the unit vector at 1 is the domain itself
    std::vector<FrLimbs> a{f[0]}, d(n, FrLimbs({0, 0, 0, 0}));
    d[1] = fr_op(FrOp::Mul, a, fr_op(FrOp::Invert, a))[0];
    fr_ntt(d);
    z[1] = d[n - 3];
    const auto want = composed(f, k, z);
    const auto got = fr_bary_open(f, k, z);
    REQUIRE(got.y == want.y);
    REQUIRE(got.q == want.q);
    REQUIRE(got.y[1] == f[n + n - 3]);
    REQUIRE(fr_bary_eval(f, k, z) == want.y);
    // bit-reversed rows: the same polynomials, inputs and quotients permuted
    std::vector<FrLimbs> fr(k * n);
    for (size_t v = 0; v < k; v++) for (size_t i = 0; i < n; i++) fr[v * n + i] = f[v * n + bitrev(i, log_n)];
    const auto rev = fr_bary_open(fr, k, z, FrOrder::BitReversed);
    REQUIRE(rev.y == want.y);
    for (size_t v = 0; v < k; v++) for (size_t i = 0; i < n; i++) REQUIRE(rev.q[v * n + i] == want.q[v * n + bitrev(i, log_n)]);
  }
  bool threw = false;
  try { fr_bary_eval(std::vector<FrLimbs>(6), 2, std::vector<FrLimbs>(2)); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_bary ok\n");
  return 0;
}
