// Exercises fr_ntt_many of include/bls12_381.hpp (k transforms in one call, optionally on a coset): k = 1 equals fr_ntt, every vector
// of a batch equals its own fr_ntt, and inverse(g) after forward(g) is the identity for g = GENERATOR = 7 (scalar.rs:99-105).
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const FrLimbs seven = {0x0000000efffffff1ull, 0x17e363d300189c0full, 0xff9c57876f8457b0ull, 0x351332208fc5a8c4ull};      // 7 R mod r
  const size_t n = 64, k = 5;
  std::vector<FrLimbs> x(k * n);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (auto& e : x) for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; }      // top limb < 2^62: below r
  // k = 1 equals fr_ntt
  std::vector<FrLimbs> one(x.begin(), x.begin() + n), ref = one;
  fr_ntt_many(one, 1); fr_ntt(ref);
  REQUIRE(one == ref);
  // every vector of the batch equals its own transform
  auto y = x; fr_ntt_many(y, k);
  for (size_t v = 0; v < k; v++) {
    std::vector<FrLimbs> a(x.begin() + v * n, x.begin() + (v + 1) * n); fr_ntt(a);
    REQUIRE(std::vector<FrLimbs>(y.begin() + v * n, y.begin() + (v + 1) * n) == a);
  }
  // coset round trip, and the coset values differ from the plain ones
  auto z = x; fr_ntt_many(z, k, false, &seven);
  REQUIRE(!(z == y));
  fr_ntt_many(z, k, true, &seven);
  REQUIRE(z == x);
  bool threw = false;
  try { std::vector<FrLimbs> bad(3 * 5); fr_ntt_many(bad, 3); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_ntt_many ok\n");
  return 0;
}
