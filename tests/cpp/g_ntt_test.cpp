// Exercises g1_ntt_many / g2_ntt_many of include/bls12_381.hpp (group transforms, k vectors in one call): inverse after forward is the
// identity on 4 x 2^6 G1 points and on 2^4 G2 points, the forward transform moves the points, the affine overload lifts and agrees with
// the projective one, and element 0 of a forward transform is the sum of the vector (w^0 = 1).
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
template <int G> static std::vector<Affine<G>> points(size_t n, uint64_t seed) {
  std::vector<Affine<G>> g(n, Affine<G>::generator());
  std::vector<Scalar> s(n);
  for (auto& e : s) {
    for (int i = 0; i < 32; i++) { seed = seed * 6364136223846793005ull + 1442695040888963407ull; e.bytes[i] = (uint8_t)(seed >> 56); }
    e.bytes[31] &= 0x3f;                                      // below r
  }
  return Projective<G>::batch_normalize(mul_batch<G>(g, s));
}
template <int G> static int round_trip(size_t k, size_t n, uint64_t seed) {
  auto a = points<G>(k * n, seed);
  a[1] = Affine<G>::identity();
  auto y = g_ntt_many<G>(a, k);                               // the affine overload
  auto ya = Projective<G>::batch_normalize(y);
  REQUIRE(!(ya[0] == a[0]) && !(ya[n - 1] == a[n - 1]));
  for (size_t v = 0; v < k; v++) {                            // Y[0] = sum_j P[j]
    std::vector<Projective<G>> vec;
    for (size_t j = 0; j < n; j++) vec.push_back(Projective<G>::identity() + a[v * n + j]);
    REQUIRE(Projective<G>::sum(vec).to_affine() == ya[v * n]);
  }
  std::vector<Projective<G>> p(a.size());                     // the projective overload on the same points agrees
  for (size_t i = 0; i < a.size(); i++) p[i] = Projective<G>::identity() + a[i];
  g_ntt_many<G>(p, k);
  REQUIRE(Projective<G>::batch_normalize(p) == ya);
  g_ntt_many<G>(y, k, true);
  REQUIRE(Projective<G>::batch_normalize(y) == a);
  return 0;
}
int main() {
  if (round_trip<1>(4, 64, 0x9E3779B97F4A7C15ull)) return 1;
  if (round_trip<2>(1, 16, 0xD1B54A32D192ED03ull)) return 1;
  { std::vector<G1Projective> p(4 * 64, G1Projective::generator()); auto q = p; g1_ntt_many(p, 4); g1_ntt_many(p, 4, true); REQUIRE(G1Projective::batch_normalize(p) == G1Projective::batch_normalize(q)); }
  bool threw = false;
  try { std::vector<G2Projective> bad(3 * 5, G2Projective::generator()); g2_ntt_many(bad, 3); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("g_ntt_many ok\n");
  return 0;
}
