// Exercises fr_lagrange_segments and g{1,2}_lagrange_combine of include/bls12_381.hpp: y equals the host loop sum lambda_i v_i over
// bls::fr_op, the coefficients of distinct nodes sum to one, a point on a node gives that node's unit vector, a repeated node clears
// the flag; equal shares combine to the share itself and a point on a node picks that node's share, for G1 and G2.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<std::vector<FrLimbs>> nodes{std::vector<FrLimbs>(300), std::vector<FrLimbs>(5), {}, std::vector<FrLimbs>(1), std::vector<FrLimbs>(4)}, values = nodes;
  for (auto& seg : nodes) for (auto& e : seg) next(e);
  for (auto& seg : values) for (auto& e : seg) next(e);
  nodes[4][3] = nodes[4][0];                                      // a repeated node
  std::vector<FrLimbs> z(5);
  for (auto& e : z) next(e);
  z[1] = nodes[1][2];                                             // on a node
  const FrLagrange r = fr_lagrange_segments(nodes, z, values);
  const FrLimbs zero{0, 0, 0, 0}, one = r.lambda[3][0];           // one node: lambda = 1 for every z
  REQUIRE(r.distinct == std::vector<uint8_t>({1, 1, 1, 1, 0}) && r.lambda[2].empty() && r.y[2] == zero);
  REQUIRE(fr_op(FrOp::Mul, {one}, {one})[0] == one && one != zero);
  for (size_t k = 0; k < nodes.size(); k++) {
    REQUIRE(r.lambda[k].size() == nodes[k].size());
    std::vector<FrLimbs> acc{zero}, sum{zero};
    for (size_t i = 0; i < nodes[k].size(); i++) {
      acc = fr_op(FrOp::Add, acc, fr_op(FrOp::Mul, {r.lambda[k][i]}, {values[k][i]}));
      sum = fr_op(FrOp::Add, sum, {r.lambda[k][i]});
    }
    REQUIRE(acc[0] == r.y[k]);
    if (r.distinct[k] && !nodes[k].empty()) REQUIRE(sum[0] == one);
  }
  for (size_t i = 0; i < 5; i++) REQUIRE(r.lambda[1][i] == (i == 2 ? one : zero));
  REQUIRE(r.lambda[4][0] == zero && r.lambda[4][3] == zero && r.lambda[4][1] != zero);
  REQUIRE(fr_lagrange_segments(nodes).lambda[0] != r.lambda[0]);  // z = 0 is another point
  // the combines: five distinct shares [k] G, then five equal ones
  const std::vector<Scalar> ks{Scalar::from_u64(3), Scalar::from_u64(1000003), Scalar::from_u64(7), Scalar::from_u64(11), Scalar::from_u64(65537)};
  const std::vector<std::vector<FrLimbs>> two{nodes[1], nodes[1]};
  {
    const auto p = G1Projective::batch_normalize(mul_batch<1>(std::vector<G1Affine>(5, G1Affine::generator()), ks));
    std::vector<uint8_t> flags;
    const auto out = g1_lagrange_combine({p, std::vector<G1Affine>(5, p[4])}, two, {z[1], z[0]}, &flags);
    REQUIRE(out[0].to_affine() == p[2] && out[1].to_affine() == p[4] && flags == std::vector<uint8_t>({1, 1}));
  }
  {
    const auto p = G2Projective::batch_normalize(mul_batch<2>(std::vector<G2Affine>(5, G2Affine::generator()), ks));
    const auto out = g2_lagrange_combine({p, std::vector<G2Affine>(5, p[1])}, two, {z[1], z[0]});
    REQUIRE(out[0].to_affine() == p[2] && out[1].to_affine() == p[1]);
  }
  bool threw = false;
  try { fr_lagrange_segments(nodes, {z[0]}); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_lagrange ok\n");
  return 0;
}
