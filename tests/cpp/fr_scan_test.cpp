// Exercises fr_scan and fr_batch_invert of include/bls12_381.hpp: a HORNER row equals the host loop h = c[i] + z h over bls::fr_op,
// running sums and products equal their host loops, and a batch inversion equals fr_op(FrOp::Invert) with a zero among the inputs.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const size_t n = 300, k = 3;                                    // rows that divide neither a lane chunk nor a tile
  std::vector<FrLimbs> x(k * n), z(k);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  for (auto& e : x) next(e);
  for (auto& e : z) next(e);
  // HORNER: every row against the host loop, one fr_op call per step over the k rows at once
  const auto h = fr_scan(FrScan::Horner, x, k, z);
  std::vector<FrLimbs> acc(k), col(k);
  for (size_t v = 0; v < k; v++) acc[v] = x[v * n + n - 1];
  for (size_t v = 0; v < k; v++) REQUIRE(h[v * n + n - 1] == acc[v]);
  for (size_t i = n - 1; i-- > 0;) {
    for (size_t v = 0; v < k; v++) col[v] = x[v * n + i];
    acc = fr_op(FrOp::Add, col, fr_op(FrOp::Mul, z, acc));
    for (size_t v = 0; v < k; v++) REQUIRE(h[v * n + i] == acc[v]);
  }
  // running sums and products of the first row
  const std::vector<FrLimbs> row(x.begin(), x.begin() + n);
  const auto sums = fr_scan(FrScan::Sum, row, 1), prods = fr_scan(FrScan::Product, row, 1), ex = fr_scan(FrScan::Sum, row, 1, {}, true);
  std::vector<FrLimbs> a{row[0]}, p{row[0]};
  REQUIRE(ex[0] == FrLimbs({0, 0, 0, 0}));
  for (size_t i = 1; i < n; i++) {
    REQUIRE(ex[i] == a[0]);
    a = fr_op(FrOp::Add, a, {row[i]}); p = fr_op(FrOp::Mul, p, {row[i]});
    REQUIRE(sums[i] == a[0] && prods[i] == p[0]);
  }
  // batch inversion against op 4, a zero in the middle
  auto y = x; y[n + 7] = FrLimbs({0, 0, 0, 0});
  std::vector<uint8_t> flags;
  const auto inv = fr_batch_invert(y, &flags);
  REQUIRE(inv == fr_op(FrOp::Invert, y));
  for (size_t i = 0; i < y.size(); i++) REQUIRE(flags[i] == (i == n + 7 ? 0 : 1));
  REQUIRE(inv[n + 7] == FrLimbs({0, 0, 0, 0}));
  bool threw = false;
  try { fr_scan(FrScan::Horner, x, k); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_scan ok\n");
  return 0;
}
