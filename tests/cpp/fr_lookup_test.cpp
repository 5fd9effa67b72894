// Exercises FrLookup of include/bls12_381.hpp: a two-column table with a repeated row against a host loop over the same keys --
// multiplicities by the first-occurrence rule, indices, misses, the accessors, the negated column (m + (r - m) = 0 through bls::fr_op),
// an empty lookup, and the refusals.
#include <cstdio>
#include <cstdlib>
#include <map>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const size_t rows = 300, n = 2000;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<std::vector<FrLimbs>> t(2, std::vector<FrLimbs>(rows)), f(2, std::vector<FrLimbs>(n));
  for (auto& col : t) for (auto& e : col) next(e);
  for (size_t i = 10; i < rows; i += 10) { t[0][i] = t[0][i - 7]; t[1][i] = t[1][i - 7]; }       // every tenth row repeats an earlier one
  t[1][5] = t[1][4];                                                                               // rows 4 and 5 differ in column 0 only
  size_t want_missing = 0;
  for (size_t i = 0; i < n; i++) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const size_t j = (size_t)(s >> 33) % rows;
    f[0][i] = t[0][j]; f[1][i] = t[1][j];
    if (i % 50 == 49) { next(f[1][i]); want_missing++; }                                           // a fresh second column: a miss
  }
  std::map<std::array<uint64_t, 8>, size_t> first;
  auto key = [](const std::vector<std::vector<FrLimbs>>& v, size_t i) { std::array<uint64_t, 8> k; for (int j = 0; j < 2; j++) for (int w = 0; w < 4; w++) k[4 * j + w] = v[j][i][w]; return k; };
  for (size_t j = 0; j < rows; j++) first.emplace(key(t, j), j);
  std::vector<uint64_t> m(rows, 0);
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; i++) {
    const auto it = first.find(key(f, i));
    if (it == first.end()) { idx[i] = FrLookup::miss; continue; }
    idx[i] = (uint32_t)it->second; m[it->second]++;
  }
  const FrLookup lk(t);
  REQUIRE(lk.cols() == 2 && lk.rows() == rows && lk.distinct() == first.size() && lk.slots() == 1024);
  const auto got = lk.count(f);
  REQUIRE(got.missing == want_missing && got.index == idx && got.mult.size() == rows);
  // the multiplicities are Montgomery scalars: m[j] * 1 (fr_op Mul by the plain integer's limbs multiplies by R^-1) is checked through
  // the negated column instead: m + (r - m) = 0 for every row, and m[j] == 0 exactly where the host count is 0
  const auto neg = lk.count(f, true);
  const auto sum = fr_op(FrOp::Add, got.mult, neg.mult);
  const FrLimbs zero = {0, 0, 0, 0};
  for (size_t j = 0; j < rows; j++) {
    REQUIRE(sum[j] == zero);
    REQUIRE((got.mult[j] == zero) == (m[j] == 0));
    REQUIRE((neg.mult[j] == zero) == (m[j] == 0));
  }
  // one lookup of row 0's key counted twice: mult[0] of f = {k, k} is twice mult[0] of f = {k}
  {
    const auto one = lk.count({{t[0][0]}, {t[1][0]}}), two = lk.count({{t[0][0], t[0][0]}, {t[1][0], t[1][0]}});
    REQUIRE(fr_op(FrOp::Add, one.mult, one.mult) == two.mult && one.index[0] == 0 && two.missing == 0);
  }
  const auto none = lk.count(std::vector<std::vector<FrLimbs>>(2));
  REQUIRE(none.missing == 0 && none.index.empty() && none.mult == std::vector<FrLimbs>(rows, zero));
  bool threw = false;
  try { lk.count({f[0]}); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { const std::vector<std::vector<FrLimbs>> empty(1); FrLookup bad(empty); } catch (const std::exception&) { threw = true; }                      // rows = 0
  REQUIRE(threw);
  std::printf("fr_lookup ok\n");
  return 0;
}
