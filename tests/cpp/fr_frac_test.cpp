// Exercises fr_grand_product and fr_frac_sum of include/bls12_381.hpp: both equal the composition of bls::fr_op, bls::fr_batch_invert
// and bls::fr_scan over the same columns, with a zero denominator among them, NULL (empty) sets and one aliased set.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const size_t c = 3, k = 2, n = 700, tot = k * n;                // rows that divide neither a lane chunk nor a tile, more than one tile
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<FrLimbs> na(c * tot), nb(c * tot), da(c * tot), db(c * tot);
  for (auto* v : {&na, &nb, &da, &db}) for (auto& e : *v) next(e);
  FrLimbs beta, gamma; next(beta); next(gamma);
  const std::vector<FrLimbs> B(tot, beta), G(tot, gamma);
  auto table = [&](const std::vector<FrLimbs>& set, size_t j) { return std::vector<FrLimbs>(set.begin() + j * tot, set.begin() + (j + 1) * tot); };
  auto factor = [&](const std::vector<FrLimbs>& a, const std::vector<FrLimbs>& b, size_t j) {
    auto t = b.empty() ? table(a, j) : fr_op(FrOp::Add, table(a, j), fr_op(FrOp::Mul, B, table(b, j)));
    return fr_op(FrOp::Add, t, G);
  };
  // a zero denominator: den_a = -(beta den_b + gamma) at element 5 of row 1, column 1
  {
    const size_t at = tot + n + 5;
    const auto v = fr_op(FrOp::Neg, fr_op(FrOp::Add, fr_op(FrOp::Mul, {beta}, {db[at]}), {gamma}));
    da[at] = v[0];
  }
  // the grand product, exclusive, with and without the beta terms
  for (int with_b = 1; with_b >= 0; with_b--) {
    const std::vector<FrLimbs> none;
    const auto& xb = with_b ? nb : none;
    const auto& yb = with_b ? db : none;
    std::vector<FrLimbs> num = factor(na, xb, 0), den = factor(da, yb, 0);
    for (size_t j = 1; j < c; j++) { num = fr_op(FrOp::Mul, num, factor(na, xb, j)); den = fr_op(FrOp::Mul, den, factor(da, yb, j)); }
    std::vector<uint8_t> want_flags, flags;
    const auto f = fr_op(FrOp::Mul, num, fr_batch_invert(den, &want_flags));
    const auto want = fr_scan(FrScan::Product, f, k, {}, true);
    const auto got = fr_grand_product(c, k, na, xb, da, yb, beta, gamma, true, &flags);
    REQUIRE(got == want && flags == want_flags);
    if (with_b) {
      REQUIRE(flags[n + 5] == 0 && got[n + 6] == FrLimbs({0, 0, 0, 0}) && got[n + 5] != FrLimbs({0, 0, 0, 0}) && got[tot - 1] == FrLimbs({0, 0, 0, 0}));
      size_t zeros = 0; for (auto b : flags) zeros += b == 0;
      REQUIRE(zeros == 1);
    }
  }
  // the fraction sum, inclusive, with multiplicities and without
  for (int with_m = 1; with_m >= 0; with_m--) {
    std::vector<FrLimbs> sum;
    std::vector<uint8_t> want_flags(tot, 1), fl, flags;
    for (size_t j = 0; j < c; j++) {
      auto term = fr_batch_invert(factor(da, db, j), &fl);
      if (with_m) term = fr_op(FrOp::Mul, table(na, j), term);
      sum = j ? fr_op(FrOp::Add, sum, term) : term;
      for (size_t i = 0; i < tot; i++) want_flags[i] &= fl[i];
    }
    const auto got = fr_frac_sum(c, k, with_m ? na : std::vector<FrLimbs>(), da, db, beta, gamma, false, &flags);
    REQUIRE(got == fr_scan(FrScan::Sum, sum, k) && flags == want_flags && flags[n + 5] == 0);
  }
  // num_a == den_a without beta terms: every factor cancels, the product is 1 everywhere (the Montgomery form of 1 = fr_op(x * x^-1))
  {
    const auto one = fr_op(FrOp::Mul, {beta}, fr_op(FrOp::Invert, {beta}))[0];
    const auto got = fr_grand_product(c, k, na, {}, na, {}, beta, gamma);
    for (const auto& e : got) REQUIRE(e == one);
  }
  bool threw = false;
  try { fr_grand_product(c, k, na, nb, std::vector<FrLimbs>(da.begin(), da.end() - 1), db, beta, gamma); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { fr_frac_sum(c, 11, {}, da, db, beta, gamma); } catch (const std::invalid_argument&) { threw = true; }      // 4200 scalars are not 33 rows
  REQUIRE(threw);
  std::printf("fr_frac ok\n");
  return 0;
}
