// Exercises FrExpr of include/bls12_381.hpp: a program with every op, a rotated column on a strided domain, a periodic column, a
// challenge column of length 1 and a constant equals the same expression composed from bls::fr_op on expanded host vectors; the
// accessors report the program; a bad program and bad columns throw.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const int log_n = 10, log_stride = 2;
  const size_t n = (size_t)1 << log_n;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<FrLimbs> a(n), b(n), per(4), chal(1), k(1);
  for (auto* v : {&a, &b, &per, &chal, &k}) for (auto& e : *v) next(e);
  // out = ((a * b(next row) + chal * a - k) * per) + b, with a MOV on the way; column 3 is never read
  FrExpr::Code code;
  code.mul(0, FrExpr::col(0), FrExpr::col(1, +1)).mad(0, FrExpr::col(4), FrExpr::col(0)).sub(0, FrExpr::reg(0), FrExpr::constant(0)).mov(1, FrExpr::col(2, -1));
  code.mul(0, FrExpr::reg(0), FrExpr::reg(1)).add(0, FrExpr::reg(0), FrExpr::col(1));
  const FrExpr e(5, 2, k, code);
  REQUIRE(e.cols() == 5 && e.regs() == 2 && e.instructions() == 6 && e.products_per_row() == 3 && e.cols_read() == 0x17);
  const auto got = e.eval({a, b, per, {}, chal}, log_n, log_stride, {(uint8_t)log_n, (uint8_t)log_n, 2, 0, 0});
  // the same from fr_op on expanded vectors
  std::vector<FrLimbs> b_next(n), per_x(n);
  for (size_t i = 0; i < n; i++) { b_next[i] = b[(i + 4) % n]; per_x[i] = per[(i + n - 4) % 4]; }
  const std::vector<FrLimbs> C(n, chal[0]), K(n, k[0]);
  auto want = fr_op(FrOp::Add, fr_op(FrOp::Mul, a, b_next), fr_op(FrOp::Mul, C, a));
  want = fr_op(FrOp::Add, fr_op(FrOp::Mul, fr_op(FrOp::Sub, want, K), per_x), b);
  REQUIRE(got.size() == n && got == want);
  // every column at full length with col_log_len left out: the same program over other data
  {
    std::vector<FrLimbs> p2(n), c2(n);
    for (size_t i = 0; i < n; i++) { p2[i] = per[i % 4]; c2[i] = chal[0]; }
    REQUIRE(e.eval({a, b, p2, {}, c2}, log_n, log_stride) == want);
  }
  bool threw = false;
  try { FrExpr::Code bad; bad.add(0, FrExpr::reg(0), FrExpr::col(0)); FrExpr x(1, 1, {}, bad); } catch (const std::exception& ex) { threw = std::string(ex.what()).find("instruction 0") != std::string::npos; }
  REQUIRE(threw);
  threw = false;
  try { e.eval({a, b, per, {}}, log_n, log_stride); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  threw = false;
  try { e.eval({a, b, per, {}, chal}, log_n, log_stride); } catch (const std::invalid_argument&) { threw = true; }      // per has 4 scalars, not N
  REQUIRE(threw);
  std::printf("fr_expr ok\n");
  return 0;
}
