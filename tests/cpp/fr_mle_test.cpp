// Exercises fr_mle_fold, fr_eq_table, fr_mle_eval and FrSumcheck of include/bls12_381.hpp: the fold equals the host loop
// lo + r (hi - lo) over bls::fr_op, the evaluation equals the inner product with the eq table, and a whole sumcheck over
// eq * (a * b - c) passes the verifier's checks (evals[0] + evals[1] is the running claim, the next claim the interpolation at the
// challenge, the last one the summand at the final values), every step of them computed with bls::fr_op.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static FrLimbs mul(const FrLimbs& a, const FrLimbs& b) { return fr_op(FrOp::Mul, {a}, {b})[0]; }
static FrLimbs add(const FrLimbs& a, const FrLimbs& b) { return fr_op(FrOp::Add, {a}, {b})[0]; }
static FrLimbs sub(const FrLimbs& a, const FrLimbs& b) { return fr_op(FrOp::Sub, {a}, {b})[0]; }
int main() {
  const int m = 7;
  const size_t n = (size_t)1 << m, h = n / 2, k = 4;
  std::vector<FrLimbs> t(k * n), point(m);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  for (auto& e : t) next(e);
  for (auto& e : point) next(e);
  const FrLimbs zero{0, 0, 0, 0};
  const FrLimbs one = fr_eq_table({})[0];                          // m = 0: the Scalar one
  REQUIRE(mul(one, t[0]) == t[0]);
  // fold against lo + r (hi - lo), all tables in three fr_op calls
  const FrLimbs r = point[0];
  std::vector<FrLimbs> lo, hi, rs(k * h, r);
  for (size_t j = 0; j < k; j++) { lo.insert(lo.end(), t.begin() + j * n, t.begin() + j * n + h); hi.insert(hi.end(), t.begin() + j * n + h, t.begin() + (j + 1) * n); }
  REQUIRE(fr_mle_fold(t, k, r) == fr_op(FrOp::Add, lo, fr_op(FrOp::Mul, rs, fr_op(FrOp::Sub, hi, lo))));
  // evaluation against the eq inner product
  const auto eq = fr_eq_table(point);
  REQUIRE(eq.size() == n);
  const auto vals = fr_mle_eval(t, k, point);
  for (size_t j = 0; j < k; j++) {
    const std::vector<FrLimbs> row(t.begin() + j * n, t.begin() + (j + 1) * n);
    REQUIRE(fr_scan(FrScan::Sum, fr_op(FrOp::Mul, row, eq), 1)[n - 1] == vals[j]);
  }
  // a whole sumcheck over f0 * f1 * f2 - f0 * f3
  const FrLimbs minus_one = sub(zero, one);
  FrSumcheck sc(t, k, {FrTerm{one, {0, 1, 2}}, FrTerm{minus_one, {0, 3}}});
  REQUIRE(sc.vars_left() == m && sc.degree() == 3);
  // small integers and the inverses of the interpolation's denominators at the nodes 0 .. 3: 1 / -6, 1 / 2, 1 / -2, 1 / 6
  std::vector<FrLimbs> node(4);
  node[0] = zero; for (int i = 1; i < 4; i++) node[i] = add(node[i - 1], one);
  const FrLimbs six = add(node[3], node[3]);
  const std::vector<FrLimbs> den = fr_op(FrOp::Invert, {sub(zero, six), node[2], sub(zero, node[2]), six});
  FrLimbs claim = zero, challenge = zero;
  bool have = false;
  for (int round = 1; round <= m; round++) {
    const auto ev = round == 1 ? sc.round() : sc.round(&challenge);
    REQUIRE(ev.size() == 4);
    if (have) REQUIRE(add(ev[0], ev[1]) == claim);
    next(challenge);
    FrLimbs acc = zero;
    for (int i = 0; i < 4; i++) {
      FrLimbs term = mul(ev[i], den[i]);
      for (int u = 0; u < 4; u++) if (u != i) term = mul(term, sub(challenge, node[u]));
      acc = add(acc, term);
    }
    claim = acc; have = true;
    REQUIRE(sc.vars_left() == (round == 1 ? m : m - round + 1));
  }
  bool threw = false;
  try { sc.round(&challenge); } catch (const std::runtime_error&) { threw = true; }      // one variable is left
  REQUIRE(threw);
  const auto v = sc.finish(challenge);
  REQUIRE(sc.vars_left() == 0 && v.size() == k);
  REQUIRE(sub(mul(mul(v[0], v[1]), v[2]), mul(v[0], v[3])) == claim);
  threw = false;
  try { fr_mle_fold(std::vector<FrLimbs>(12), 2, r); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_mle ok\n");
  return 0;
}
