// Exercises FrMatrix / fr_spmv of include/bls12_381.hpp: every output of a matrix with short rows, empty rows and one row longer than a
// tile equals the host loop over bls::fr_op (one Mul call over all non-zeros, then additions row by row), for two right-hand sides.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const size_t n_rows = 40, n_cols = 33, k = 2;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 11; };
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<uint32_t> row_ptr{0}, col;
  for (size_t i = 0; i < n_rows; i++) {
    const size_t len = i == 17 ? 2 * 2048 + 7 : (i % 7 == 3 ? 0 : 1 + rnd() % 5);      // one row across three tiles, some empty rows
    for (size_t j = 0; j < len; j++) col.push_back((uint32_t)(rnd() % n_cols));
    row_ptr.push_back((uint32_t)col.size());
  }
  std::vector<FrLimbs> val(col.size()), x(k * n_cols);
  for (auto& e : val) next(e);
  for (auto& e : x) next(e);
  FrMatrix m(row_ptr, col, val, n_cols);
  REQUIRE(m.rows() == n_rows && m.cols() == n_cols && m.nnz() == col.size());
  const auto out = fr_spmv(m, x);
  REQUIRE(out.size() == k * n_rows);
  for (size_t v = 0; v < k; v++) {
    std::vector<FrLimbs> g(col.size());
    for (size_t p = 0; p < col.size(); p++) g[p] = x[v * n_cols + col[p]];
    const auto prod = fr_op(FrOp::Mul, val, g);
    for (size_t i = 0; i < n_rows; i++) {
      std::vector<FrLimbs> acc{FrLimbs({0, 0, 0, 0})};
      for (size_t p = row_ptr[i]; p < row_ptr[i + 1]; p++) acc = fr_op(FrOp::Add, acc, {prod[p]});
      REQUIRE(out[v * n_rows + i] == acc[0]);
    }
  }
  bool threw = false;
  try { FrMatrix bad(row_ptr, col, val, 5); } catch (const std::exception&) { threw = true; }      // a column index is not below n_cols
  REQUIRE(threw);
  threw = false;
  try { fr_spmv(m, std::vector<FrLimbs>(n_cols + 1)); } catch (const std::invalid_argument&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_spmv ok\n");
  return 0;
}
