// Exercises bls::FrPoseidon of include/bls12_381.hpp: hash_many is element 1 of permute on (tag, x), both forms of an instance agree, and a
// Merkle tree (nodes and roots) equals the tree rebuilt level by level from hash_many calls.  The parameters are made up here (a Cauchy
// matrix over small integers, counted round constants): TEST parameters, as every instance is the caller's.
#include <cstdio>
#include <cstdlib>
#include "bls12_381.hpp"
using namespace bls;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
  const int t = 3, rf = 8, rp = 57;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&](FrLimbs& e) { for (int i = 0; i < 4; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; e[i] = i == 3 ? (s >> 2) : s; } };      // top limb < 2^62: below r
  std::vector<FrLimbs> rc((size_t)(rf + rp) * t), xy(2 * t), mds;
  for (auto& e : rc) next(e);
  for (auto& e : xy) next(e);
  // 1 / (x_i + y_j): sums, then one batch inversion
  std::vector<FrLimbs> xs, ys;
  for (int i = 0; i < t; i++) for (int j = 0; j < t; j++) { xs.push_back(xy[i]); ys.push_back(xy[t + j]); }
  mds = fr_batch_invert(fr_op(FrOp::Add, xs, ys));
  FrPoseidon sparse(t, rf, rp, rc, mds), dense(t, rf, rp, rc, mds, FrPoseidon::Form::Dense);
  REQUIRE(sparse.width() == t && sparse.rounds_full() == rf && sparse.rounds_partial() == rp);
  REQUIRE(sparse.form() == FrPoseidon::Form::Sparse && dense.form() == FrPoseidon::Form::Dense);
  REQUIRE(sparse.products_per_permutation() == 604 && dense.products_per_permutation() == 828);
  const size_t n = 300;
  FrLimbs tag; next(tag);
  std::vector<FrLimbs> pre(n * 2), states;
  for (auto& e : pre) next(e);
  for (size_t i = 0; i < n; i++) { states.push_back(tag); states.push_back(pre[2 * i]); states.push_back(pre[2 * i + 1]); }
  const auto pa = sparse.permute(states), pb = dense.permute(states);
  REQUIRE(pa == pb);
  const auto ha = sparse.hash_many(tag, pre), hb = dense.hash_many(tag, pre);
  REQUIRE(ha == hb && ha.size() == n);
  for (size_t i = 0; i < n; i++) REQUIRE(ha[i] == pa[3 * i + 1]);
  // k = 3 trees of 2^9 leaves: nine levels
  const int height = 9; const size_t k = 3;
  std::vector<FrLimbs> leaves(k << height), nodes;
  for (auto& e : leaves) next(e);
  const auto roots = sparse.merkle(tag, leaves, height, k, &nodes);
  REQUIRE(roots.size() == k && nodes.size() == k * 511);
  REQUIRE(dense.merkle(tag, leaves, height, k) == roots);
  std::vector<FrLimbs> cur = leaves, all;
  for (int l = 0; l < height; l++) { cur = sparse.hash_many(tag, cur); all.insert(all.end(), cur.begin(), cur.end()); }
  REQUIRE(cur == roots && all == nodes);
  REQUIRE(sparse.merkle(tag, roots, 0, k) == roots);
  bool threw = false;
  try { FrPoseidon bad(6, rf, rp, std::vector<FrLimbs>((size_t)(rf + rp) * 6), std::vector<FrLimbs>(36)); } catch (const std::exception&) { threw = true; }
  REQUIRE(threw);
  std::printf("fr_poseidon ok\n");
  return 0;
}
