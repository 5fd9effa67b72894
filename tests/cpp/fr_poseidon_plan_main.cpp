// tests/cpp/fr_poseidon_plan_main.cpp -- csrc/fr_poseidon_plan.h on its own (a stand-alone host program, built with
// -fsanitize=address,undefined by tests/test_fr_poseidon_plan.py): the host Fr arithmetic, the sparse derivation against the textbook
// rounds for seeded parameters of every width, the singular case, every refused argument of the validation and of the launch plans.
// Prints one line per check and exits non-zero at the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fr_poseidon_plan.h"

using namespace bls;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint64_t next64() {                          // SplitMix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static FrpFe rand_fe() {
  for (;;) {
    FrpFe a{{next64(), next64(), next64(), next64() >> 1}};
    if (frp_below_r(a.v)) return a;
  }
}
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void flatten(const std::vector<FrpFe>& v, std::vector<uint64_t>* out) {
  out->clear();
  for (const FrpFe& a : v) for (int w = 0; w < 4; w++) out->push_back(a.v[w]);
}
// a Cauchy matrix 1 / (x_i + y_j)
static std::vector<FrpFe> cauchy(int t) {
  std::vector<FrpFe> x(t), y(t), m((size_t)t * t);
  for (int i = 0; i < t; i++) { x[i] = rand_fe(); y[i] = rand_fe(); }
  for (int i = 0; i < t; i++) for (int j = 0; j < t; j++) m[(size_t)i * t + j] = frp_inv(frp_add(x[i], y[j]));
  return m;
}

static void test_arithmetic() {
  const FrpFe one = frp_one();
  CHECK(one.v[0] == 0x00000001fffffffeull && one.v[3] == 0x1824b159acc5056full, "2^256 mod r");
  for (int i = 0; i < 200; i++) {
    const FrpFe a = rand_fe(), b = rand_fe(), c = rand_fe();
    CHECK(frp_eq(frp_mul(a, one), a), "a * 1");
    CHECK(frp_eq(frp_mul(a, b), frp_mul(b, a)), "commutative");
    CHECK(frp_eq(frp_mul(frp_mul(a, b), c), frp_mul(a, frp_mul(b, c))), "associative");
    CHECK(frp_eq(frp_mul(a, frp_add(b, c)), frp_add(frp_mul(a, b), frp_mul(a, c))), "distributive");
    CHECK(frp_eq(frp_sub(frp_add(a, b), b), a), "a + b - b");
    CHECK(frp_is_zero(a) || frp_eq(frp_mul(a, frp_inv(a)), one), "a / a");
    CHECK(frp_eq(frp_scale(a, 5), frp_mul(a, frp_scale(one, 5))), "2^5 a");
  }
  FrpFe top{{FRP_R64[0] - 1, FRP_R64[1], FRP_R64[2], FRP_R64[3]}};      // r - 1 in Montgomery limbs = -R^-1 ... a value at the edge
  CHECK(frp_is_zero(frp_add(top, frp_neg(top))), "x + (-x) at the edge");
  CHECK(frp_eq(frp_mul(top, top), frp_mul(frp_neg(top), frp_neg(top))), "(-x)^2");
  printf("ok arithmetic\n");
}

static void test_forms() {
  const int widths[6] = {2, 3, 4, 5, 9, 12};
  const int rounds[5][2] = {{2, 0}, {2, 1}, {4, 3}, {8, 5}, {8, 57}};
  for (int wi = 0; wi < 6; wi++)
    for (int ri = 0; ri < 5; ri++)
      for (int kind = 0; kind < 2; kind++) {         // a Cauchy matrix, a random matrix
        const int t = widths[wi], rf = rounds[ri][0], rp = rounds[ri][1];
        std::vector<FrpFe> rc((size_t)(rf + rp) * t), m = kind == 0 ? cauchy(t) : std::vector<FrpFe>((size_t)t * t);
        for (FrpFe& c : rc) c = rand_fe();
        if (kind == 1) for (FrpFe& e : m) e = rand_fe();
        std::vector<uint64_t> rcw, mw;
        flatten(rc, &rcw); flatten(m, &mw);
        FrPoseidonHost sp, de;
        std::string e1 = fr_poseidon_build(t, rf, rp, rcw.data(), mw.data(), FRP_FORM_AUTO, &sp);
        std::string e2 = fr_poseidon_build(t, rf, rp, rcw.data(), mw.data(), FRP_FORM_DENSE, &de);
        CHECK(e1.empty() && e2.empty(), "valid parameters refused: %s %s", e1.c_str(), e2.c_str());
        CHECK(sp.form == FRP_FORM_SPARSE && de.form == FRP_FORM_DENSE, "t=%d: forms %d %d", t, sp.form, de.form);
        const size_t T = (size_t)t;
        CHECK(sp.products == (size_t)rf * (3 * T + T * T) + (size_t)rp * (2 * T + 2) + (T - 1) * (T - 1), "sparse products");
        CHECK(de.products == (size_t)rf * (3 * T + T * T) + (size_t)rp * (3 + T * T), "dense products");
        CHECK(sp.image.size() == (size_t)FRP_ENTRY * ((size_t)rf * t + (size_t)rp * 2 * t + (T - 1) * (T - 1) + T * T), "sparse image size");
        CHECK(de.image.size() == (size_t)FRP_ENTRY * ((size_t)rf * t + (size_t)rp + 2 * T * T), "dense image size");
        for (uint32_t w : sp.image) CHECK(w < (1u << 29), "an image limb has more than 29 bits");
        for (int s = 0; s < 3; s++) {
          std::vector<FrpFe> a(t), b, c;
          for (FrpFe& x : a) x = s == 0 ? frp_zero() : rand_fe();
          b = a; c = a;
          frp_host_textbook(sp, &a);
          frp_host_sparse(sp, &b);
          for (int i = 0; i < t; i++) CHECK(frp_eq(a[i], b[i]), "t=%d rounds=(%d,%d) matrix %d: the sparse form differs from the textbook at element %d", t, rf, rp, kind, i);
          // the walk of the constants alone (what the dense kernels use): k_r on element 0, u into the second half
          const int h = rf / 2;
          for (int r = 0; r < h; r++) frp_host_full_round(de, de.rc.data() + (size_t)r * t, &c);
          for (int r = 0; r < rp; r++) {
            std::vector<FrpFe> x = c, y(t);
            x[0] = frp_pow5(frp_add(x[0], de.k[r]));
            for (int i = 0; i < t; i++) { FrpFe acc = frp_zero(); for (int j = 0; j < t; j++) acc = frp_add(acc, frp_mul(de.mds[(size_t)i * t + j], x[j])); y[i] = acc; }
            c = y;
          }
          for (int r = 0; r < h; r++) {
            std::vector<FrpFe> cc(de.rc.begin() + (size_t)(h + rp + r) * t, de.rc.begin() + (size_t)(h + rp + r + 1) * t);
            if (r == 0) for (int i = 0; i < t; i++) cc[i] = frp_add(cc[i], de.u[i]);
            frp_host_full_round(de, cc.data(), &c);
          }
          for (int i = 0; i < t; i++) CHECK(frp_eq(a[i], c[i]), "t=%d rounds=(%d,%d): the carried constants differ from the textbook at element %d", t, rf, rp, i);
        }
      }
  printf("ok forms\n");
}

static void test_singular() {
  for (int t : {2, 3, 4, 5, 9, 12}) {
    std::vector<FrpFe> m = cauchy(t), rc((size_t)7 * t);
    for (FrpFe& c : rc) c = rand_fe();
    if (t == 2) m[3] = frp_zero();
    else for (int j = 1; j < t; j++) m[(size_t)2 * t + j] = m[(size_t)1 * t + j];      // two equal rows in the lower-right block
    std::vector<uint64_t> rcw, mw;
    flatten(rc, &rcw); flatten(m, &mw);
    for (int rp : {0, 3}) {
      FrPoseidonHost p;
      std::string e = fr_poseidon_build(t, 4, rp, rcw.data(), mw.data(), FRP_FORM_AUTO, &p);
      CHECK(e.empty(), "singular block refused: %s", e.c_str());
      CHECK(p.form == FRP_FORM_DENSE, "t=%d r_partial=%d: AUTO must fall back to DENSE on a singular block", t, rp);
    }
  }
  printf("ok singular\n");
}

static void expect_refused(const char* what, const std::string& got, const char* needle) {
  CHECK(!got.empty() && strstr(got.c_str(), needle), "%s: expected a refusal naming '%s', got '%s'", what, needle, got.c_str());
}
static void test_refusals() {
  const int t = 3, rf = 4, rp = 3;
  std::vector<FrpFe> m = cauchy(t), rc((size_t)(rf + rp) * t);
  for (FrpFe& c : rc) c = rand_fe();
  std::vector<uint64_t> rcw, mw;
  flatten(rc, &rcw); flatten(m, &mw);
  rcw.resize(4 * 13 * (16 + 129), 0); mw.resize(4 * 13 * 13, 0);
  FrPoseidonHost p;
  for (int bad : {-1, 0, 1, 6, 7, 8, 10, 11, 13}) expect_refused("t", fr_poseidon_build(bad, rf, rp, rcw.data(), mw.data(), 0, &p), "t must be one of");
  for (int bad : {-2, 0, 1, 3, 15, 18}) expect_refused("r_full", fr_poseidon_build(t, bad, rp, rcw.data(), mw.data(), 0, &p), "r_full");
  for (int bad : {-1, 129}) expect_refused("r_partial", fr_poseidon_build(t, rf, bad, rcw.data(), mw.data(), 0, &p), "r_partial");
  for (int bad : {-1, 2, 3}) expect_refused("form", fr_poseidon_build(t, rf, rp, rcw.data(), mw.data(), bad, &p), "form");
  expect_refused("NULL constants", fr_poseidon_build(t, rf, rp, nullptr, mw.data(), 0, &p), "NULL round_constants");
  expect_refused("NULL mds", fr_poseidon_build(t, rf, rp, rcw.data(), nullptr, 0, &p), "NULL mds");
  expect_refused("NULL out", fr_poseidon_build(t, rf, rp, rcw.data(), mw.data(), 0, nullptr), "NULL out");
  std::vector<uint64_t> w = rcw;
  for (int i = 0; i < 4; i++) w[4 * 10 + i] = FRP_R64[i];                           // r itself
  expect_refused("constant = r", fr_poseidon_build(t, rf, rp, w.data(), mw.data(), 0, &p), "round_constants[10] (round 3, element 1)");
  w = rcw; w[4 * 20 + 3] = ~0ull;
  expect_refused("constant >= r", fr_poseidon_build(t, rf, rp, w.data(), mw.data(), 0, &p), "round_constants[20] (round 6, element 2)");
  w = mw; w[4 * 5 + 3] = FRP_R64[3] + 1;
  expect_refused("mds >= r", fr_poseidon_build(t, rf, rp, rcw.data(), w.data(), 0, &p), "mds[5] (row 1, column 2)");
  CHECK(fr_poseidon_build(t, rf, rp, rcw.data(), mw.data(), 0, &p).empty(), "the valid instance");
  // launch plans
  CHECK(fr_poseidon_many_plan(FRP_K_PERMUTE, 3, ((size_t)1 << 28) / 3 + 1).n_steps == -1, "n * t > 2^28");
  CHECK(fr_poseidon_many_plan(FRP_K_PERMUTE, 3, ((size_t)1 << 28) / 3).n_steps == 1, "n * t <= 2^28");
  CHECK(fr_poseidon_many_plan(FRP_K_HASH, 12, (size_t)-1 / 4).n_steps == -1, "n * t overflows 64 bits");
  CHECK(fr_poseidon_many_plan(FRP_K_HASH, 6, 1).n_steps == -1, "width outside the set");
  CHECK(fr_poseidon_many_plan(FRP_K_LEVEL, 3, 1).n_steps == -1, "not a kernel of this plan");
  CHECK(fr_poseidon_many_plan(FRP_K_HASH, 3, 0).n_steps == 0, "n == 0");
  CHECK(fr_poseidon_merkle_plan(3, -1, 1, true).n_steps == -1, "negative height");
  CHECK(fr_poseidon_merkle_plan(3, 29, 1, true).n_steps == -1, "2^29 leaves");
  CHECK(fr_poseidon_merkle_plan(3, 28, 1, true).n_steps > 0, "2^28 leaves");
  CHECK(fr_poseidon_merkle_plan(3, 28, 2, true).n_steps == -1, "2 x 2^28 leaves");
  CHECK(fr_poseidon_merkle_plan(12, 9, 1, true).n_steps == -1, "11^9 leaves");
  CHECK(fr_poseidon_merkle_plan(3, 10, (size_t)-1 / 8, true).n_steps == -1, "k * a^height overflows 64 bits");
  CHECK(fr_poseidon_merkle_plan(2, 28, ((size_t)1 << 28) / 28 + 1, true).n_steps == -1, "arity 1: k * height nodes");
  CHECK(fr_poseidon_merkle_plan(3, 10, 0, true).n_steps == 0, "k == 0");
  const FrPoseidonPlan a = fr_poseidon_merkle_plan(3, 10, 3, true), b = fr_poseidon_merkle_plan(3, 10, 3, false);
  CHECK(a.n_steps == 10 && b.n_steps == 10 && a.node_count == 3 * 1023 && a.leaves == 3 * 1024 && a.scratch == 0 && b.scratch == 3 * 1022, "height 10: one launch per level");
  size_t off = 0;
  for (int l = 0; l < 10; l++) {
    const size_t n = (size_t)3 << (9 - l);
    CHECK(a.step[l].kernel == FRP_K_LEVEL && a.step[l].items == n && a.step[l].grid == (n + 255) / 256 && a.step[l].dst == FRP_BUF_NODES && a.step[l].dst_off == off, "level %d with nodes", l + 1);
    CHECK(a.step[l].src == (l ? FRP_BUF_NODES : FRP_BUF_IN) && (l == 0 || a.step[l].src_off == a.step[l - 1].dst_off) && a.step[l].roots == (l == 9), "level %d reads the level below", l + 1);
    CHECK(b.step[l].dst == (l == 9 ? FRP_BUF_OUT : FRP_BUF_NODES) && b.step[l].dst_off == (l == 9 ? 0 : off) && b.step[l].src_off == a.step[l].src_off, "level %d without nodes", l + 1);
    off += n;
  }
  const FrPoseidonPlan c = fr_poseidon_merkle_plan(3, 6, 4096, false);
  CHECK(c.n_steps == 6 && c.step[0].grid == 512 && c.step[5].items == 4096 && c.scratch == 4096 * 62, "4096 trees of 64 leaves");
  const FrPoseidonPlan d = fr_poseidon_merkle_plan(3, 0, 5, true);
  CHECK(d.n_steps == 1 && d.step[0].kernel == FRP_K_COPY && d.node_count == 0, "height 0");
  printf("ok refusals\n");
}

int main() {
  test_arithmetic();
  test_forms();
  test_singular();
  test_refusals();
  printf("all ok\n");
  return 0;
}
