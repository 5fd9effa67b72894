// tests/cpp/fr_expr_plan_main.cpp -- csrc/fr_expr_plan.h on its own: a stand-alone program, built with -fsanitize=address,undefined
// -fno-sanitize-recover by tests/test_fr_expr_plan.py and run directly.  It hands frx_prog_build one program per rule of
// include/bls12_381_hip.h (each must be refused with a text that names the instruction), a few thousand seeded random VALID programs
// at the limit sizes -- 256 instructions, 8 registers, 32 constants, 32 columns, rotations +-32767 -- each then broken in one place
// (refused at exactly that instruction), and sweeps the launch plan over log_n 0..28 x n_regs 1..8.  The code and constant arrays are
// heap blocks of exactly the size the arguments state, so a read past either is reported.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "fr_expr_plan.h"

using namespace bls;

static long checks = 0;
static std::string g_what;
#define REQUIRE(c) do { checks++; if (!(c)) { std::printf("FAILED: %s (line %d) %s\n", #c, __LINE__, g_what.c_str()); std::exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { uint64_t z = (g_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

static uint32_t REG(uint32_t i) { return i; }
static uint32_t COL(uint32_t j, int rot) { return 0x40000000u | (((uint32_t)rot & 0xffffu) << 8) | j; }
static uint32_t CONST(uint32_t i) { return 0x80000000u | i; }
static uint32_t INSTR(uint32_t op, uint32_t dst) { return op | (dst << 8); }

struct Prog {
  int n_cols = 1, n_regs = 1, n_consts = 0;
  std::vector<uint64_t> consts;
  std::vector<uint32_t> code;
  size_t n_instr() const { return code.size() / 3; }
  void add(uint32_t w0, uint32_t a, uint32_t b) { code.push_back(w0); code.push_back(a); code.push_back(b); }
};
// frx_prog_build on exact-size heap copies
static const char* build(const Prog& p, FrxProg* img, FrxInfo* info) {
  uint64_t* cs = p.consts.empty() ? nullptr : (uint64_t*)std::malloc(p.consts.size() * 8);
  uint32_t* cd = p.code.empty() ? nullptr : (uint32_t*)std::malloc(p.code.size() * 4);
  if (cs) std::memcpy(cs, p.consts.data(), p.consts.size() * 8);
  if (cd) std::memcpy(cd, p.code.data(), p.code.size() * 4);
  const char* r = frx_prog_build(p.n_cols, p.n_regs, p.n_consts, cs, p.n_instr(), cd, img, info);
  std::free(cs); std::free(cd);
  return r;
}
static void refused_at(const Prog& p, size_t instr, const char* rule) {
  g_what = rule;
  FrxProg* img = new FrxProg(); FrxInfo info;
  const char* r = build(p, img, &info);
  REQUIRE(r != nullptr);
  char want[48];
  std::snprintf(want, sizeof want, "instruction %zu:", instr);
  REQUIRE(std::strstr(r, want) != nullptr);
  REQUIRE(std::strlen(r) > std::strlen(want) + 12);            // ... and says which rule
  delete img;
}
static void refused(const Prog& p, const char* rule) {
  g_what = rule;
  const char* r = build(p, nullptr, nullptr);
  REQUIRE(r != nullptr && std::strlen(r) > 10);
}
static void accepted(const Prog& p, const char* what) {
  g_what = what;
  const char* r = build(p, nullptr, nullptr);
  if (r) g_what += std::string(": ") + r;
  REQUIRE(r == nullptr);
}

// a base program the single-rule cases start from: r0 = col0; r1 = r0 * const0; r1 += col1(+1) * r0
static Prog base() {
  Prog p; p.n_cols = 2; p.n_regs = 2; p.n_consts = 1; p.consts = {1, 0, 0, 0};
  p.add(INSTR(FRX_MOV, 0), COL(0, 0), 0);
  p.add(INSTR(FRX_MUL, 1), REG(0), CONST(0));
  p.add(INSTR(FRX_MAD, 1), COL(1, 1), REG(0));
  return p;
}

static void rules() {
  accepted(base(), "the base program");
  Prog p;
  // the counts
  for (int v : {0, -1, 33}) { p = base(); p.n_cols = v; refused(p, "n_cols out of range"); }
  for (int v : {0, -1, 9}) { p = base(); p.n_regs = v; refused(p, "n_regs out of range"); }
  for (int v : {-1, 33}) { p = base(); p.n_consts = v; refused(p, "n_consts out of range"); }
  p = base(); p.code.clear(); refused(p, "n_instr == 0");
  p = base(); while (p.n_instr() < 257) p.add(INSTR(FRX_MOV, 0), COL(0, 0), 0); refused(p, "n_instr == 257");
  p = base(); p.consts.clear(); refused(p, "consts NULL with n_consts > 0");
  p = base(); p.n_consts = 0; p.code[5] = REG(0); refused(p, "consts given with n_consts == 0");
  // a constant not below r: r itself, r + 1, 2^256 - 1; r - 1 is fine
  p = base(); p.consts = {FRX_R64[0], FRX_R64[1], FRX_R64[2], FRX_R64[3]}; refused(p, "constant == r");
  p = base(); p.consts = {FRX_R64[0] + 1, FRX_R64[1], FRX_R64[2], FRX_R64[3]}; refused(p, "constant == r + 1");
  p = base(); p.consts = {~0ull, ~0ull, ~0ull, ~0ull}; refused(p, "constant == 2^256 - 1");
  p = base(); p.consts = {FRX_R64[0] - 1, FRX_R64[1], FRX_R64[2], FRX_R64[3]}; accepted(p, "constant == r - 1");
  // per instruction: unknown op, unknown operand kind, indices out of range, stray bits, MOV's b, reads before writes
  p = base(); p.code[3] = INSTR(5, 1); refused_at(p, 1, "unknown op 5");
  p = base(); p.code[3] = INSTR(255, 1); refused_at(p, 1, "unknown op 255");
  p = base(); p.code[4] = 0xC0000000u; refused_at(p, 1, "operand kind 3 (a)");
  p = base(); p.code[8] = 0xC0000001u; refused_at(p, 2, "operand kind 3 (b)");
  p = base(); p.code[6] = INSTR(FRX_MAD, 2); refused_at(p, 2, "dst not below n_regs");
  p = base(); p.code[4] = REG(2); refused_at(p, 1, "register operand not below n_regs");
  p = base(); p.code[7] = COL(2, 0); refused_at(p, 2, "column not below n_cols");
  p = base(); p.code[5] = CONST(1); refused_at(p, 1, "constant not below n_consts");
  p = base(); p.code[3] |= 1u << 16; refused_at(p, 1, "stray bit in the instruction word");
  p = base(); p.code[3] |= 1u << 31; refused_at(p, 1, "stray top bit in the instruction word");
  p = base(); p.code[4] |= 1u << 8; refused_at(p, 1, "stray bit in a register operand");
  p = base(); p.code[4] |= 1u << 29; refused_at(p, 1, "stray bit 29 in a register operand");
  p = base(); p.code[7] |= 1u << 24; refused_at(p, 2, "stray bit in a column operand");
  p = base(); p.code[5] |= 1u << 8; refused_at(p, 1, "stray bit in a constant operand");
  p = base(); p.code[2] = REG(1); refused_at(p, 0, "MOV with b != 0 (a register word)");
  p = base(); p.code[2] = COL(0, 0); refused_at(p, 0, "MOV with b != 0 (a column word)");
  p = base(); p.code[1] = REG(0); refused_at(p, 0, "a register read by the first instruction");
  p = base(); p.code[4] = REG(1); refused_at(p, 1, "operand a read before written");
  p = base(); p.code[3] = INSTR(FRX_ADD, 1); p.code[5] = REG(1); refused_at(p, 1, "operand b read before written");
  p = base(); p.code[3] = INSTR(FRX_MAD, 1); refused_at(p, 1, "MAD's dst read before written");
  p = base(); p.code[0] = INSTR(FRX_MAD, 0); p.code[2] = COL(0, 0); refused_at(p, 0, "MAD as the first instruction");
  // MOV's b is not a read: word 0 there is not REG(0)
  p = base(); p.n_regs = 1; p.code.resize(3); accepted(p, "MOV alone");
  g_what = "NULL code";
  REQUIRE(frx_prog_build(1, 1, 0, nullptr, 1, nullptr, nullptr, nullptr) != nullptr);
  std::printf("rules\n");
}

// a random valid program of n instructions
static Prog random_valid(size_t n, int n_cols, int n_regs, int n_consts) {
  Prog p; p.n_cols = n_cols; p.n_regs = n_regs; p.n_consts = n_consts;
  for (int i = 0; i < n_consts; i++) {
    uint64_t c[4] = {rnd(), rnd(), rnd(), rnd() >> 2};             // below 2^254 < r ...
    if (below(8) == 0) { c[0] = FRX_R64[0] - 1; c[1] = FRX_R64[1]; c[2] = FRX_R64[2]; c[3] = FRX_R64[3]; }      // ... or r - 1
    for (int w = 0; w < 4; w++) p.consts.push_back(c[w]);
  }
  uint32_t written = 0;
  const auto operand = [&]() -> uint32_t {
    for (;;) {
      const uint32_t k = below(3);
      if (k == FRX_REG) { if (!written) continue; uint32_t r; do r = below(n_regs); while (!((written >> r) & 1u)); return REG(r); }
      if (k == FRX_COL) { const int rots[] = {0, 1, -1, 32767, -32767, -32768, (int)below(65536) - 32768}; return COL(below(n_cols), rots[below(7)]); }
      if (n_consts) return CONST(below(n_consts));
    }
  };
  for (size_t i = 0; i < n; i++) {
    uint32_t op = below(5), dst = below(n_regs);
    if (op == FRX_MAD && !((written >> dst) & 1u)) op = FRX_MUL;
    const uint32_t a = operand();
    p.add(INSTR(op, dst), a, op == FRX_MOV ? 0 : operand());
    written |= 1u << dst;
  }
  return p;
}

static void random_programs() {
  FrxProg* img = new FrxProg();
  for (int it = 0; it < 4000; it++) {
    const bool limit = it % 2 == 0;
    const int n_cols = limit ? FRX_MAX_COLS : 1 + (int)below(FRX_MAX_COLS), n_regs = limit ? FRX_MAX_REGS : 1 + (int)below(FRX_MAX_REGS);
    const int n_consts = limit ? FRX_MAX_CONSTS : (int)below(FRX_MAX_CONSTS + 1);
    const size_t n = limit ? FRX_MAX_INSTR : 1 + below(FRX_MAX_INSTR);
    const Prog p = random_valid(n, n_cols, n_regs, n_consts);
    g_what = "random valid program " + std::to_string(it);
    FrxInfo info;
    const char* r = build(p, img, &info);
    if (r) g_what += std::string(": ") + r;
    REQUIRE(r == nullptr);
    // the image is the header, the code as given, the constants as 32-bit words, zeros elsewhere; the figures are the program's
    REQUIRE(img->w[0] == n && img->w[1] == (uint32_t)n_regs && img->w[2] == (uint32_t)n_cols && img->w[3] == (uint32_t)n_consts);
    size_t products = 0; uint32_t cols_read = 0; int max_rot = 0;
    for (size_t i = 0; i < n; i++) {
      const uint32_t op = frx_op(p.code[3 * i]);
      if (op == FRX_MUL || op == FRX_MAD) products++;
      for (int s = 1; s <= (op == FRX_MOV ? 1 : 2); s++) {
        const uint32_t w = p.code[3 * i + s];
        if (frx_kind(w) == FRX_COL) { cols_read |= 1u << frx_index(w); const int m = std::abs(frx_rot(w)); if (m > max_rot) max_rot = m; }
      }
    }
    REQUIRE(info.products == products && info.cols_read == cols_read && info.max_rot == max_rot && info.n_instr == n);
    bool same = true;
    for (size_t i = 0; i < FRX_IMAGE_WORDS - (size_t)FRX_CODE_OFF; i++) {
      uint32_t want = 0;
      if (i < 3 * n) want = p.code[i];
      else if (i >= 3 * (size_t)FRX_MAX_INSTR && i - 3 * FRX_MAX_INSTR < 8 * (size_t)n_consts) { const size_t c = i - 3 * FRX_MAX_INSTR; want = (uint32_t)(p.consts[c / 2] >> (32 * (c % 2))); }
      same = same && img->w[FRX_CODE_OFF + i] == want;
    }
    REQUIRE(same);
    // the same program broken at one instruction is refused at exactly that instruction
    Prog q = p;
    const size_t at = below((uint32_t)n);
    switch (below(4)) {
      case 0: q.code[3 * at] = INSTR(5 + below(250), frx_dst(q.code[3 * at])); break;
      case 1: q.code[3 * at + 1] = 0xC0000000u | below(256); break;
      case 2: q.code[3 * at + 1] = COL(n_cols, 0); if (n_cols == 256) continue; break;
      default: q.code[3 * at] |= 1u << (16 + below(16)); break;
    }
    g_what = "broken program " + std::to_string(it);
    r = build(q, img, &info);
    REQUIRE(r != nullptr);
    char want[48];
    std::snprintf(want, sizeof want, "instruction %zu:", at);
    REQUIRE(std::strstr(r, want) != nullptr);
  }
  delete img;
  std::printf("programs\n");
}

static void plans() {
  for (int log_n = -2; log_n <= FRX_MAX_LOG_N + 2; log_n++)
    for (int n_regs = -1; n_regs <= FRX_MAX_REGS + 1; n_regs++) {
      g_what = "plan log_n=" + std::to_string(log_n) + " n_regs=" + std::to_string(n_regs);
      const bool want = log_n >= 0 && log_n <= FRX_MAX_LOG_N && n_regs >= 1 && n_regs <= FRX_MAX_REGS;
      const FrExprPlan p = fr_expr_plan(log_n, n_regs);
      REQUIRE(p.ok == (want ? 1 : 0));
      if (!want) { REQUIRE(p.grid == 0); continue; }
      const size_t n = (size_t)1 << log_n;
      REQUIRE(p.rows == n && p.block == (unsigned)FRX_BLOCK && p.chunk >= 1 && p.chunk <= (unsigned)FRX_CHUNK_MAX && p.tile == (size_t)p.block * p.chunk);
      REQUIRE(p.grid >= 1 && (size_t)p.grid * p.tile >= n && (size_t)(p.grid - 1) * p.tile < n);      // the grid covers N exactly
      REQUIRE(p.lds == (size_t)p.block * n_regs * 32 && p.lds <= FRX_LDS_CU && 2 * p.lds <= FRX_LDS_CU);
      // small shapes, as the emulation runs them
      for (int b : {64, 128, 256})
        for (int ch : {1, 2, 3, 7}) {
          FrxShape s; s.block = b; s.chunk = ch;
          const FrExprPlan q = fr_expr_plan(log_n, n_regs, s);
          REQUIRE(q.ok == 1 && (size_t)q.grid * q.tile >= n && (size_t)(q.grid - 1) * q.tile < n && q.lds == (size_t)b * n_regs * 32);
        }
    }
  g_what = "shapes the plan must refuse";
  for (int b : {0, 32, 96, 2048}) { FrxShape s; s.block = b; s.chunk = 1; REQUIRE(!fr_expr_plan(10, 1, s).ok); }
  for (int ch : {0, -1, 65}) { FrxShape s; s.block = 64; s.chunk = ch; REQUIRE(!fr_expr_plan(10, 1, s).ok); }
  { FrxShape s; s.block = 1024; s.chunk = 1; REQUIRE(fr_expr_plan(10, 5, s).ok && !fr_expr_plan(10, 6, s).ok); }      // 1024 lanes x 6 registers x 32 B > 160 KB
  std::printf("plans\n");
}

int main() {
  rules();
  random_programs();
  plans();
  std::printf("%ld checks\nall ok\n", checks);
  return 0;
}
