// fr_expr_plan.h -- the Fr expression programs (blsgpu_fr_expr_*) as plain host code: the limits, the validation of a caller's program
// with the image the kernel reads (frx_prog_build), and the launch plan of an evaluation.  No HIP calls here: api_fr.hip builds the
// image once per handle and launches from the plan, tests/simt/emu_fr_expr.cpp walks the same plan on the host,
// tests/cpp/fr_expr_plan_main.cpp sweeps both under sanitizers.
//
// A program is straight-line code over a small register file, one instruction = three words {op | dst << 8, a, b}
// (include/bls12_381_hip.h).  It is validated ONCE, here: after frx_prog_build has accepted it the kernel decodes without a single
// check, every index is in range, and no register is read before an instruction of the same program wrote it -- so a row's result never
// depends on what the register file (LDS) held before.
//
// The launch.  One row per lane-step: a workgroup of `block` lanes takes a tile of block * chunk rows, lane l the rows
// base + e * block + l, so consecutive lanes sit on consecutive rows and a column read is two 16-byte loads per lane, coalesced apart
// from the wrap.  The register file is `n_regs` scalars per lane in LDS (block * n_regs * 32 bytes, reused by the lane's next row), so
// LDS -- not the tile -- is what the occupancy hangs on: 64 KB at eight registers, two workgroups per CU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace bls {

constexpr int FRX_MAX_COLS = 32, FRX_MAX_REGS = 8, FRX_MAX_CONSTS = 32, FRX_MAX_INSTR = 256;
constexpr int FRX_MAX_LOG_N = 28;
constexpr int FRX_BLOCK = 256;
constexpr int FRX_CHUNK_MAX = 4;                      // rows per lane of the shipped shapes
constexpr size_t FRX_LDS_CU = 160 * 1024;

enum FrxOp { FRX_ADD = 0, FRX_SUB = 1, FRX_MUL = 2, FRX_MAD = 3, FRX_MOV = 4 };
enum FrxKind { FRX_REG = 0, FRX_COL = 1, FRX_CONST = 2 };

// What the kernel reads, uploaded once per handle: a header, the code words as the caller gave them (validated: the format decodes with
// shifts and masks alone), the constants as eight 32-bit words each.
constexpr int FRX_HDR_WORDS = 4;                      // n_instr, n_regs, n_cols, n_consts
constexpr int FRX_CODE_OFF = FRX_HDR_WORDS;
constexpr int FRX_CONST_OFF = FRX_CODE_OFF + 3 * FRX_MAX_INSTR;
constexpr int FRX_IMAGE_WORDS = FRX_CONST_OFF + 8 * FRX_MAX_CONSTS;
static_assert(FRX_CONST_OFF % 4 == 0, "the constants are read as 16-byte words");
struct FrxProg { uint32_t w[FRX_IMAGE_WORDS]; };
static_assert(sizeof(FrxProg) == 4112, "the image: 16 bytes of header, 3 KB of code, 1 KB of constants");

// what the handle's accessors report
struct FrxInfo {
  int n_cols = 0, n_regs = 0, n_consts = 0;
  size_t n_instr = 0, products = 0;                   // products: MUL + MAD instructions
  uint32_t cols_read = 0;                             // bit j: some instruction reads column j
  int max_rot = 0;                                    // the largest |rotation| of a column operand
};

// the column pointers and lengths of one evaluation: a kernel argument (by value)
struct FrxCols {
  const uint32_t* p[FRX_MAX_COLS];
  uint32_t log_len[FRX_MAX_COLS];      // words, not bytes: the kernel reads them with scalar loads
};

// ---- the operand and instruction words ---------------------------------------------------------------------------------------
constexpr uint32_t frx_kind(uint32_t w) { return w >> 30; }
constexpr uint32_t frx_index(uint32_t w) { return w & 0xffu; }
constexpr int frx_rot(uint32_t w) { return (int)(int16_t)(uint16_t)(w >> 8); }      // bits 23..8 as a signed 16-bit integer
constexpr uint32_t frx_op(uint32_t w) { return w & 0xffu; }
constexpr uint32_t frx_dst(uint32_t w) { return (w >> 8) & 0xffu; }

constexpr uint64_t FRX_R64[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};      // scalar.rs:76-81
inline bool frx_below_r(const uint64_t* a) {
  for (int i = 3; i >= 0; i--) { if (a[i] < FRX_R64[i]) return true; if (a[i] > FRX_R64[i]) return false; }
  return false;
}

// Checks a program against the rules of include/bls12_381_hip.h and builds the kernel's image.  Returns NULL when it is valid, or the
// text that names the instruction and the rule it breaks (a buffer of the calling thread, good until its next call).
inline const char* frx_prog_build(int n_cols, int n_regs, int n_consts, const uint64_t* consts, size_t n_instr, const uint32_t* code, FrxProg* out, FrxInfo* info) {
  static thread_local char text[192];
  if (n_cols < 1 || n_cols > FRX_MAX_COLS) return "fr_expr: n_cols must be in [1, 32]";
  if (n_regs < 1 || n_regs > FRX_MAX_REGS) return "fr_expr: n_regs must be in [1, 8]";
  if (n_consts < 0 || n_consts > FRX_MAX_CONSTS) return "fr_expr: n_consts must be in [0, 32]";
  if (n_instr < 1 || n_instr > (size_t)FRX_MAX_INSTR) return "fr_expr: n_instr must be in [1, 256]";
  if (!code) return "fr_expr: NULL code";
  if ((n_consts != 0) != (consts != nullptr)) return "fr_expr: consts must be NULL exactly when n_consts is 0";
  for (int i = 0; i < n_consts; i++)
    if (!frx_below_r(consts + 4 * i)) { std::snprintf(text, sizeof text, "fr_expr: constant %d is not a canonical Scalar (limbs >= r)", i); return text; }
  FrxInfo f;
  f.n_cols = n_cols; f.n_regs = n_regs; f.n_consts = n_consts; f.n_instr = n_instr;
  uint32_t written = 0;                                // bit i: an earlier instruction wrote register i
  const char* why = nullptr;
  // an operand that is READ: kind, index, stray bits, and for a register that it has been written
  const auto operand = [&](uint32_t w, const char* name) -> bool {
    static thread_local char sub[96];
    const uint32_t kind = frx_kind(w), idx = frx_index(w);
    why = sub;
    switch (kind) {
      case FRX_REG:
        if (w & 0x3fffff00u) { std::snprintf(sub, sizeof sub, "operand %s has a stray bit (a register operand uses bits 7..0)", name); return false; }
        if (idx >= (uint32_t)n_regs) { std::snprintf(sub, sizeof sub, "operand %s names register %u, not below n_regs", name, idx); return false; }
        if (!((written >> idx) & 1u)) { std::snprintf(sub, sizeof sub, "operand %s reads register %u before any instruction wrote it", name, idx); return false; }
        return true;
      case FRX_COL:
        if (w & 0x3f000000u) { std::snprintf(sub, sizeof sub, "operand %s has a stray bit (a column operand uses bits 23..0)", name); return false; }
        if (idx >= (uint32_t)n_cols) { std::snprintf(sub, sizeof sub, "operand %s names column %u, not below n_cols", name, idx); return false; }
        f.cols_read |= 1u << idx;
        { const int r = frx_rot(w); const int m = r < 0 ? -r : r; if (m > f.max_rot) f.max_rot = m; }
        return true;
      case FRX_CONST:
        if (w & 0x3fffff00u) { std::snprintf(sub, sizeof sub, "operand %s has a stray bit (a constant operand uses bits 7..0)", name); return false; }
        if (idx >= (uint32_t)n_consts) { std::snprintf(sub, sizeof sub, "operand %s names constant %u, not below n_consts", name, idx); return false; }
        return true;
      default:
        std::snprintf(sub, sizeof sub, "operand %s has the unknown kind 3", name);
        return false;
    }
  };
  for (size_t i = 0; i < n_instr; i++) {
    const uint32_t w0 = code[3 * i], a = code[3 * i + 1], b = code[3 * i + 2];
    const uint32_t op = frx_op(w0), dst = frx_dst(w0);
    static thread_local char sub0[96];
    bool ok = true;
    if (w0 >> 16) { why = "the instruction word has a stray bit (op in bits 7..0, dst in bits 15..8)"; ok = false; }
    else if (op > (uint32_t)FRX_MOV) { std::snprintf(sub0, sizeof sub0, "unknown op %u", op); why = sub0; ok = false; }
    else if (dst >= (uint32_t)n_regs) { std::snprintf(sub0, sizeof sub0, "dst names register %u, not below n_regs", dst); why = sub0; ok = false; }
    else if (!operand(a, "a")) ok = false;
    else if (op == FRX_MOV) { if (b != 0) { why = "MOV takes one operand: b must be 0"; ok = false; } }
    else if (!operand(b, "b")) ok = false;
    if (ok && op == FRX_MAD && !((written >> dst) & 1u)) { std::snprintf(sub0, sizeof sub0, "MAD reads its dst, register %u, before any instruction wrote it", dst); why = sub0; ok = false; }
    if (!ok) { std::snprintf(text, sizeof text, "fr_expr: instruction %zu: %s", i, why); return text; }
    written |= 1u << dst;
    if (op == FRX_MUL || op == FRX_MAD) f.products++;
  }
  if (out) {
    FrxProg& p = *out;
    for (int i = 0; i < FRX_IMAGE_WORDS; i++) p.w[i] = 0;
    p.w[0] = (uint32_t)n_instr; p.w[1] = (uint32_t)n_regs; p.w[2] = (uint32_t)n_cols; p.w[3] = (uint32_t)n_consts;
    for (size_t i = 0; i < 3 * n_instr; i++) p.w[FRX_CODE_OFF + i] = code[i];
    for (int i = 0; i < 4 * n_consts; i++) { p.w[FRX_CONST_OFF + 2 * i] = (uint32_t)consts[i]; p.w[FRX_CONST_OFF + 2 * i + 1] = (uint32_t)(consts[i] >> 32); }
  }
  if (info) *info = f;
  return nullptr;
}

// ---- the launch plan -----------------------------------------------------------------------------------------------------------
struct FrxShape { int block = FRX_BLOCK, chunk = 1; };
// the register file: two planes of 16-byte halves per register, address ((reg * 2 + half) * block + lane) * 16
constexpr size_t frx_lds_bytes(int block, int n_regs) { return (size_t)block * n_regs * 32; }
static_assert(frx_lds_bytes(FRX_BLOCK, FRX_MAX_REGS) == 64 * 1024, "eight registers at the shipped block: the 64 KB a kernel gets unasked");
static_assert(2 * frx_lds_bytes(FRX_BLOCK, FRX_MAX_REGS) <= FRX_LDS_CU, "two workgroups of the shipped shape must fit a CU's LDS at every n_regs");
static_assert(frx_lds_bytes(FRX_BLOCK, 2) == 16 * 1024, "two registers: 16 KB");

// rows per lane: one while that still gives every CU its workgroups (up to 2^18 rows: 1024 of them), then up to four
inline FrxShape frx_shape(int log_n) {
  FrxShape s;
  s.chunk = log_n >= 20 ? FRX_CHUNK_MAX : log_n == 19 ? 2 : 1;
  return s;
}

struct FrExprPlan {
  int ok = 0;                  // 0: refused (log_n, n_regs or the shape out of range)
  unsigned grid = 0, block = 0, chunk = 0;
  size_t lds = 0;              // bytes of dynamic LDS
  size_t rows = 0, tile = 0;   // N, rows per workgroup
};
inline FrExprPlan fr_expr_plan(int log_n, int n_regs, FrxShape s) {
  FrExprPlan p;
  if (log_n < 0 || log_n > FRX_MAX_LOG_N || n_regs < 1 || n_regs > FRX_MAX_REGS) return p;
  if (s.block < 64 || s.block > 1024 || s.block % 64 || s.chunk < 1 || s.chunk > 64 || frx_lds_bytes(s.block, n_regs) > FRX_LDS_CU) return p;
  p.rows = (size_t)1 << log_n;
  p.tile = (size_t)s.block * s.chunk;
  p.grid = (unsigned)((p.rows + p.tile - 1) / p.tile);
  p.block = (unsigned)s.block; p.chunk = (unsigned)s.chunk;
  p.lds = frx_lds_bytes(s.block, n_regs);
  p.ok = 1;
  return p;
}
inline FrExprPlan fr_expr_plan(int log_n, int n_regs) { return fr_expr_plan(log_n, n_regs, frx_shape(log_n)); }

}  // namespace bls
