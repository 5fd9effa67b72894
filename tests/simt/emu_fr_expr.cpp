// tests/simt/emu_fr_expr.cpp -- the Fr expression interpreter (bls12_381_amd/csrc/fr_expr.hip.h) compiled for the HOST (test
// infrastructure only).  emu_fr_expr_eval launches k_frx_eval FROM THE PLAN of csrc/fr_expr_plan.h -- the function api_fr.hip launches
// from -- with its grid, block, dynamic LDS and rows per lane, at whatever (block, chunk) the test asks for: at 64 x 2 a table of 512 rows
// is four workgroups.  emu_fr_expr_build is frx_prog_build, the validation and the image the handle uploads.
//
// Over tests/simt/emu_harness.h.  The kernel has no cross-lane operation (a lane touches its own register slots only), so the lanes of
// a workgroup run one after the other (launch_loop).  The library is built with the trapping bounds / shift checks, buffers from
// emu_guarded() end flush against an inaccessible page, and the tests call this library from a child process
// (tests/simt_fr_expr_child.py).  -DFRX_FAULT=n builds the kernel with one of its five seeded faults (tests/test_simt_fr_expr.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * 8 * 8)                            // frx_lds_bytes of the shipped block at eight registers
#include "emu_harness.h"

#include "fr_expr.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frx_lds_bytes(bls::FRX_BLOCK, bls::FRX_MAX_REGS), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");

using namespace bls;

namespace {

FrExprPlan plan_of(int log_n, int n_regs, int block, int chunk) {
  if (block == 0) return fr_expr_plan(log_n, n_regs);
  if (block > EMU_LANES) return FrExprPlan();
  FrxShape s; s.block = block; s.chunk = chunk;
  return fr_expr_plan(log_n, n_regs, s);
}

}  // namespace

extern "C" {

// the plan of an evaluation (block == 0: the shipped shape of log_n).  info: grid, block, chunk, lds, tile, rows.  Returns 1, or 0 for a refusal.
int emu_fr_expr_plan(int log_n, int n_regs, int block, int chunk, size_t* info) {
  const FrExprPlan p = plan_of(log_n, n_regs, block, chunk);
  info[0] = p.grid; info[1] = p.block; info[2] = p.chunk; info[3] = p.lds; info[4] = p.tile; info[5] = p.rows;
  return p.ok;
}
// frx_prog_build.  image: FRX_IMAGE_WORDS u32; info: products, cols_read, max_rot, image words; err: the refusal's text (err_len bytes).
// Returns 0 for a valid program, 1 for a refused one.
int emu_fr_expr_build(int n_cols, int n_regs, int n_consts, const uint64_t* consts, size_t n_instr, const uint32_t* code, uint32_t* image, size_t* info, char* err, size_t err_len) {
  FrxProg* prog = new FrxProg();
  FrxInfo f;
  const char* what = frx_prog_build(n_cols, n_regs, n_consts, consts, n_instr, code, prog, &f);
  info[3] = FRX_IMAGE_WORDS;
  if (what) { std::snprintf(err, err_len, "%s", what); delete prog; return 1; }
  for (int i = 0; i < FRX_IMAGE_WORDS; i++) image[i] = prog->w[i];
  info[0] = f.products; info[1] = f.cols_read; info[2] = (size_t)f.max_rot;
  if (err_len) err[0] = 0;
  delete prog;
  return 0;
}
// image: what emu_fr_expr_build wrote; cols / log_len: FRX_MAX_COLS entries (NULL / 0 for a column that is not read); out: 2^log_n scalars.
// Returns the grid, or -1 for what the plan refuses.
int emu_fr_expr_eval(const u32* image, const u32* const* cols, const uint32_t* log_len, int log_n, int log_stride, int block, int chunk, u32* out) {
  const FrExprPlan p = plan_of(log_n, (int)image[1], block, chunk);
  if (!p.ok || p.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
  FrxCols k;
  for (int j = 0; j < FRX_MAX_COLS; j++) { k.p[j] = cols[j]; k.log_len[j] = log_len[j]; }
  const unsigned ch = p.chunk;
  launch_loop(p.grid, p.block, [=] { k_frx_eval(image, k, log_n, log_stride, ch, out); });
  return (int)p.grid;
}
}
