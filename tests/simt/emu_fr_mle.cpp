// tests/simt/emu_fr_mle.cpp -- the multilinear kernels of bls12_381_amd/csrc/fr_mle.hip.h (fold, eq table, sumcheck round and its finish)
// compiled for the HOST (test infrastructure only).  Every entry point here WALKS A PLAN of csrc/fr_mle_plan.h -- the functions
// api_fr.hip launches from -- step by step, with its grids, blocks, LDS sizes, buffer roles and pitches, at whatever (block, chunk) the
// test asks for: a tile of 64 x 1 positions reaches the multi-workgroup path and the finish kernel at m = 8.
//
// The kernels add across lanes with __shfl_down and meet at the workgroup barrier, so every launch runs its block on one host thread per
// lane (the lane pool of tests/simt/emu_harness.h); there is no one-lane shortcut here.
//
// Built with the trapping bounds / shift checks, buffers from emu_guarded() end flush against an inaccessible page, and the
// tests call this library from a child process (tests/simt_fr_mle_child.py).
#define EMU_LANES 256
#define EMU_DYN_LDS_WORDS (256 * 2 * 8 * 8 + 4 * 7 * 8)           // frm_round_lds_bytes of the shipped shape with k = 8
#include "emu_harness.h"

#include "fr_mle.hip.h"
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frm_round_lds_bytes(bls::FrMleShape(), bls::FRM_MAX_K), "EMU_DYN_LDS_WORDS is smaller than the shipped shape's LDS");
static_assert(sizeof(bls::u32) * EMU_DYN_LDS_WORDS >= bls::frm_eq_lds_bytes(bls::frm_eq_lo(28, bls::FrMleShape())), "EMU_DYN_LDS_WORDS is smaller than the eq tile");

using namespace bls;

namespace {

FrMleShape shape_of(int block, int chunk) { FrMleShape s; s.block = block; s.chunk = chunk; return s; }

// api_fr.hip's frmle_launch with the launches replaced by the lane pool
int walk(const FrMlePlan& plan, FrMleShape shape, const u32* in, size_t pitch_in, u32* out, size_t pitch_out, const u32* r, const u32* point, size_t k, const FrmProg* prog,
         u32* scratch, u32* rec, int* kernels_out) {
  if (plan.n_steps < 0) return -1;
  u32* buf[4] = {const_cast<u32*>(in), out, scratch, rec};
  for (int i = 0; i < plan.n_steps; i++) {
    const FrMleStep s = plan.step[i];
    if (s.lds > sizeof(u32) * EMU_DYN_LDS_WORDS) return -1;
    u32* src = s.src >= 0 ? buf[s.src] : nullptr;
    u32* dst = s.dst >= 0 ? buf[s.dst] : nullptr;
    const size_t pi = s.pitch_in ? s.pitch_in : pitch_in, po = s.pitch_out ? s.pitch_out : pitch_out;
    kernels_out[i] = s.kernel;
    switch (s.kernel) {
      case FRM_K_FOLD: {
        const u32* rr = s.var >= 0 ? point + (size_t)s.var * 8 : r;
        launch_threads(s.grid, s.block, [=] { k_frm_fold(src, pi, dst, po, s.m - 1, s.items, rr); });
        break;
      }
      case FRM_K_EQ:
        launch_threads(s.grid, s.block, [=] { k_frm_eq(point, s.m, frm_eq_lo(s.m, shape), dst); });
        break;
      case FRM_K_COPY:
        for (size_t j = 0; j < s.items; j++) memcpy(dst + j * po * 8, src + j * pi * 8, 32);
        break;
      case FRM_K_ROUND:
        launch_threads(s.grid, s.block, [=] { k_frm_round<false>(src, pi, s.items, (unsigned)k, (unsigned)shape.chunk, *prog, nullptr, dst); });
        break;
      case FRM_K_ROUND_FUSED:
        launch_threads(s.grid, s.block, [=] { k_frm_round<true>(src, pi, s.items, (unsigned)k, (unsigned)shape.chunk, *prog, r, dst); });
        break;
      default:
        launch_threads(s.grid, s.block, [=] { k_frm_round_finish(src, s.items, prog->deg + 1, dst); });
        break;
    }
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}

}  // namespace

extern "C" {

// kernels_out of every entry point: the FrMleKernel of every step, -1 ends it (at least 30 ints).  Each returns the number of steps, -1
// for a shape or size the plan does not take, -2 for a term program the validation refuses.

// in: (k - 1) * pitch_in + 2^m scalars, out: (k - 1) * pitch_out + 2^(m-1) (may be `in` itself with equal pitches); r: one scalar
int emu_frm_fold(const u32* in, size_t pitch_in, u32* out, size_t pitch_out, int m, size_t k, const u32* r, int block, int chunk, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  const FrMleShape sh = shape_of(block, chunk);
  return walk(fr_mle_fold_plan(m, k, sh), sh, in, pitch_in, out, pitch_out, r, nullptr, k, nullptr, nullptr, nullptr, kernels_out);
}
// point: m scalars (NULL for m = 0), out: 2^m
int emu_frm_eq(const u32* point, int m, u32* out, int block, int chunk, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  const FrMleShape sh = shape_of(block, chunk);
  return walk(fr_eq_table_plan(m, sh), sh, nullptr, 0, out, 0, nullptr, point, 1, nullptr, nullptr, nullptr, kernels_out);
}
// the scalars the scratch of an evaluation must hold
size_t emu_frm_eval_scratch(int m, size_t k, int block, int chunk) { return fr_mle_eval_plan(m, k, shape_of(block, chunk)).scratch; }
// tables: (k - 1) * pitch + 2^m scalars (not written), point: m scalars, out: k scalars, scratch: emu_frm_eval_scratch scalars
int emu_frm_eval(const u32* tables, size_t pitch, int m, size_t k, const u32* point, u32* out, u32* scratch, int block, int chunk, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  const FrMleShape sh = shape_of(block, chunk);
  return walk(fr_mle_eval_plan(m, k, sh), sh, tables, pitch, out, 1, nullptr, point, k, nullptr, scratch, nullptr, kernels_out);
}
// the records (of deg + 1 scalars each) a round's scratch must hold; -1 for a shape the plan refuses
long emu_frm_round_recs(int m, size_t k, int deg, int fused, int block, int chunk) {
  const FrMlePlan p = fr_sumcheck_round_plan(m, k, deg, fused != 0, shape_of(block, chunk));
  return p.n_steps < 0 ? -1 : (long)p.recs;
}
// the degree of a program, or -2 when the validation refuses it
int emu_frm_prog_degree(size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef) {
  FrmProg prog;
  return frm_prog_build(k, n_terms, term_ptr, term_tab, coef, &prog) ? -2 : (int)prog.deg;
}
// tables: (k - 1) * pitch + 2^m scalars; r_prev: one scalar or NULL; evals: deg + 1 scalars; rec: emu_frm_round_recs records
int emu_frm_round(u32* tables, size_t pitch, int m, size_t k, size_t n_terms, const uint32_t* term_ptr, const uint8_t* term_tab, const uint64_t* coef, const u32* r_prev, u32* evals,
                  u32* rec, int block, int chunk, int* kernels_out) {
  if (!shape_ok(block, chunk)) return -1;
  const FrMleShape sh = shape_of(block, chunk);
  FrmProg prog;
  if (frm_prog_build(k, n_terms, term_ptr, term_tab, coef, &prog)) return -2;
  return walk(fr_sumcheck_round_plan(m, k, (int)prog.deg, r_prev != nullptr, sh), sh, tables, pitch, evals, 0, r_prev, nullptr, k, &prog, nullptr, rec, kernels_out);
}
}
