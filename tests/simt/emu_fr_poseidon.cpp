// tests/simt/emu_fr_poseidon.cpp -- the Poseidon kernels of bls12_381_amd/csrc/fr_poseidon.hip.h (permute, hash / Merkle level)
// compiled for the HOST (test infrastructure only).  emu_frp_create runs the validation, the sparse
// derivation and the image builder of csrc/fr_poseidon_plan.h -- what blsgpu_fr_poseidon_create runs -- and emu_frp_run WALKS A PLAN of
// that header step by step, with its grids, blocks, buffer roles and level offsets, at whatever block the test asks for: with 16 lanes
// per workgroup every level of a small tree still spans several workgroups and a partial last one.
//
// Every launch runs its block on one host thread per lane (the lane pool of tests/simt/emu_harness.h), as the other emulations do.
//
// Built with the trapping bounds / shift checks, buffers from emu_guarded() -- the constant image included -- end flush against
// an inaccessible page, and the tests call this library from a child process (tests/simt_fr_poseidon_child.py).
#define EMU_LANES 256
#include "emu_harness.h"

#include "fr_poseidon.hip.h"

using namespace bls;

namespace {

FrPoseidonHost g_inst;                              // the instance of the last emu_frp_create
u32* g_img = nullptr;                               // its image, in a guarded buffer of exactly its size

template <int T, bool SP>
void run_step(const FrPoseidonStep& s, const FrArg& tag, const u32* src, u32* dst, u32* roots) {
  const FrpArgs a = g_inst.args;
  const u32* img = g_img;
  switch (s.kernel) {
    case FRP_K_PERMUTE: launch_threads(s.grid, s.block, [=] { k_frp_permute<T, SP>(a, img, src, dst, s.items); }); break;
    default: launch_threads(s.grid, s.block, [=] { k_frp_hash<T, SP>(a, img, tag, src, dst, roots, s.items); }); break;      // HASH, LEVEL
  }
}

}  // namespace

extern "C" {

// blsgpu_fr_poseidon_create on the host: 0 and info = {form, products, image words}, or -1 and the refusal's text in `err`
int emu_frp_create(int t, int r_full, int r_partial, const uint64_t* rc, const uint64_t* mds, int form, size_t* info, char* err, size_t err_len) {
  FrPoseidonHost h;
  const std::string what = fr_poseidon_build(t, r_full, r_partial, rc, mds, form, &h);
  if (!what.empty()) { snprintf(err, err_len, "%s", what.c_str()); return -1; }
  g_inst = h;
  g_img = (u32*)emu_guarded(h.image.size() * 4);
  if (!g_img) return -2;
  memcpy(g_img, h.image.data(), h.image.size() * 4);
  info[0] = (size_t)h.form; info[1] = h.products; info[2] = h.image.size();
  return 0;
}

// the plan of a call: kind 0 permute, 1 hash_many (n = count), 2 merkle (n = k trees).  sizes = {leaves, node_count, scratch}; returns
// the number of steps, -1 for a refusal
int emu_frp_plan(int kind, size_t n, int height, int keep_nodes, int block, size_t* sizes) {
  FrPoseidonShape sh; sh.block = block;
  const FrPoseidonPlan plan = kind == 2 ? fr_poseidon_merkle_plan(g_inst.t, height, n, keep_nodes != 0, sh) : fr_poseidon_many_plan(kind == 0 ? FRP_K_PERMUTE : FRP_K_HASH, g_inst.t, n, sh);
  sizes[0] = plan.leaves; sizes[1] = plan.node_count; sizes[2] = plan.scratch;
  return plan.n_steps;
}

// Runs a call on the instance of emu_frp_create.  in: the states / preimages / leaves; out: the states / digests / roots; nodes: the
// caller's nodes array, or the scratch of sizes[2] scalars when keep_nodes == 0 (NULL when that is 0).  kernels_out: the FrPoseidonKernel
// of every step, then -1 (FRP_MAX_STEPS + 1 ints).  Returns the number of steps.
int emu_frp_run(int kind, const u32* tag, const u32* in, size_t n, int height, int keep_nodes, u32* out, u32* nodes, int block, int* kernels_out) {
  if (block > EMU_LANES || block > FRP_BLOCK) return -1;
  FrPoseidonShape sh; sh.block = block;
  const FrPoseidonPlan plan = kind == 2 ? fr_poseidon_merkle_plan(g_inst.t, height, n, keep_nodes != 0, sh) : fr_poseidon_many_plan(kind == 0 ? FRP_K_PERMUTE : FRP_K_HASH, g_inst.t, n, sh);
  if (plan.n_steps < 0) return -1;
  FrArg tg = {};
  if (tag) for (int w = 0; w < 8; w++) tg.w[w] = tag[w];
  for (int i = 0; i < plan.n_steps; i++) {
    const FrPoseidonStep s = plan.step[i];
    kernels_out[i] = s.kernel;
    if (s.kernel == FRP_K_COPY) { memcpy(out, in, s.items * 32); continue; }
    const u32* src = (s.src == FRP_BUF_IN ? in : (const u32*)nodes) + s.src_off * 8;
    u32* dst = (s.dst == FRP_BUF_OUT ? out : nodes) + s.dst_off * 8;
    u32* roots = s.roots && s.dst != FRP_BUF_OUT ? out : nullptr;
    const bool sp = g_inst.form == FRP_FORM_SPARSE;
#define EMU_CASE(T) case T: if (sp) run_step<T, true>(s, tg, src, dst, roots); else run_step<T, false>(s, tg, src, dst, roots); break;
    switch (g_inst.t) { EMU_CASE(2) EMU_CASE(3) EMU_CASE(4) EMU_CASE(5) EMU_CASE(9) EMU_CASE(12) default: return -1; }
#undef EMU_CASE
  }
  kernels_out[plan.n_steps] = -1;
  return plan.n_steps;
}
}
