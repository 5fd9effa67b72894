// tests/simt/emu_msm_front.cpp -- the integer front end of the large MSM (bls12_381_amd/csrc/msm.hip.h) compiled for the HOST (test
// infrastructure only): the two-level counting sort, the fallback sort and the work-item kernels.  The entry points launch the
// __global__ functions themselves with the grid, block and dynamic-LDS shapes of api_msm.hip (msm_sort_fast, msm_sort_fallback,
// msm_accumulate; the key split is the one of csrc/msm_plan.h), one stage per entry point: the tests hand every stage inputs of their
// own (tests/test_simt_msm_front.py).
//
// A library of its own because k_sort_scan and k_scan_top run 1024 lanes and k_sort_fine runs up to 8192 workgroups.  With the lane
// pool of emu_harness.h (one host thread per lane) that was measured at 28 s for ONE sort with 7424 counters: every workgroup wakes
// the whole pool, every barrier parks and wakes its lanes.  These kernels are integer code whose lanes meet only at __syncthreads
// (no DPP, no shuffle), so here the lanes of a workgroup are FIBERS of one thread, resumed in lane order; a lane that reaches the
// barrier hands over to the next, and one round over the lanes is one barrier phase (launch_fibers below; hip_runtime.h
// EMU_SYNCTHREADS_HOOK).  The interleaving is one of those the GPU may produce; LDS and global atomics keep their meaning.  Its limit:
// between two barriers lane l always runs before lane l + 1, so a MISSING barrier whose producer is the lower lane is not seen.  The
// trapping checks, launch_loop and emu_guarded() are those of tests/simt/emu_harness.h; the tests call this library from a child
// process (tests/simt_msm_front_child.py), which places every buffer, at exactly the size msm_plan.h msm_sizes gives for it, flush
// against an inaccessible page.
//
// Not checked here: the dynamic LDS of the emulation is one fixed array (EMU_DYN_LDS_WORDS = 16384 words, the 2 * SORT_MAX_COUNTERS
// the scatter may ask for), so a launch that ASKS for too few LDS bytes is only caught on the GPU.
#define EMU_SYNCTHREADS_HOOK
#define EMU_LANES 4                      // the thread pool is never started
#include "emu_harness.h"

// emu_switch(from, to): park the running context (its callee-saved registers on its own stack, the stack pointer in *from) and resume
// the one whose stack pointer is `to`.  swapcontext does the same with a system call per switch, and one sort with 7424 counters
// switches ten million times.
#if !defined(__x86_64__)
#error "emu_msm_front.cpp switches fibers with x86-64 code"
#endif
extern "C" void emu_switch(void** from, void* to);
asm(".text\n.hidden emu_switch\n.globl emu_switch\n.type emu_switch,@function\nemu_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n  ret\n"
    ".size emu_switch, .-emu_switch\n");

#include "msm.hip.h"
#include "msm_plan.h"

using namespace bls;

namespace {

constexpr unsigned FIBERS = 1024;        // the widest block (k_sort_scan, k_scan_top)
constexpr size_t FIBER_STACK = 256 << 10;
void* g_sp[FIBERS];                      // the saved stack pointer of every parked fiber
void* g_sched_sp;
bool g_done[FIBERS];
unsigned g_cur;
bool g_in_fibers = false;             // a workgroup is running as fibers: only then may a kernel reach the barrier
const std::function<void()>* g_job;
// a fiber lives as long as the process: it runs the current job as lane g_cur, reports, and parks until the next workgroup
void fiber_main() {
  for (;;) { (*g_job)(); g_done[g_cur] = true; emu_switch(&g_sp[g_cur], g_sched_sp); }
}

// kernel<<<grid, block>>>: the lanes of a workgroup as fibers, resumed in lane order until all have left the kernel
template <class Fn> void launch_fibers(unsigned grid, unsigned block, Fn fn) {
  static char* stacks = nullptr;
  if (!stacks) {
    stacks = (char*)mmap(nullptr, FIBERS * FIBER_STACK, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (stacks == (char*)MAP_FAILED) __builtin_trap();
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    for (unsigned l = 0; l < FIBERS; l++) {
      // the lowest page of every stack is inaccessible: a fiber that outgrows its stack faults instead of writing into its neighbour's
      if (mprotect(stacks + l * FIBER_STACK, page, PROT_NONE) != 0) __builtin_trap();
      // what emu_switch pops on the first resume: six registers, then fiber_main as the return address, entered as if by a call
      void** sp = (void**)(stacks + (l + 1) * FIBER_STACK) - 8;
      for (int k = 0; k < 8; k++) sp[k] = nullptr;
      sp[6] = (void*)&fiber_main;
      g_sp[l] = sp;
    }
  }
  if (block > FIBERS) __builtin_trap();
  const std::function<void()> job = fn;
  g_job = &job;
  blockDim.x = block; gridDim.x = grid;
  g_in_fibers = true;
  for (unsigned i = 0; i < grid; i++) {
    blockIdx.x = i;
    for (unsigned l = 0; l < block; l++) g_done[l] = false;
    for (unsigned left = block; left;)
      for (unsigned l = 0; l < block; l++)
        if (!g_done[l]) {
          g_cur = l; threadIdx.x = l;
          emu_switch(&g_sched_sp, g_sp[l]);
          if (g_done[l]) left--;
        }
  }
  g_in_fibers = false;
}

// msm_plan.h: the split of the (bucket set, |digit| - 1) key, as msm_shape takes it
typedef MsmSortSplit Split;
Split split_of(int cw, int nwin, int merged) { return msm_sort_split(cw, merged ? 1 : nwin, merged != 0); }

// api_msm.hip msm_sort_fast: the hist and scatter launches by words per sort scalar
template <int WORDS>
void hist(const u32* in, u32* ghist, int ns, int cw, int nwin, const Split& s, int merged, u32* status) {
  launch_fibers(nblk(ns, SORT_TILE), SORT_THREADS, [=] { k_sort_hist<WORDS>(in, ghist, ns, cw, nwin, s.fine_bits, s.ncoarse, merged, status); });
}
template <int WORDS>
void scatter(const u32* in, const u32* gbase, u32* gcur, u32* ent, int ns, int cw, int nwin, const Split& s, int merged, u32 stride) {
  launch_fibers(nblk(ns, SORT_TILE), SORT_THREADS, [=] { k_sort_scatter<WORDS>(in, gbase, gcur, ent, ns, cw, nwin, s.fine_bits, s.ncoarse, merged, stride); });
}

}  // namespace

// __syncthreads of the kernels (hip_runtime.h): back to the scheduler, which resumes this lane after every other live lane has run
// A kernel with a barrier launched through launch_loop has no fiber to park: trap.
void emu_syncthreads() {
  if (!g_in_fibers) __builtin_trap();
  emu_switch(&g_sp[g_cur], g_sched_sp);
}

extern "C" {

int emu_front_constants(int which) {
  const int v[] = {SORT_TILE, SORT_THREADS, SORT_MAX_COUNTERS, ITEM_CAP_MAX, ITEM_BINS, ITEM_BLOCK_BUCKETS, HEAVY_SMALL, HEAVY_BIG_BLOCKS, (int)sizeof(ItemDesc), (int)sizeof(uint4)};
  return v[which];
}
// the counters the sort needs, or -1 where msm_plan.h msm_shape refuses the configuration (the counter table)
int emu_sort_counters(int cw, int nwin, int merged) {
  const int nc = split_of(cw, nwin, merged).nc;
  return nc > SORT_MAX_COUNTERS ? -1 : nc;
}

// api_msm.hip msm_sort_fast, the two-level counting sort.  hist: the slot's counter buffer of 3 * SORT_MAX_COUNTERS + 4 words in the fixed
// layout [MAX] counts | [MAX + 1] bases | [MAX] cursors (msm_sizes hist), counts zero on entry as the product keeps them;
// words: 8 (plain, merged allowed), 4 (GLV halves), 2 (psi digits); stride: bases->n with resident tables, else 0
void emu_sort_fast(int words, const u32* in, int ns, int cw, int nwin, int merged, u32 stride, u32* hist_buf, u32* ctrl, u32* ent, u32* sorted, u32* offs, u32* status) {
  const Split s = split_of(cw, nwin, merged);
  u32* ghist = hist_buf;
  u32* gbase = ghist + SORT_MAX_COUNTERS;
  u32* gcur = gbase + SORT_MAX_COUNTERS + 1;
  if (words == 4) hist<4>(in, ghist, ns, cw, nwin, s, 0, status);
  else if (words == 2) hist<2>(in, ghist, ns, cw, nwin, s, 0, status);
  else hist<8>(in, ghist, ns, cw, nwin, s, merged ? 1 : 0, status);
  launch_fibers(1, 1024, [=] { k_sort_scan(ghist, gbase, gcur, s.nc, ctrl, 4 + 2 * ITEM_BINS); });
  if (words == 4) scatter<4>(in, gbase, gcur, ent, ns, cw, nwin, s, 0, 0);
  else if (words == 2) scatter<2>(in, gbase, gcur, ent, ns, cw, nwin, s, 0, 0);
  else scatter<8>(in, gbase, gcur, ent, ns, cw, nwin, s, merged ? 1 : 0, stride);
  launch_fibers(s.nc, 256, [=] { k_sort_fine(ent, gbase, sorted, offs, s.fine_bits, s.nc); });
}

// api_msm.hip msm_sort_fallback, the fallback sort over n 256-bit scalars.  hist: nb words, zero on entry (the product's buffer is
// larger, but only these are cleared), bsum: 4096 words (msm_sizes bsum), ent / rank / sorted: total = nwin * n words each
void emu_sort_fallback(const u32* in, int n, int cw, int nwin, u32* hist_buf, u32* bsum, u32* ent, u32* rank, u32* offs, u32* sorted, u32* status) {
  const size_t nb = (size_t)nwin << (cw - 1), total = (size_t)nwin * n;
  launch_loop(nblk(n, 256), 256, [=] { k_msm_digits(in, ent, rank, hist_buf, n, cw, nwin, status); });
  const unsigned sb = nblk(nb, 1024);
  launch_fibers(sb, 256, [=] { k_scan_block_sums(hist_buf, bsum, (int)nb); });
  launch_fibers(1, 1024, [=] { k_scan_top(bsum, (int)sb); });
  launch_fibers(sb, 256, [=] { k_scan_apply(hist_buf, bsum, offs, (int)nb); });
  launch_loop(nblk(total, 256), 256, [=] { k_msm_scatter(ent, rank, offs, sorted, n, total); });
}

// api_msm.hip msm_accumulate, the work items of gnb buckets.  ctrl: 4 + 2 * ITEM_BINS words, zero on entry (k_sort_scan / the fallback
// sort's memset clear them)
void emu_items(const u32* offs, int gnb, u32 cap, u32* ctrl, u32* items, u32* heavy) {
  u32* bins = ctrl + 4;
  u32* bcur = ctrl + 4 + ITEM_BINS;
  launch_fibers(nblk(gnb, ITEM_BLOCK_BUCKETS), 256, [=] { k_item_count(offs, bins, ctrl, gnb, cap); });
  launch_fibers(1, 256, [=] { k_item_scan(bins, ctrl, cap); });
  launch_fibers(nblk(gnb, ITEM_BLOCK_BUCKETS), 256, [=] { k_item_fill(offs, bins, bcur, ctrl, reinterpret_cast<ItemDesc*>(items), reinterpret_cast<uint4*>(heavy), gnb, cap); });
}
}
