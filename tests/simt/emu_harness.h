// tests/simt/emu_harness.h -- what every pooled emulation library of tests/simt shares (test infrastructure only): the definitions
// of the lane state that tests/simt/hip/hip_runtime.h declares, the lane pool with its two launchers, and emu_guarded().  An
// emu_*.cpp defines EMU_LANES (the largest block it launches) and, where its kernels use dynamic LDS, EMU_DYN_LDS_WORDS, includes
// this header ONCE, then the csrc headers it emulates, and adds only its plan walkers and extern "C" entry points.  Every library is
// still a .so of its own, with its own pool and its own g_emu: both macros size static arrays.
//
// The libraries are built with trapping bounds / shift checks (the compile line of tests/simt_harness.py): an index outside an LDS array
// traps.  emu_guarded() places a buffer so that it ends flush against an inaccessible page: an access past its end faults.  Both end
// the process, so the tests call these libraries from a child process of their own.
#pragma once
#ifndef EMU_LANES
#error "define EMU_LANES before including emu_harness.h"
#endif
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <functional>
#include <thread>
#include <vector>

thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
EmuState g_emu;

namespace {

// A pool of EMU_LANES lane threads, started once: a workgroup is one job for the lanes below its block size.
struct LanePool {
  std::vector<std::thread> th;
  EmuMeet<1> start, done;
  std::function<void()> job;
  unsigned block = 0, grid = 0, blk = 0;
  LanePool() {
    for (unsigned l = 0; l < EMU_LANES; l++)
      th.emplace_back([this, l] {
        for (;;) {
          start.barrier(EMU_LANES + 1);
          if (l < block) {
            threadIdx.x = l; blockDim.x = block; blockIdx.x = blk; gridDim.x = grid;
            job();
          }
          done.barrier(EMU_LANES + 1);
        }
      });
  }
  void workgroup(unsigned g, unsigned b, unsigned i, const std::function<void()>& fn) {
    job = fn; grid = g; block = b; blk = i;
    start.barrier(EMU_LANES + 1);
    done.barrier(EMU_LANES + 1);
  }
};
LanePool* pool() { static LanePool* p = new LanePool(); return p; }          // never destroyed: its threads wait for work until the process ends

unsigned nblk(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }   // host.h
// kernel<<<grid, block>>> with one host thread per lane
template <class Fn> void launch_threads(unsigned grid, unsigned block, Fn fn) {
  for (unsigned i = 0; i < grid; i++) pool()->workgroup(grid, block, i, fn);
}
// the same for a kernel without any cross-lane operation: the lanes one after the other in this thread
template <class Fn> void launch_loop(unsigned grid, unsigned block, Fn fn) {
  blockDim.x = block; gridDim.x = grid;
  for (unsigned i = 0; i < grid; i++)
    for (unsigned l = 0; l < block; l++) { blockIdx.x = i; threadIdx.x = l; fn(); }
}
// a (block, chunk) tile shape the wavefront-scanning kernels (scan, SpMV, MLE) and the pool both take
bool shape_ok(int block, int chunk) { return block >= 64 && block <= EMU_LANES && block % 64 == 0 && chunk >= 1; }

}  // namespace

// `bytes` bytes whose end is the start of an inaccessible page; never freed
extern "C" void* emu_guarded(size_t bytes) {
  const size_t page = (size_t)sysconf(_SC_PAGESIZE);
  const size_t body = (bytes + page - 1) / page * page;
  const size_t guard = (size_t)1 << 20;          // wider than any stride of the kernels: a read far past the end still faults
  char* m = (char*)mmap(nullptr, body + guard, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == (char*)MAP_FAILED) return nullptr;
  if (mprotect(m + body, guard, PROT_NONE) != 0) return nullptr;
  return m + body - bytes;
}
