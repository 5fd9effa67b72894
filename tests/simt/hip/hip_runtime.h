// tests/simt/hip/hip_runtime.h -- host-side stand-in for <hip/hip_runtime.h>, TEST INFRASTRUCTURE ONLY.
//
// The lane-cooperative device code of bls12_381_amd/csrc (pairlane.hip.h, quad.hip.h, the pairing code, the segmented MSM) is plain
// integer C++ plus a few cross-lane primitives: a DPP move with a quad permutation, wavefront shuffles, the workgroup barrier and LDS
// atomics.  Compiled for the host with this header first on the include path, every lane of a workgroup becomes a host thread and a
// cross-lane operation becomes a slot exchange between the threads that take part in it, so the CPU test-suite can run the SAME device
// functions bit for bit against the oracle (tests/test_simt_emulation.py, tests/test_simt_msm.py).  Nothing in the product builds
// against or links this file.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstddef>
#include <cstring>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

struct EmuDim3 { unsigned x = 0, y = 0, z = 0; };
extern thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))
#define __noinline__ __attribute__((noinline))
#define __launch_bounds__(...)
#define __shared__ static
#define __align__(n) __attribute__((aligned(n)))
// dynamic LDS (`extern __shared__ u32 name[]` in the HIP build, fe.hip.h): a static array of a fixed size, the largest a launch may ask for
#ifndef EMU_DYN_LDS_WORDS
#define EMU_DYN_LDS_WORDS (16 * 1024)
#endif
#define BLS_DYN_LDS(name) static u32 name[EMU_DYN_LDS_WORDS]

// ---- lanes of one workgroup: at most EMU_LANES host threads, one workgroup at a time ------------------------------------
#ifndef EMU_LANES
#define EMU_LANES 4
#endif

// A meeting point of the N lanes that take part in ONE cross-lane operation: each leaves its value, waits for the others and reads
// the value of its source lane.  The values of consecutive meetings alternate between two sets of slots, so one wait per exchange is
// enough: a lane writes set p again only after a meeting on set 1 - p, which every lane reaches after its read of set p.  A lane that
// waits goes to sleep (futex) after a short spin: there are many more lanes than host cores, and a spinning lane would take the
// core of the lane it waits for.
template <int N> struct EmuMeet {
  std::atomic<unsigned> arrived{0};
  std::atomic<unsigned> phase{0};
  std::atomic<unsigned> sleepers{0};
  int slot[2][N];
  void wait(unsigned n, unsigned ph) {
    if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      arrived.store(0, std::memory_order_relaxed);
      phase.store(ph + 1, std::memory_order_seq_cst);
      if (sleepers.load(std::memory_order_seq_cst)) syscall(SYS_futex, reinterpret_cast<unsigned*>(&phase), FUTEX_WAKE_PRIVATE, 0x7fffffff, nullptr, nullptr, 0);
      return;
    }
    for (int i = 0; i < 4; i++) { if (phase.load(std::memory_order_acquire) != ph) return; __builtin_ia32_pause(); }
    sleepers.fetch_add(1, std::memory_order_seq_cst);
    while (phase.load(std::memory_order_seq_cst) == ph) syscall(SYS_futex, reinterpret_cast<unsigned*>(&phase), FUTEX_WAIT_PRIVATE, ph, nullptr, nullptr, 0);
    sleepers.fetch_sub(1, std::memory_order_seq_cst);
  }
  // lane `me` of the n lanes that meet here leaves v and takes the value of lane `from` (both numbered within the meeting)
  int exchange(unsigned n, unsigned me, unsigned from, int v) {
    const unsigned ph = phase.load(std::memory_order_acquire);        // only the lanes of this meeting move it, and all of them are past the last one
    slot[ph & 1][me] = v;
    wait(n, ph);
    return slot[ph & 1][from];
  }
  void barrier(unsigned n) { wait(n, phase.load(std::memory_order_acquire)); }
};

struct EmuState {
  EmuMeet<1> wg;                                  // __syncthreads: all blockDim.x lanes
  // DPP: one meeting per (quad, set of lanes that exchange values).  v_mov_b32_dpp quad_perm:[a,b,c,d] makes lane L read lane
  // (L & ~3) | perm[L & 3]; the lanes that meet are those connected through the permutation ([1,0,3,2]: the two pairs of a quad, each on
  // its own -- the pairs of a quad may sit in different iterations of a loop, or one of them may have left the kernel), never lanes that
  // exchange nothing.
  EmuMeet<4> dpp[(EMU_LANES + 3) / 4][16];
  // shuffles: one meeting per group of `width` lanes (a power of two <= 64, so a group never spans wavefronts)
  EmuMeet<64> shfl[7][EMU_LANES];
};
extern EmuState g_emu;

static inline int emu_update_dpp(int old, int src, int ctrl, int /*row_mask*/, int /*bank_mask*/, bool /*bound_ctrl*/) {
  (void)old;
  const unsigned lane = threadIdx.x, q = lane & 3u;
  // the set of lanes of this quad connected with q through  l -> perm[l]
  unsigned mask = 1u << q;
  for (int pass = 0; pass < 3; pass++)
    for (unsigned l = 0; l < 4; l++) {
      const unsigned s = ((unsigned)ctrl >> (2 * l)) & 3u;
      if (((mask >> l) | (mask >> s)) & 1u) mask |= (1u << l) | (1u << s);
    }
  const unsigned from = ((unsigned)ctrl >> (2 * q)) & 3u;
  if (mask == (1u << q)) return src;              // reads itself
  return g_emu.dpp[lane >> 2][mask].exchange((unsigned)__builtin_popcount(mask), q, from, src);
}
// __shfl_down / __shfl_up within groups of `width` lanes: a source lane outside the group gives the caller's own value
static inline int emu_shfl(int v, int src_in_group, int width) {
  const unsigned lane = threadIdx.x, w = (unsigned)width, me = lane & (w - 1);
  const bool ok = src_in_group >= 0 && src_in_group < width;
  const int got = g_emu.shfl[__builtin_ctz(w)][lane / w].exchange(w, me, ok ? (unsigned)src_in_group : me, v);
  return ok ? got : v;
}
static inline int __shfl_down(int v, unsigned d, int width = 64) { return emu_shfl(v, (int)((threadIdx.x & (unsigned)(width - 1)) + d), width); }
static inline int __shfl_up(int v, unsigned d, int width = 64) { return emu_shfl(v, (int)(threadIdx.x & (unsigned)(width - 1)) - (int)d, width); }
// LDS atomics of the wide kernel (ds_add_u64 / ds_wrxchg_rtn_b64) and of the MSM counting sorts
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicExch(unsigned long long* p, unsigned long long v) { return __atomic_exchange_n(p, v, __ATOMIC_RELAXED); }
static inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
// status-word flags (global memory)
static inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline void __threadfence() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
template <class T> static inline T min(T a, T b) { return a < b ? a : b; }
// bit intrinsics of fr.hip.h's transform kernels (every header that includes it for the field code sees them too)
static inline unsigned long long __brevll(unsigned long long x) { return __builtin_bitreverse64(x); }
static inline int __clzll(unsigned long long x) { return __builtin_clzll(x); }
// wave vote: every emulated lane decides for itself (only used for an early loop exit whose extra iterations are identities)
static inline int __all(int p) { return p; }
struct uint4 { unsigned x, y, z, w; };
struct uint2 { unsigned x, y; };
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
static inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
#define __builtin_amdgcn_update_dpp emu_update_dpp
// EMU_SYNCTHREADS_HOOK: a library whose kernels meet ONLY at the workgroup barrier may run the lanes of a workgroup as fibers of one
// thread and supplies the barrier itself (tests/simt/emu_msm_front.cpp)
#ifdef EMU_SYNCTHREADS_HOOK
void emu_syncthreads();
static inline void __syncthreads() { emu_syncthreads(); }
#else
static inline void __syncthreads() { g_emu.wg.barrier(blockDim.x); }
#endif
#define __builtin_amdgcn_s_setprio(x) ((void)0)
#define __builtin_amdgcn_s_getreg(x) 0u
#define __builtin_amdgcn_readfirstlane(x) (x)
#define __builtin_readcyclecounter() 0ull
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
