// tools/fr_lookup_plain_add.hip -- a stand-alone A/B outside the library: k_frl_count as shipped (csrc/fr_lookup.hip.h, launched from
// the plan) against k_plain below, the same probe with ONE global atomicAdd per hit and no LDS stage -- the simpler design the two
// counting paths have to justify themselves against.  c = 1, tables of 2^8 / 2^12 / 2^16 / 2^20 rows, n = 2^log_n looked-up rows
// (argument, default 24) uniform / all on one row / 90 % on 16 rows; HIP events around windows of 10 calls (memsets included), the minimum
// of three; the two counter arrays are compared.  Results: profiles/fr_lookup_plain_add.md.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-sched-strategy=iterative-ilp -Iinclude -iquote bls12_381_amd/csrc \
//         tools/fr_lookup_plain_add.hip -o build/fr_lookup_plain_add && build/fr_lookup_plain_add 24
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "fr_lookup.hip.h"
using namespace bls;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); std::exit(2); } } while (0)

__global__ void __launch_bounds__(FRL_BLOCK) k_plain(const u32* __restrict__ f, size_t pitch, size_t n, int c, const u32* __restrict__ keys, const u32* __restrict__ slot, u32 mask,
                                                      unsigned iters, u32* counters, u32* __restrict__ index, unsigned long long* missing) {
  __shared__ unsigned wg_miss;
  const unsigned block = blockDim.x, lane = threadIdx.x;
  if (lane == 0) wg_miss = 0;
  __syncthreads();
  for (unsigned it = 0; it < iters; it++) {
    const size_t i = ((size_t)it * gridDim.x + blockIdx.x) * block + lane;
    if (i >= n) break;
    u32 h = frl_hash_cols(f, pitch, c, i, nullptr) & mask;
    u32 hit = 0;
    for (u32 step = 0; step <= mask; step++) {
      const u32 v = slot[h];
      if (v == 0) break;
      if (frl_equal_key(f, pitch, c, i, keys + (size_t)(v - 1) * c * 8)) { hit = v; break; }
      h = (h + 1) & mask;
    }
    if (index) index[i] = hit ? hit - 1 : FRL_MISS;
    if (!hit) { atomicAdd(&wg_miss, 1u); continue; }
    atomicAdd(&counters[hit - 1], 1u);
  }
  __syncthreads();
  if (lane == 0 && wg_miss && missing) atomicAdd(missing, (unsigned long long)wg_miss);
}

static uint64_t g_s = 1;
static uint64_t next64() { g_s += 0x9E3779B97F4A7C15ull; uint64_t z = g_s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

int main(int argc, char** argv) {
  const int log_n = argc > 1 ? std::atoi(argv[1]) : 24;
  if (log_n < 10 || log_n > 24) return 1;
  const size_t n = (size_t)1 << log_n;
  const int c = 1;
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int lr : {8, 12, 16, 20}) {
    const size_t rows = (size_t)1 << lr;
    const FrLookupPlan plan = fr_lookup_plan(rows, n);
    if (!plan.ok) return 1;
    std::vector<uint64_t> t(rows * 4);
    for (size_t i = 0; i < rows; i++) for (int w = 0; w < 4; w++) t[4 * i + w] = next64() >> 2;
    u32 *d_t, *d_keys, *d_slot, *d_cnt[2], *d_index, *d_f; unsigned long long* d_miss;
    CK(hipMalloc(&d_t, rows * 32)); CK(hipMalloc(&d_keys, rows * 32)); CK(hipMalloc(&d_slot, plan.slots * 4)); CK(hipMalloc(&d_cnt[0], rows * 4)); CK(hipMalloc(&d_cnt[1], rows * 4));
    CK(hipMalloc(&d_index, n * 4)); CK(hipMalloc(&d_f, n * 32)); CK(hipMalloc(&d_miss, 8));
    CK(hipMemcpy(d_t, t.data(), rows * 32, hipMemcpyHostToDevice));
    CK(hipMemsetAsync(d_slot, 0, plan.slots * 4, st)); CK(hipMemsetAsync(d_cnt[0], 0, 4, st));
    const u32 mask = (u32)(plan.slots - 1);
    hipLaunchKernelGGL(k_frl_build, dim3(plan.build_grid), dim3(plan.block), 0, st, (const u32*)d_t, rows, (u32)rows, c, d_keys, d_slot, mask, d_cnt[0]);
    CK(hipGetLastError()); CK(hipStreamSynchronize(st));
    size_t hot[16];
    for (auto& hrow : hot) hrow = next64() % rows;
    std::vector<uint64_t> f(n * 4);
    for (int dist = 0; dist < 3; dist++) {
      for (size_t i = 0; i < n; i++) {
        const uint64_t r = next64();
        const size_t row = dist == 0 ? r % rows : dist == 1 ? rows / 2 : ((r >> 40) % 10 < 9 ? hot[(r >> 32) & 15] : r % rows);
        for (int w = 0; w < 4; w++) f[4 * i + w] = t[4 * row + w];
      }
      CK(hipMemcpy(d_f, f.data(), n * 32, hipMemcpyHostToDevice));
      double best[2] = {1e30, 1e30};
      for (int variant = 0; variant < 2; variant++) {
        auto call = [&] {
          CK(hipMemsetAsync(d_miss, 0, 8, st)); CK(hipMemsetAsync(d_cnt[variant], 0, rows * 4, st));
          if (variant == 1) hipLaunchKernelGGL(k_plain, dim3(plan.count_grid), dim3(plan.block), 0, st, (const u32*)d_f, n, n, c, (const u32*)d_keys, (const u32*)d_slot, mask, plan.iters, d_cnt[1], d_index, d_miss);
          else if (plan.lds_path) hipLaunchKernelGGL(k_frl_count<true>, dim3(plan.count_grid), dim3(plan.block), plan.count_lds, st, (const u32*)d_f, n, n, c, (const u32*)d_keys, (const u32*)d_slot, mask, (u32)rows, plan.iters, d_cnt[0], d_index, d_miss);
          else hipLaunchKernelGGL(k_frl_count<false>, dim3(plan.count_grid), dim3(plan.block), plan.count_lds, st, (const u32*)d_f, n, n, c, (const u32*)d_keys, (const u32*)d_slot, mask, (u32)rows, plan.iters, d_cnt[0], d_index, d_miss);
        };
        call(); CK(hipGetLastError()); CK(hipStreamSynchronize(st));
        for (int w = 0; w < 3; w++) {
          CK(hipEventRecord(e0, st));
          for (int k = 0; k < 10; k++) call();
          CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
          float ms; CK(hipEventElapsedTime(&ms, e0, e1));
          best[variant] = std::min(best[variant], (double)ms / 10);
        }
      }
      std::vector<u32> a(rows), b(rows);
      CK(hipMemcpy(a.data(), d_cnt[0], rows * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), d_cnt[1], rows * 4, hipMemcpyDeviceToHost));
      unsigned long long total = 0; for (u32 v : a) total += v;
      std::printf("rows=2^%d n=2^%d c=1 %s: shipped(%s) %.4f ms, plain add %.4f ms, plain/shipped %.2f, equal %d, total %llu\n", lr, log_n, dist == 0 ? "uniform" : dist == 1 ? "one_row" : "hot16",
                  plan.lds_path ? "lds" : "cache", best[0], best[1], best[1] / best[0], (int)(a == b), total);
      std::fflush(stdout);
    }
    CK(hipFree(d_t)); CK(hipFree(d_keys)); CK(hipFree(d_slot)); CK(hipFree(d_cnt[0])); CK(hipFree(d_cnt[1])); CK(hipFree(d_index)); CK(hipFree(d_f)); CK(hipFree(d_miss));
  }
  return 0;
}
