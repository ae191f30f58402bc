// block_scan.h -- the u64 block scan the planner's kernels (kernel_plan.h) and
// the router's (kernel_route.h) share.  Blocks of kThreads = 256 threads, wave64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xsknf_gpu {
namespace scan {

constexpr int kThreads = 256;

// Inclusive scan of one u64 per thread over the block; *total = the block's sum.
// wtot: 4 words of LDS.  Every thread of the block calls it.
__device__ inline uint64_t block_incl_scan(uint64_t x, uint64_t *wtot, uint64_t *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) wtot[wv] = x;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const uint64_t t = wtot[w];
    if (w < wv) pre += t;
    tot += t;
  }
  __syncthreads();   // wtot is rewritten by the next scan
  *total = tot;
  return pre + x;
}

}  // namespace scan
}  // namespace xsknf_gpu
