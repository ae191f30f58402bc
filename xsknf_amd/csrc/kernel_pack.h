// kernel_pack.h -- the kernels of the multi-device calls (multi.hip): the
// per-shard counters xsknf_gpu_multi_counters reduces, the gather of a packed
// scatter on the root, and the root's apply of the records a return brings back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"
#include "checksummer_internal.h"
#include "desc_rules.h"

namespace xsknf_gpu {
namespace multi {

constexpr uint32_t kFingerprintMod = 65521;

// Per frame of one shard: [frames, bytes, drops, forwards, checks, weighted
// checks] -- the bytes over every descriptor's len (xsknf_amd/shard.py
// counters()), the checks over the frames of at least 42 bytes inside the span
// (the UDP check of an ihl-5 frame at +40, as bench.py check_fingerprint reads
// it), weighted by (global offset mod 65521) + 1 so that a check landing in
// another frame shows.  One wave per 64 frames, a block sum, one atomic per
// counter and block (vector atomics to device memory).
__global__ void __launch_bounds__(256) shard_counters(const uint8_t *umem, uint64_t span,
                                                      const xsknf_gpu_desc *descs, const int32_t *verdicts,
                                                      uint64_t n, uint64_t base, unsigned long long *out) {
  unsigned long long c[XSKNF_GPU_MULTI_COUNTERS] = {};
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const xsknf_gpu_desc d = descs[i];
    const int32_t v = verdicts[i];
    c[0] += 1;
    c[1] += d.len;
    c[2] += v == -1;
    c[3] += v >= 0;
    const uint64_t off = desc_offset(d.addr);
    // desc_rules.h in_umem(off, d.len, span), written out: the call costs 2 instructions and measured slower
    if (d.len >= 42 && off <= span && d.len <= span - off) {
      const unsigned long long ck = umem[off + 40] | static_cast<unsigned>(umem[off + 41]) << 8;
      c[4] += ck;
      c[5] += ck * ((off + base) % kFingerprintMod + 1);
    }
  }
  __shared__ unsigned long long red[XSKNF_GPU_MULTI_COUNTERS][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < XSKNF_GPU_MULTI_COUNTERS; ++k) {
    unsigned long long x = c[k];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) red[k][wv] = x;
  }
  __syncthreads();
  if (threadIdx.x < XSKNF_GPU_MULTI_COUNTERS) {
    const int k = threadIdx.x;
    atomicAdd(&out[k], red[k][0] + red[k][1] + red[k][2] + red[k][3]);
  }
}

// Root: copy frames [0, n) of one shard into its packed buffer.  Frame f's
// bytes lie in the 16-byte aligned chunks [src & ~15, round16(src + len)) of
// memory (src = its address) and go to the slot at dst & ~15 of the packed
// buffer, whose length is exactly those chunks (dst = src mod 16 + the slot's
// start): whole chunks move, and the bytes around the frame in its first and
// last chunk are copied with it into its own slot.  One wave per 64 frames:
// the tile's chunk counts are prefix-summed across the wave and the lanes deal
// the tile's chunks round robin (a 64-B frame is 4-5 chunks, a jumbo one 563).
// A chunk reaching past the UMEM's end is copied byte by byte.
__global__ void __launch_bounds__(256) pack_frames(const uint8_t *umem, uint64_t umem_size,
                                                   const xsknf_gpu_desc *orig, const xsknf_gpu_desc *packed,
                                                   uint64_t n, uint8_t *dst) {
  __shared__ uint32_t pre[4][65];
  __shared__ uint64_t src_of[4][64], dst_of[4][64];   // a frame's first chunk and its slot (read by any lane)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t tiles = (n + 63) / 64;
  for (uint64_t t = blockIdx.x * 4ull + wv; t < tiles; t += gridDim.x * 4ull) {
    const uint64_t f = t * 64 + lane;
    uint64_t s0 = 0, d0 = 0;   // the first chunk's address (absolute) and its slot offset in dst
    uint32_t nch = 0;
    if (f < n) {
      const xsknf_gpu_desc o = orig[f], q = packed[f];
      const uint64_t src = reinterpret_cast<uintptr_t>(umem) + desc_offset(o.addr);
      if (q.addr != kOutOfRange && o.len > 0) {
        s0 = src & ~15ull;
        d0 = q.addr & ~15ull;
        nch = static_cast<uint32_t>(chunk_count(src, o.len));
      }
    }
    // inclusive scan of the chunk counts over the wave
    uint32_t x = nch;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    pre[wv][lane + 1] = x;
    if (lane == 0) pre[wv][0] = 0;
    src_of[wv][lane] = s0;
    dst_of[wv][lane] = d0;
    __builtin_amdgcn_wave_barrier();   // (one wave's LDS accesses complete in order)
    const uint32_t total = __shfl(x, 63);
    const uint64_t begin = reinterpret_cast<uintptr_t>(umem), end = begin + umem_size;
    for (uint32_t k = lane; k < total; k += 64) {
      // the frame j of the tile whose chunks hold chunk k: pre[j] <= k < pre[j + 1]
      int lo = 0, hi = 63;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[wv][mid] <= k) lo = mid; else hi = mid - 1;
      }
      const uint32_t c = k - pre[wv][lo];
      // (from LDS, not by a lane shuffle: the loop's last round leaves lanes
      // inactive, and a shuffle reads nothing from an inactive lane)
      const uint64_t sa = src_of[wv][lo] + 16ull * c, da = dst_of[wv][lo] + 16ull * c;
      if (sa >= begin && sa + 16 <= end) {
        *reinterpret_cast<uint4 *>(dst + da) = *reinterpret_cast<const uint4 *>(sa);
      } else {   // a chunk reaching before the UMEM's first byte or past its last
        for (uint64_t b = sa > begin ? sa : begin; b < sa + 16 && b < end; ++b)
          dst[da + (b - sa)] = *reinterpret_cast<const uint8_t *>(b);
      }
    }
    __builtin_amdgcn_wave_barrier();   // pre[wv] is rewritten by the next tile
  }
}

// Root: the returned records / verdicts of the whole batch, in place: a record
// (make_record(u, check), checksummer_internal.h) writes the check's two bytes, low
// byte first, at the frame's offset u + 6 (checksummer_user.c:108) and becomes
// the forward verdict (:110-111); any other value is already the verdict.
__global__ void __launch_bounds__(256) apply_records(uint8_t *umem, const xsknf_gpu_desc *orig, int32_t *verdicts,
                                                     uint64_t n, int32_t fwd) {
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
    const uint32_t r = static_cast<uint32_t>(verdicts[i]);
    if (!xsknf_gpu::is_record(r)) continue;
    uint8_t *p = umem + desc_offset(orig[i].addr) + xsknf_gpu::record_check_offset(r);
    const uint16_t c = xsknf_gpu::record_check(r);
    p[0] = static_cast<uint8_t>(c);
    p[1] = static_cast<uint8_t>(c >> 8);
    verdicts[i] = fwd;
  }
}

}  // namespace multi
}  // namespace xsknf_gpu
