// kernel_macswap.h -- the macswap NF's device pass.  Part of
// macswap_device.hip's translation unit (none of checksummer.hip's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "desc_rules.h"

namespace xsknf_gpu {
namespace macswap {

constexpr int kThreads = 256;       // frames per block and step: one lane per frame
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

struct Args {
  uint8_t *umem;
  uint64_t umem_size;
  const uint4 *descs;
  int32_t *verdicts;
  uint32_t n;
  int32_t fwd_verdict;   // rule 3's value for every frame that passes rules 0 and 1
  uint32_t swap;         // 0: a double swap, the frames are neither read nor written
};

// The low word of hi:lo shifted right by r bytes, r = 0..3.
__device__ __forceinline__ uint32_t bytes_from(uint32_t lo, uint32_t hi, uint32_t r) {
  return static_cast<uint32_t>((static_cast<uint64_t>(hi) << 32 | lo) >> (8 * r));
}

__device__ __forceinline__ void st8(uint8_t *p, uint32_t v) { *p = static_cast<uint8_t>(v); }
__device__ __forceinline__ void st16(uint8_t *p, uint32_t v) { *reinterpret_cast<uint16_t *>(p) = static_cast<uint16_t>(v); }
__device__ __forceinline__ void st32(uint8_t *p, uint32_t v) { *reinterpret_cast<uint32_t *>(p) = v; }

// Rule 2 for the 12 bytes at f = umem + off (include/xsknf_gpu.h, the store
// contract): read as the 3 (f 4-byte aligned) or 4 aligned words that hold
// them, each with a byte of [off, off + 12); stored as naturally aligned
// pieces that all lie inside [off, off + 12), by f's alignment r = off & 3
// (umem is 16-byte aligned):
//   r = 0   dword  dword  dword
//   r = 1   byte   short  dword  dword  byte
//   r = 2   short  dword  dword  short
//   r = 3   byte   dword  dword  short  byte
// A byte before off or from off + 12 on is never part of a store: a neighbour
// that shares a word with this frame is written by its own lane alone.
__device__ __forceinline__ void swap_macs(uint8_t *f) {
  const uint32_t r = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(f)) & 3;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(f - r);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
  const uint32_t w3 = r ? w[3] : 0;   // (holds f[11] for r > 0; past the frame's words for r == 0)
  // the old bytes 0..3, 4..7, 8..11 and the new ones: 6..9, 10 11 0 1, 2..5
  const uint32_t x0 = bytes_from(w0, w1, r), x1 = bytes_from(w1, w2, r), x2 = bytes_from(w2, w3, r);
  const uint32_t y0 = x1 >> 16 | x2 << 16, y1 = x2 >> 16 | x0 << 16, y2 = x0 >> 16 | x1 << 16;
  switch (r) {
    case 0:
      st32(f, y0);
      st32(f + 4, y1);
      st32(f + 8, y2);
      break;
    case 1:
      st8(f, y0);
      st16(f + 1, y0 >> 8);
      st32(f + 3, y0 >> 24 | y1 << 8);
      st32(f + 7, y1 >> 24 | y2 << 8);
      st8(f + 11, y2 >> 24);
      break;
    case 2:
      st16(f, y0);
      st32(f + 2, y0 >> 16 | y1 << 16);
      st32(f + 6, y1 >> 16 | y2 << 16);
      st16(f + 10, y2 >> 16);
      break;
    default:
      st8(f, y0);
      st32(f + 1, y0 >> 8 | y1 << 24);
      st32(f + 5, y1 >> 8 | y2 << 24);
      st16(f + 9, y2 >> 8);
      st8(f + 11, y2 >> 24);
      break;
  }
}

// One lane per frame; a block takes kThreads consecutive frames per step and
// every gridDim.x-th such tile.  Per frame: the 16-byte descriptor (coalesced),
// 12 or 16 bytes of the frame read and 12 written back -- one 64-byte sector,
// two where the 12 bytes straddle a sector's edge -- and the verdict as a
// coalesced 4-byte store: 44 to 48 bytes asked for, 16 + 64 + 64 + 4 = 148
// bytes of memory traffic for a frame in a line of its own.  With a double
// swap only the descriptor and the verdict move (20 bytes).  All plain cached
// accesses: the router and forwarder that follow read the same descriptors,
// verdicts and frames.  No LDS, no atomics, no block waits on another.
__global__ __launch_bounds__(kThreads) void macswap_pass(const Args a) {
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
    const uint4 d = a.descs[i];
    const uint64_t off = desc_offset(static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32);
    const uint32_t len = d.z;
    int32_t v = -1;
    if (in_umem(off, len, a.umem_size) && len >= 14) {   // rules 0, 1
      if (a.swap) swap_macs(a.umem + off);               // rule 2
      v = a.fwd_verdict;                                 // rule 3
    }
    a.verdicts[i] = v;
  }
}

}  // namespace macswap
}  // namespace xsknf_gpu
