// desc_rules.h -- what a descriptor means, stated once for every C++ file, host
// or device: where its bytes start, whether they lie in a UMEM, which 16-byte
// chunks hold them, and the address that marks it outside every UMEM.
// (xsknf_rt.c is plain C and keeps its addr_offset; xsknf_amd/frames.py, shard.py
// and tests/*_cases.py restate the rules on purpose: the tests' models.)
// Plain C++17, no GPU call: shard_plan.cpp and forward_host.cpp build with g++.
#pragma once
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

#if defined(__HIPCC__)
#define XSKNF_HD __host__ __device__
#else
#define XSKNF_HD
#endif

namespace xsknf_gpu {

// An address past any UMEM, for a frame outside the root's UMEM in the
// descriptors its shard receives: verdict -1, no bytes.
constexpr uint64_t kOutOfRange = 1ull << 47;

// The frame's first byte in its UMEM: xsknf_rt.c addr_offset
// (xsk_umem__add_offset_to_addr, src/xsknf.c:509); identity in aligned mode.
XSKNF_HD inline uint64_t desc_offset(uint64_t addr) {
  return (addr & XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK) + (addr >> XSKNF_GPU_UNALIGNED_BUF_OFFSET_SHIFT);
}

// [off, off + len) lies inside a UMEM of `size` bytes (no sum that can wrap).
// The reference indexes the UMEM with what the kernel's rx validation let
// through (src/xsknf.c:510, :565-566); here the descriptors are the caller's,
// and any other one is never read or written: verdict -1, skipped by the copies.
XSKNF_HD inline bool in_umem(uint64_t off, uint32_t len, uint64_t size) {
  return off <= size && len <= size - off;
}

// The 16-byte aligned chunks of memory that hold `len` > 0 bytes from byte
// address `start` on, the first at start & ~15: the reference walks a frame 2
// bytes at a time (checksummer_user.c:94-102) and copies it with one memcpy
// (src/xsknf.c:565), the kernels move chunks.  Callers give len == 0 no chunk.
XSKNF_HD inline uint64_t chunk_count(uint64_t start, uint32_t len) {
  return ((start & 15) + len + 15) >> 4;
}

// Their bytes: a frame's slot in its shard's packed buffer (xsknf_gpu_shard_pack_plan).
XSKNF_HD inline uint64_t slot_bytes(uint64_t start, uint32_t len) {
  return 16 * chunk_count(start, len);
}

}  // namespace xsknf_gpu
