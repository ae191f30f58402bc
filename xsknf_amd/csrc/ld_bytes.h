// ld_bytes.h -- a frame's bytes read as the aligned words that hold them: the
// device parse of the firewall (kernel_firewall.h) and the load balancer
// (kernel_lb.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xsknf_gpu {

// Bytes [pos, pos + nb), nb = 1..4, of the UMEM as a little-endian value in the
// result's low 8 nb bits (the bits above are other bytes: the caller masks).
// Read as the aligned 4-byte words that hold them -- the second only where the
// bytes cross into it -- so every word read holds a byte the frame owns.
__device__ __forceinline__ uint32_t ld_bytes(const uint8_t *umem, uint64_t pos, uint32_t nb) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(umem + (pos & ~3ull));
  const uint32_t r = static_cast<uint32_t>(pos) & 3;
  const uint32_t lo = w[0];
  if (r + nb <= 4) return lo >> (8 * r);
  return (lo >> (8 * r)) | (w[1] << (32 - 8 * r));   // r is 1..3 here
}

}  // namespace xsknf_gpu
