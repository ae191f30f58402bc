// kernel_firewall.h -- the firewall's device lookup.  Part of
// firewall_device.hip's translation unit (none of checksummer.hip's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acl_table.h"
#include "desc_rules.h"
#include "ld_bytes.h"

namespace xsknf_gpu {
namespace firewall {

constexpr int kThreads = 256;       // frames per block and step: one lane per frame
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

struct Args {
  const uint8_t *umem;
  uint64_t umem_size;
  const uint4 *descs;
  const AclKey *keys;
  const int32_t *actions;
  int32_t *verdicts;
  uint32_t n;
  uint32_t slots;
};

// Rules 0-7 of include/xsknf_gpu.h for one frame.
__device__ __forceinline__ int32_t verdict_of(const Args &a, uint64_t addr, uint32_t len) {
  const uint64_t off = desc_offset(addr);
  if (!in_umem(off, len, a.umem_size) || len < 14) return -1;              // rules 0, 1
  if (len < 34) {   // rules 2, 3: only the ethertype counts (f[12..13]; the frame may end there)
    return (ld_bytes(a.umem, off + 12, 2) & 0xffff) != 0x0008 ? 0 : -1;
  }
  // f[12..15] (the ethertype and the ihl byte), f[23], f[26..33]: all inside the
  // frame, loaded together before any of them is looked at
  const uint32_t e = ld_bytes(a.umem, off + 12, 4);
  const uint32_t proto = ld_bytes(a.umem, off + 23, 1) & 0xff;
  const uint32_t sa = ld_bytes(a.umem, off + 26, 4), da = ld_bytes(a.umem, off + 30, 4);
  if ((e & 0xffff) != 0x0008) return 0;                                    // rule 2
  const uint32_t next = 14 + 4 * ((e >> 16) & 15);                         // rule 4
  if (proto != 6 && proto != 17) return 0;                                 // rule 5
  if (next + (proto == 6 ? 20u : 8u) > len) return -1;
  const uint32_t ports = ld_bytes(a.umem, off + next, 4);                  // rule 6
  return acl_lookup(a.keys, a.actions, a.slots, sa, da, ports, proto);     // rule 7
}

// One lane per frame; a block takes kThreads consecutive frames per step and
// every gridDim.x-th such tile.  Per frame: the 16-byte descriptor (coalesced),
// 4 to 9 aligned words of the frame's bytes 12..33 and next..next+3 -- one or
// two 64-byte sectors for ihl 5, whatever the frame's phase -- then one 16-byte
// key slot per probe and the 4-byte action on a hit, and the verdict as a
// coalesced 4-byte store.  All plain cached accesses: the table is reused from
// frame to frame (L2, then the Infinity Cache), and the router and forwarder
// that follow read the same descriptors, verdicts and frames.  Lanes whose
// verdict the parse decides skip the probe loop; the loop itself ends after at
// most `slots` probes whatever the table holds.  No LDS, no atomics, no block
// waits on another.
__global__ __launch_bounds__(kThreads) void firewall_lookup(const Args a) {
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t f = blockIdx.x * kThreads + threadIdx.x; f < a.n; f += stride) {
    const uint4 d = a.descs[f];
    a.verdicts[f] = verdict_of(a, static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32, d.z);
  }
}

}  // namespace firewall
}  // namespace xsknf_gpu
