// kernel_acl_count.h -- an ACL's hit counters on the device (include/xsknf_gpu.h
// xsknf_gpu_acl_counters_*): the device-scope add, and how the hits of one wave
// reach the counters in lb_propose<true> of kernel_lb.h.  (The firewall's
// lookup, kernel_firewall_count.h, stages a block's repeated hits in LDS
// instead; the wave's combine is one of its A/B shapes.)  Device functions
// only, no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acl_table.h"

namespace xsknf_gpu {
namespace acl_count {

__device__ __forceinline__ void add_agent(uint64_t *p, uint64_t v) {
  __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// The hits of one wave, combined before they touch memory.  Called by lanes
// that run together (one program counter: the lanes of the wave that are at
// this call in this trip of their loop); a lane with hit == false, and a lane
// that is not here at all, is in nobody's group.  One round per DISTINCT slot
// among the hits: the first hit lane's slot is broadcast, a ballot finds the
// lanes that share it, their lens are summed lane by lane into a scalar, and
// the group's leader -- its lowest lane -- keeps the two sums.  Every lane is in
// one group, so the rounds read each len once: about 64 scalar steps per wave
// whether the hits name one slot or 64.  `todo` is a ballot, the same in every
// lane, so all of them stay to the last round.  Then the leaders add together:
// one packets and one bytes instruction per wave, one lane per distinct slot --
// one elephant flow costs its slot 2 adds per wave, not 128.
__device__ __forceinline__ void count_hits(AclCounter *counters, bool hit, uint32_t slot, uint32_t len) {
  const int lane = static_cast<int>(__lane_id());
  uint64_t todo = __ballot(hit);
  uint32_t packets = 0;
  uint64_t bytes = 0;
  while (todo) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
    const uint32_t s = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(slot), leader));
    const uint64_t group = __ballot(hit && slot == s);
    uint64_t sum = 0;
    for (uint64_t m = group; m; m &= m - 1) {
      const int l = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(m)) - 1);
      sum += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(len), l));
    }
    if (lane == leader) {
      packets = static_cast<uint32_t>(__popcll(group));
      bytes = sum;
    }
    todo &= ~group;
  }
  if (packets) {
    add_agent(&counters[slot].packets, packets);
    add_agent(&counters[slot].bytes, bytes);
  }
}

// Every hit lane adds for itself: the A/B twin (`make ab`, XSKNF_ACL_COUNT_SHAPE=naive), and what the
// firewall's staged lookup does for a slot's first hit in a block.
__device__ __forceinline__ void count_hits_naive(AclCounter *counters, bool hit, uint32_t slot, uint32_t len) {
  if (hit) {
    add_agent(&counters[slot].packets, 1);
    add_agent(&counters[slot].bytes, len);
  }
}

}  // namespace acl_count
}  // namespace xsknf_gpu
