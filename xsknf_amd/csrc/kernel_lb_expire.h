// kernel_lb_expire.h -- ending the idle flows of the load balancer's device table
// (include/xsknf_gpu.h xsknf_gpu_lb_sessions_expire).  Part of
// lb_remove_device.hip's translation unit, beside lb_drain (kernel_lb_remove.h),
// whose Args, flush() and four compaction launches it uses.
//
//   lb_expire  one lane per slot, grid-stride.  A live slot whose stamp is idle,
//              (uint32_t)(clock - stamp) > max_idle, derives its partner key from
//              its own key and value (lb::partner_key), probes for it
//              (lb::find) and checks it (lb::is_partner).  If there is a checked
//              partner and that partner is not idle, the slot stays: a flow
//              leaves whole or not at all.  Otherwise the lane stores the
//              tombstone to its own slot's p and counts it.  A lane only ever
//              buries its OWN slot, so no slot has two claimants and a plain
//              store does (lb_drain's case, not lb_remove_keys').
//
// Why one launch gives the set semantics -- every decision as if taken on the
// table as it stood -- whatever the lane order.  Everything a lane reads to
// decide is written by no lane of the launch: the stamps, the clock, a slot's
// key words a, b, c and its value.  Only p changes, and only to the tombstone.
// So the one thing a lane can see differently from "the table as it stood" is
// its partner's p: lb::find walks over a tombstone, the lane finds no partner
// and decides alone -- it is idle, so it goes.  But the partner's own lane buried
// that slot only after finding both halves idle (is_partner is symmetric in the
// pair, and idle() reads words nobody writes), which is the decision this lane
// would have taken with the partner still in place.  A stale p from this CU's
// L1 can only show a buried partner as live; its stamp then says idle all the
// same.  A tombstone in a probe chain never ends the chain early (p != 0), so no
// lookup of a third key changes either.
//
// Counting follows flush(): each lane adds to one LDS word, the block's first
// lane issues the three atomics.  Nothing here waits for another lane.
#pragma once
#include "kernel_lb_remove.h"

namespace xsknf_gpu {
namespace lbr {

__global__ __launch_bounds__(kThreads) void lb_expire(const Args a) {
  __shared__ uint32_t removed;
  if (threadIdx.x == 0) removed = 0;
  __syncthreads();
  const uint32_t now = *a.clock;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.slots; s += stride) {
    const lb::Key k = a.keys[s];
    if (!lb::live(k) || !lb::idle(now, a.stamps[s], a.max_idle)) continue;
    const lb::Val v = a.vals[s];
    const lb::Key pk = lb::partner_key(k, v);
    const uint32_t ps = lb::find(a.keys, a.slots, pk);
    if (ps != lb::kNone && lb::is_partner(pk, a.vals[ps], k, v) && !lb::idle(now, a.stamps[ps], a.max_idle)) continue;
    a.keys[s].p = lb::kTombstoneP;
    atomicAdd(&removed, 1u);
  }
  flush(a, &removed);
}

}  // namespace lbr
}  // namespace xsknf_gpu
