// kernel_lb_stamp.h -- rule 11 on the parallel path: the last-seen stamps of a
// batch of the load balancer or the lbfw NF (include/xsknf_gpu.h, "ageing").
// Part of lb_device.hip's translation unit, beside kernel_lb.h, whose four
// kernels stay as they are: an object without ageing launches exactly those
// four, an object with ageing launches lb_stamp between lb_commit and
// lb_ordered.
//
// It is a launch of its own for the reason lb_commit is: behind lb_commit every
// new session lies in its slot, and no lookup sees a half-written one.  It comes
// BEFORE lb_ordered because lb_ordered, the last launch, adds the new keys to the
// session count that parallel_path() reads: in front of it lb_stamp takes the
// same decision as lb_apply and lb_commit did.  A batch that stood down is
// stamped by lb_ordered itself: lb::frame() and lb::put() stamp through
// Tables::stamps (lb_table.h), the host model's own code.
//
// One lane per frame:
//   HIT       (rule 7) stores the clock to the stamp of the slot state[f] holds.
//             No session moves inside a batch, so the slot is still the key's.
//   creator   of a staged key -- the frame whose index the staging slot holds
//             after lb_propose, as in lb_commit -- looks the key up in the
//             session table, where lb_commit has just stored it, and stamps its
//             slot: the forward key, the backward key, or both (rule 9).
//   others    nothing.  A frame that took its session from staging uses a
//             session of this batch, and its creator stamps the same value; a
//             frame that PASSes, drops or that the ACL decided (kDone) stamps
//             nothing by rule 11.
//
// Why no order among lanes is needed: every stamp of one batch is the same value,
// the clock word as the stream left it before the batch (xsknf_gpu_lb_clock is a
// write in stream order, so no launch of the batch runs beside one).  Several
// lanes that store to one word store the same bits, and which of them is last
// cannot show.  The stores are plain 4-byte vector stores; nothing in the batch
// reads a stamp.  On the parallel path a failed insert does not exist (the batch
// would have stood down), so "a failed insert stamps nothing" is lb_ordered's.
#pragma once
#include "kernel_lb.h"

namespace xsknf_gpu {
namespace lbk {

__global__ __launch_bounds__(kThreads) void lb_stamp(const Args a) {
  if (!parallel_path(a)) return;
  const uint32_t now = *a.t.clock;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t f = blockIdx.x * kThreads + threadIdx.x; f < a.n; f += stride) {
    const uint32_t st = a.state[f], cls = st & kClassMask;
    if (cls == kHit) {
      a.t.stamps[st & 0xffffff] = now;
      continue;
    }
    if (cls != kProposer) continue;
    const uint32_t *r = a.prop + f * kPropWords;
    if (a.staging[r[kSlotS]] == enc(static_cast<uint32_t>(f), 0)) {
      const uint32_t s = lb::find(a.t.keys, a.t.slots, lb::Key{r[kSa], r[kSb], r[kSc], r[kProto]});
      if (s != lb::kNone) a.t.stamps[s] = now;   // (always found: lb_commit stored it)
    }
    if (a.staging[r[kSlotB]] == enc(static_cast<uint32_t>(f), 1)) {
      const uint32_t s = lb::find(a.t.keys, a.t.slots, lb::Key{r[kBa], r[kBb], r[kBc], r[kProto]});
      if (s != lb::kNone) a.t.stamps[s] = now;
    }
  }
}

}  // namespace lbk
}  // namespace xsknf_gpu
