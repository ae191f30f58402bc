// lb_stage.h -- the load balancer object's pinned buffers ("stages"), shared by
// the translation units that send host data down a stream: lb_remove_device.hip
// (key lists, the list drain's set), which owns them, and lb_backends_device.hip
// (an update's entries or tables).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

struct xsknf_gpu_lb;

namespace xsknf_gpu {

struct LbStage {
  void *host;      // pinned, cap bytes
  void *dev;       // cap bytes
  size_t cap;
  hipEvent_t done;
  bool recorded;   // `done` lies on a stream
};

// The smallest stage of at least `bytes` bytes that its stream has passed, or a
// new one (lb_remove_device.hip).  The user records st->done behind its last
// use and sets st->recorded.  0, -ENOMEM or -EIO.
int lb_stage_acquire(xsknf_gpu_lb *lb, size_t bytes, LbStage **out);

}  // namespace xsknf_gpu
