// lb_backends_device.hip -- how an update of the load balancer's services and
// backends reaches the device copy (include/xsknf_gpu.h
// xsknf_gpu_lb_backends_update; the host pass is lb.cpp's, which calls the
// functions below: lb_table.h declares them).
//
// lb.cpp rebuilds both tables from the edited list and hands over either the
// service slots and backend entries that changed, as 32-byte LbEntry, or the
// tables whole (kernel_lb_backends.h says when).  Both lie in a pinned buffer
// that belongs to the object (a stage of lb_stage.h, shared with the removals),
// so the call returns while the stream still has to read them:
//   entries  one async copy into the stage's device buffer, then one launch that
//            stores 16 B per entry into the region;
//   table    one async copy over the region, no launch.
// An event recorded behind them tells a later call whether the stage is free.
//
// The region: creation's allocation has room for creation's backends only, so
// the first update allocates svc_slots + XSKNF_GPU_LB_MAX_BACKENDS 16-byte
// entries (2.03 MiB), adds them to device_bytes, sends the tables whole and
// points d_svc / d_bk there -- on the host at once, which is what the NEXT
// batch's kernel arguments are made from; batches enqueued earlier hold the old
// addresses, and the old tables stay allocated and untouched until _destroy.
// A translation unit of its own: none of the other kernels is rebuilt for it.
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_lb_backends.h"
#include "lb_stage.h"

namespace xsknf_gpu {

namespace {

static_assert(sizeof(LbEntry) == 32 && sizeof(lb::Service) == 16 && sizeof(lb::Backend) == 16,
              "lb_backends_scatter reads an entry as two 16-byte words and stores one");

int hip_rc(hipError_t e, const char *where) {
  set_error(e, where);
  return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

size_t region_entries(const xsknf_gpu_lb *lb) { return static_cast<size_t>(lb->svc_slots) + XSKNF_GPU_LB_MAX_BACKENDS; }

}  // namespace

int lb_backends_prepare(xsknf_gpu_lb *lb, size_t bytes, LbStage **stage_out, void **host_out) {
  if (bytes > sizeof(uint4) * region_entries(lb) * 2) return -EINVAL;   // (lb.cpp asks for what it sends)
  if (!lb->d_region) {
    const size_t rb = sizeof(uint4) * region_entries(lb);
    void *d = nullptr;
    const hipError_t e = hipMalloc(&d, rb);
    if (e != hipSuccess) return hip_rc(e, "load balancer services region");
    lb->d_region = d;
    lb->device_bytes += rb;
  }
  const int rc = lb_stage_acquire(lb, bytes, stage_out);
  if (rc) return rc;
  *host_out = (*stage_out)->host;
  return 0;
}

int lb_backends_enqueue(xsknf_gpu_lb *lb, LbStage *stage, uint32_t entries, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (entries == 0) {
    const size_t bytes = sizeof(uint4) * (static_cast<size_t>(lb->svc_slots) + lb->backends);
    if (bytes > stage->cap || lb->backends > XSKNF_GPU_LB_MAX_BACKENDS) return -EINVAL;
    e = hipMemcpyAsync(lb->d_region, stage->host, bytes, hipMemcpyHostToDevice, s);
    lb->d_svc = static_cast<lb::Service *>(lb->d_region);
    lb->d_bk = reinterpret_cast<lb::Backend *>(lb->d_svc + lb->svc_slots);
  } else {
    const size_t bytes = sizeof(LbEntry) * static_cast<size_t>(entries);
    if (bytes > stage->cap || static_cast<void *>(lb->d_svc) != lb->d_region) return -EINVAL;
    e = hipMemcpyAsync(stage->dev, stage->host, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      lb_backends::Args a;
      a.entries = static_cast<const uint4 *>(stage->dev);
      a.region = static_cast<uint4 *>(lb->d_region);
      a.n = entries;
      a.limit = static_cast<uint32_t>(region_entries(lb));
      const uint32_t tiles = entries / lb_backends::kThreads + (entries % lb_backends::kThreads != 0);
      const dim3 grid(tiles < static_cast<uint32_t>(lb_backends::kMaxBlocks) ? tiles : lb_backends::kMaxBlocks);
      hipLaunchKernelGGL(lb_backends::lb_backends_scatter, grid, dim3(lb_backends::kThreads), 0, s, a);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipEventRecord(stage->done, s);
  stage->recorded = true;   // (also after an error: the copy may be under way)
  if (e != hipSuccess) return hip_rc(e, "load balancer backends update");
  return 0;
}

int lb_backends_release(xsknf_gpu_lb *lb) {
  if (!lb->d_region) return 0;
  const hipError_t e = hipFree(lb->d_region);
  lb->d_region = nullptr;
  if (e != hipSuccess) return hip_rc(e, "load balancer release");
  return 0;
}

}  // namespace xsknf_gpu
