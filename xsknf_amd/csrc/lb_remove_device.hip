// lb_remove_device.hip -- removing sessions from the load balancer's device table
// (include/xsknf_gpu.h xsknf_gpu_lb_sessions_remove, _drain_backend,
// _drain_backends, _sessions_expire, _sessions_clear; lb.cpp validates and calls
// the functions below, which lb_table.h declares; the kernels are
// kernel_lb_remove.h's, kernel_lb_drain_list.h's and kernel_lb_expire.h's).
//
// Everything is enqueued on the caller's stream and nothing is read back:
//   remove  [result zeroed] one async copy of the key list, 16 B per key, from a
//           pinned buffer into its device twin, lb_remove_keys, and the four
//           compaction launches, which return at once unless the tombstones
//           have passed the bound
//   drain   [result zeroed] lb_drain over the slots and the same four launches
//   drain a list  [result zeroed] one async copy of the listed backends as a set,
//           8 B per slot, lb_drain_list over the slots and the same four launches
//   expire  [result zeroed] lb_expire over the slots and the same four launches
//   clear   one memset over the keys, the values and the two counters
//
// The caller's key list is host memory that the call must not reference after it
// returns, so it is copied into a pinned buffer that belongs to the object (a
// "stage", as for the ACL's updates: acl_update_device.hip).  An event recorded
// behind the launches tells a later call whether the stage is free again
// (hipEventQuery: the host never waits); a call that finds no free stage of its
// size makes a new one, so the buffers grow with the number of calls in flight
// and are released by xsknf_gpu_lb_destroy.
//
// The spare table a compaction rebuilds into -- as large as the session table's
// keys and values -- is allocated by the first removal and is part of
// device_bytes from then on.  It needs no contents: lb_compact_zero clears it
// when it is used.  With ageing the spare table has stamps of its own, 4 B per
// slot, allocated with it or, where it came first, by _aging_enable.  A
// translation unit of its own: none of the other kernels is
// rebuilt for it.
#include <errno.h>
#include <string.h>

#include <new>
#include <vector>

#include "checksummer_internal.h"
#include "kernel_lb_drain_list.h"
#include "kernel_lb_expire.h"
#include "kernel_lb_remove.h"
#include "lb_stage.h"

struct xsknf_gpu_lb_staging {
  std::vector<xsknf_gpu::LbStage *> stages;
};

namespace xsknf_gpu {

namespace {

static_assert(sizeof(struct xsknf_gpu_lb_session_key) == 16, "lb_remove_keys reads a listed key as one 16-byte word");

int hip_rc(hipError_t e, const char *where) {
  set_error(e, where);
  return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

int stage_free(LbStage *st) {
  int rc = 0;
  hipError_t e = hipEventDestroy(st->done);
  if (e != hipSuccess) rc = hip_rc(e, "load balancer removal release");
  e = hipHostFree(st->host);
  if (e != hipSuccess) rc = hip_rc(e, "load balancer removal release");
  e = hipFree(st->dev);
  if (e != hipSuccess) rc = hip_rc(e, "load balancer removal release");
  delete st;
  return rc;
}

}  // namespace

// The smallest stage of at least `bytes` bytes that its stream has passed, or a new one.
int lb_stage_acquire(xsknf_gpu_lb *lb, size_t bytes, LbStage **out) {
  if (!lb->staging && !(lb->staging = new (std::nothrow) xsknf_gpu_lb_staging())) return -ENOMEM;
  LbStage *best = nullptr;
  for (LbStage *st : lb->staging->stages) {
    if (st->cap < bytes || (best && best->cap <= st->cap)) continue;
    if (st->recorded) {
      const hipError_t e = hipEventQuery(st->done);
      if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        continue;
      }
      if (e != hipSuccess) return hip_rc(e, "load balancer removal");
      st->recorded = false;
    }
    best = st;
  }
  if (!best) {
    size_t cap = 4096;   // powers of two up to 1 MiB, then whole MiB
    while (cap < bytes && cap < (1u << 20)) cap *= 2;
    if (cap < bytes) cap = (bytes + (1u << 20) - 1) & ~static_cast<size_t>((1u << 20) - 1);
    LbStage *st = new (std::nothrow) LbStage();
    if (!st) return -ENOMEM;
    try {
      lb->staging->stages.reserve(lb->staging->stages.size() + 1);
    } catch (const std::bad_alloc &) {
      delete st;
      return -ENOMEM;
    }
    st->cap = cap;
    hipError_t e = hipHostMalloc(&st->host, cap, hipHostMallocDefault);
    if (e != hipSuccess) {
      delete st;
      return hip_rc(e, "load balancer removal buffer");
    }
    e = hipMalloc(&st->dev, cap);
    if (e != hipSuccess) {
      (void)hipHostFree(st->host);
      delete st;
      return hip_rc(e, "load balancer removal buffer");
    }
    e = hipEventCreateWithFlags(&st->done, hipEventDisableTiming);
    if (e != hipSuccess) {
      (void)hipFree(st->dev);
      (void)hipHostFree(st->host);
      delete st;
      return hip_rc(e, "load balancer removal buffer");
    }
    lb->staging->stages.push_back(st);
    best = st;
  }
  *out = best;
  return 0;
}

int lb_want_spare(xsknf_gpu_lb *lb) {
  if (!lb->d_spare) {
    const size_t bytes = (sizeof(lb::Key) + sizeof(lb::Val)) * static_cast<size_t>(lb->slots);
    void *d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return hip_rc(e, "load balancer spare table");
    lb->d_spare = static_cast<lb::Key *>(d);
    lb->device_bytes += bytes;
  }
  if (lb->d_stamps && !lb->d_spare_stamps) {
    const size_t bytes = sizeof(uint32_t) * static_cast<size_t>(lb->slots);
    void *d = nullptr;
    const hipError_t e = hipMalloc(&d, bytes);
    if (e != hipSuccess) return hip_rc(e, "load balancer spare stamps");
    lb->d_spare_stamps = static_cast<uint32_t *>(d);
    lb->device_bytes += bytes;
  }
  return 0;
}

namespace {

int want_spare(xsknf_gpu_lb *lb) { return lb_want_spare(lb); }

lbr::Args table_args(const xsknf_gpu_lb *lb, uint64_t *result_dev) {
  lbr::Args a;
  memset(&a, 0, sizeof(a));
  a.keys = lb->d_keys;
  a.vals = lb->d_vals;
  a.spare_keys = lb->d_spare;
  a.spare_vals = reinterpret_cast<lb::Val *>(lb->d_spare + lb->slots);
  a.count = lb->d_count;
  a.result = reinterpret_cast<unsigned long long *>(result_dev);
  a.slots = lb->slots;
  a.stamps = lb->d_stamps;
  a.spare_stamps = lb->d_spare_stamps;
  a.clock = lb->d_clock;
  return a;
}

dim3 grid_for(uint32_t items) {
  const uint32_t tiles = items / lbr::kThreads + (items % lbr::kThreads != 0);   // (no sum that can wrap)
  return dim3(tiles < static_cast<uint32_t>(lbr::kMaxBlocks) ? tiles : lbr::kMaxBlocks);
}

// Behind a removal: the four launches that rebuild the table if it is due.
void enqueue_compaction(const lbr::Args &a, hipStream_t s) {
  const dim3 grid = grid_for(a.slots), block(lbr::kThreads);
  hipLaunchKernelGGL(lbr::lb_compact_zero, grid, block, 0, s, a);
  hipLaunchKernelGGL(lbr::lb_compact_move, grid, block, 0, s, a);
  hipLaunchKernelGGL(lbr::lb_compact_back, grid, block, 0, s, a);
  hipLaunchKernelGGL(lbr::lb_compact_done, dim3(1), dim3(64), 0, s, a);
}

}  // namespace

int lb_remove_enqueue(xsknf_gpu_lb *lb, const void *keys, uint32_t n, bool pair, uint64_t *result_dev, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  LbStage *st = nullptr;
  const size_t bytes = sizeof(struct xsknf_gpu_lb_session_key) * static_cast<size_t>(n);
  if (n) {
    int rc = want_spare(lb);
    if (!rc) rc = lb_stage_acquire(lb, bytes, &st);
    if (rc) return rc;
  }
  hipError_t e = result_dev ? hipMemsetAsync(result_dev, 0, sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT, s) : hipSuccess;
  if (e != hipSuccess) return hip_rc(e, "load balancer removal");
  if (n == 0) return 0;
  memcpy(st->host, keys, bytes);
  e = hipMemcpyAsync(st->dev, st->host, bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_rc(e, "load balancer removal copy");
  lbr::Args a = table_args(lb, result_dev);
  a.list = static_cast<const uint4 *>(st->dev);
  a.n = n;
  a.pair = pair;
  hipLaunchKernelGGL(lbr::lb_remove_keys, grid_for(n), dim3(lbr::kThreads), 0, s, a);
  enqueue_compaction(a, s);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(st->done, s);
  st->recorded = true;   // (also after an error: the copy may be under way)
  if (e != hipSuccess) return hip_rc(e, "load balancer removal");
  return 0;
}

int lb_drain_enqueue(xsknf_gpu_lb *lb, uint32_t addr, uint32_t port, uint32_t proto, uint64_t *result_dev, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = want_spare(lb);
  if (rc) return rc;
  hipError_t e = result_dev ? hipMemsetAsync(result_dev, 0, sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT, s) : hipSuccess;
  if (e != hipSuccess) return hip_rc(e, "load balancer drain");
  lbr::Args a = table_args(lb, result_dev);
  a.addr = addr;
  a.port = port;
  a.proto = proto;
  hipLaunchKernelGGL(lbr::lb_drain, grid_for(a.slots), dim3(lbr::kThreads), 0, s, a);
  enqueue_compaction(a, s);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_rc(e, "load balancer drain");
  return 0;
}

int lb_drain_list_enqueue(xsknf_gpu_lb *lb, const void *set, uint32_t set_slots, uint64_t *result_dev, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  LbStage *st = nullptr;
  const size_t bytes = sizeof(lb::IdSlot) * static_cast<size_t>(set_slots);
  if (set_slots) {
    int rc = want_spare(lb);
    if (!rc) rc = lb_stage_acquire(lb, bytes, &st);
    if (rc) return rc;
  }
  hipError_t e = result_dev ? hipMemsetAsync(result_dev, 0, sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT, s) : hipSuccess;
  if (e != hipSuccess) return hip_rc(e, "load balancer list drain");
  if (set_slots == 0) return 0;
  memcpy(st->host, set, bytes);
  e = hipMemcpyAsync(st->dev, st->host, bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_rc(e, "load balancer list drain copy");
  lbr::ListArgs a;
  a.t = table_args(lb, result_dev);
  a.set = static_cast<const lb::IdSlot *>(st->dev);
  a.set_slots = set_slots;
  hipLaunchKernelGGL(lbr::lb_drain_list, grid_for(a.t.slots), dim3(lbr::kThreads), 0, s, a);
  enqueue_compaction(a.t, s);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(st->done, s);
  st->recorded = true;   // (also after an error: the copy may be under way)
  if (e != hipSuccess) return hip_rc(e, "load balancer list drain");
  return 0;
}

int lb_expire_enqueue(xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result_dev, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = want_spare(lb);
  if (rc) return rc;
  hipError_t e = result_dev ? hipMemsetAsync(result_dev, 0, sizeof(uint64_t) * XSKNF_GPU_LB_REMOVE_RESULT, s) : hipSuccess;
  if (e != hipSuccess) return hip_rc(e, "load balancer expire");
  lbr::Args a = table_args(lb, result_dev);
  a.max_idle = max_idle;
  hipLaunchKernelGGL(lbr::lb_expire, grid_for(a.slots), dim3(lbr::kThreads), 0, s, a);
  enqueue_compaction(a, s);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_rc(e, "load balancer expire");
  return 0;
}

int lb_clear_enqueue(xsknf_gpu_lb *lb, void *stream) {
  // keys, values and the 16 bytes behind them (lb.cpp's one allocation): the count and the tombstones
  const size_t bytes = (sizeof(lb::Key) + sizeof(lb::Val)) * static_cast<size_t>(lb->slots) + 16;
  const hipError_t e = hipMemsetAsync(lb->d_keys, 0, bytes, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_rc(e, "load balancer sessions_clear");
  return 0;
}

int lb_remove_release(xsknf_gpu_lb *lb) {
  int rc = 0;
  if (lb->staging) {
    for (LbStage *st : lb->staging->stages) {
      const int r = stage_free(st);
      if (r) rc = r;
    }
    delete lb->staging;
    lb->staging = nullptr;
  }
  if (lb->d_spare) {
    const hipError_t e = hipFree(lb->d_spare);
    if (e != hipSuccess) rc = hip_rc(e, "load balancer release");
    lb->d_spare = nullptr;
  }
  if (lb->d_spare_stamps) {
    const hipError_t e = hipFree(lb->d_spare_stamps);
    if (e != hipSuccess) rc = hip_rc(e, "load balancer release");
    lb->d_spare_stamps = nullptr;
  }
  return rc;
}

}  // namespace xsknf_gpu
