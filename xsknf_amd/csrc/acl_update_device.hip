// acl_update_device.hip -- how an ACL update reaches the device table
// (include/xsknf_gpu.h xsknf_gpu_acl_update; the host pass is acl.cpp's, which
// calls the functions below: acl_table.h declares them).
//
// acl.cpp hands over either the slots the update changed, each once and in its
// final state, as 24-byte records {slot, key, action}, or -- after a rebuild in
// place -- the whole table.  Both lie in a pinned host buffer that belongs to
// the ACL object (a "stage"), so the call returns while the stream still has to
// read them:
//   records  one async copy of 24 B per record into the stage's device buffer,
//            then one launch (kernel_acl_update.h) that stores 20 B per record
//            into the table;
//   table    one async copy of 20 B per slot over the table, no launch.
// An object with hit counters (xsknf_gpu_acl_counters_enable) adds to these:
//   records  16 B more stored for a slot whose record says its counters start
//            again (AclUpdateRec, kAclRecZero);
//   table    the new slots' old slots, 4 B per slot, copied behind the table,
//            and one launch that gathers the counters through that map into a
//            second array (20 B per slot read at most, 16 B written).  The two
//            arrays change roles on the host as the launch is enqueued: every
//            call on the object is made in order on one stream already.
// An event recorded behind them tells a later update whether the stage is free
// again (hipEventQuery: the host never waits); an update that finds no free
// stage of its size makes a new one, so the buffers grow with the number of
// updates in flight and are released by xsknf_gpu_acl_destroy.  A translation
// unit of its own: none of the checksummer's kernels is rebuilt for it.
#include <errno.h>

#include <new>
#include <vector>

#include "checksummer_internal.h"
#include "kernel_acl_update.h"

namespace xsknf_gpu {

struct AclStage {
  void *host;      // pinned, cap bytes
  void *dev;       // cap bytes, or NULL until records need it
  size_t cap;
  hipEvent_t done;
  bool recorded;   // `done` lies on a stream
};

}  // namespace xsknf_gpu

struct xsknf_gpu_acl_staging {
  std::vector<xsknf_gpu::AclStage *> stages;
};

namespace xsknf_gpu {

namespace {

int hip_rc(hipError_t e, const char *where) {
  set_error(e, where);
  return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

int stage_free(AclStage *st) {
  int rc = 0;
  hipError_t e = hipEventDestroy(st->done);
  if (e != hipSuccess) rc = hip_rc(e, "ACL update release");
  e = hipHostFree(st->host);
  if (e != hipSuccess) rc = hip_rc(e, "ACL update release");
  if (st->dev && (e = hipFree(st->dev)) != hipSuccess) rc = hip_rc(e, "ACL update release");
  delete st;
  return rc;
}

}  // namespace

int acl_stage_acquire(xsknf_gpu_acl *acl, size_t bytes, bool records, AclStage **stage_out, void **host_out) {
  if (!acl->staging && !(acl->staging = new (std::nothrow) xsknf_gpu_acl_staging())) return -ENOMEM;
  // the smallest stage that is large enough and that its stream has passed
  AclStage *best = nullptr;
  for (AclStage *st : acl->staging->stages) {
    if (st->cap < bytes || (best && best->cap <= st->cap)) continue;
    if (st->recorded) {
      const hipError_t e = hipEventQuery(st->done);
      if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        continue;
      }
      if (e != hipSuccess) return hip_rc(e, "ACL update");
      st->recorded = false;
    }
    best = st;
  }
  if (!best) {
    size_t cap = 4096;   // powers of two up to 1 MiB, then whole MiB
    while (cap < bytes && cap < (1u << 20)) cap *= 2;
    if (cap < bytes) cap = (bytes + (1u << 20) - 1) & ~static_cast<size_t>((1u << 20) - 1);
    AclStage *st = new (std::nothrow) AclStage();
    if (!st) return -ENOMEM;
    try {
      acl->staging->stages.reserve(acl->staging->stages.size() + 1);
    } catch (const std::bad_alloc &) {
      delete st;
      return -ENOMEM;
    }
    st->cap = cap;
    hipError_t e = hipHostMalloc(&st->host, cap, hipHostMallocDefault);
    if (e != hipSuccess) {
      delete st;
      return hip_rc(e, "ACL update buffer");
    }
    e = hipEventCreateWithFlags(&st->done, hipEventDisableTiming);
    if (e != hipSuccess) {
      (void)hipHostFree(st->host);
      delete st;
      return hip_rc(e, "ACL update buffer");
    }
    acl->staging->stages.push_back(st);
    best = st;
  }
  if (records && !best->dev) {
    const hipError_t e = hipMalloc(&best->dev, best->cap);
    if (e != hipSuccess) {
      best->dev = nullptr;
      return hip_rc(e, "ACL update buffer");
    }
  }
  *stage_out = best;
  *host_out = best->host;
  return 0;
}

int acl_enqueue_records(xsknf_gpu_acl *acl, AclStage *stage, uint32_t n, void *stream) {
  if (n == 0) return 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t bytes = sizeof(AclUpdateRec) * static_cast<size_t>(n);
  if (!stage->dev || bytes > stage->cap) return -EINVAL;   // (acl.cpp asks for what it sends)
  hipError_t e = hipMemcpyAsync(stage->dev, stage->host, bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_rc(e, "ACL update copy");
  acl_update::Args a;
  a.recs = static_cast<const uint2 *>(stage->dev);
  a.keys = acl->d_keys;
  a.actions = acl->d_actions;
  a.n = n;
  a.slots = acl->slots;
  a.counters = acl->d_ctr;
  const uint32_t tiles = n / acl_update::kThreads + (n % acl_update::kThreads != 0);   // (no sum that can wrap)
  const dim3 grid(tiles < static_cast<uint32_t>(acl_update::kMaxBlocks) ? tiles : acl_update::kMaxBlocks);
  hipLaunchKernelGGL(acl_update::acl_scatter, grid, dim3(acl_update::kThreads), 0, s, a);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(stage->done, s);
  stage->recorded = true;   // (also after an error: the copy may be under way)
  if (e != hipSuccess) return hip_rc(e, "ACL update scatter");
  return 0;
}

int acl_enqueue_table(xsknf_gpu_acl *acl, AclStage *stage, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t bytes = (sizeof(AclKey) + sizeof(int32_t)) * static_cast<size_t>(acl->slots);
  const size_t map_bytes = acl->d_ctr ? sizeof(uint32_t) * static_cast<size_t>(acl->slots) : 0;
  if (bytes + map_bytes > stage->cap || (acl->d_ctr && !acl->d_ctr_spare)) return -EINVAL;
  hipError_t e = hipMemcpyAsync(acl->d_keys, stage->host, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && acl->d_ctr) {
    // the counters follow their keys: the map, then the gather into the spare
    // array, which is the current one for everything enqueued from here on
    e = hipMemcpyAsync(acl->d_ctr_map, static_cast<char *>(stage->host) + bytes, map_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      const acl_update::GatherArgs g = {acl->d_ctr_map, acl->d_ctr, acl->d_ctr_spare, acl->slots};
      const uint32_t tiles = acl->slots / acl_update::kThreads + (acl->slots % acl_update::kThreads != 0);
      const dim3 grid(tiles < static_cast<uint32_t>(acl_update::kMaxBlocks) ? tiles : acl_update::kMaxBlocks);
      hipLaunchKernelGGL(acl_update::acl_counters_gather, grid, dim3(acl_update::kThreads), 0, s, g);
      e = hipGetLastError();
      AclCounter *was = acl->d_ctr;
      acl->d_ctr = acl->d_ctr_spare;
      acl->d_ctr_spare = was;
    }
  }
  if (e == hipSuccess) e = hipEventRecord(stage->done, s);
  stage->recorded = true;
  if (e != hipSuccess) return hip_rc(e, "ACL update table copy");
  return 0;
}

int acl_counters_device_enable(xsknf_gpu_acl *acl) {
  const size_t bytes = sizeof(AclCounter) * static_cast<size_t>(acl->slots) + sizeof(uint64_t) * kAclTotals;
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  // (zero before anything a caller enqueues next, on whatever stream)
  if (e == hipSuccess && ((e = hipMemset(d, 0, bytes)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)) (void)hipFree(d);
  if (e != hipSuccess) return hip_rc(e, "ACL counters");
  acl->d_ctr_base = d;
  acl->d_ctr = static_cast<AclCounter *>(d);
  acl->d_totals = reinterpret_cast<uint64_t *>(acl->d_ctr + acl->slots);
  acl->d_ctr_bytes = bytes;
  return 0;
}

int acl_counters_spare(xsknf_gpu_acl *acl) {
  if (acl->d_ctr_spare) return 0;
  const size_t cb = sizeof(AclCounter) * static_cast<size_t>(acl->slots), mb = sizeof(uint32_t) * static_cast<size_t>(acl->slots);
  void *d = nullptr;
  const hipError_t e = hipMalloc(&d, cb + mb);
  if (e != hipSuccess) return hip_rc(e, "ACL counters' spare array");
  acl->d_ctr_spare_base = d;
  acl->d_ctr_spare = static_cast<AclCounter *>(d);
  acl->d_ctr_map = reinterpret_cast<uint32_t *>(static_cast<char *>(d) + cb);
  acl->d_ctr_bytes += cb + mb;
  return 0;
}

int acl_counters_device_clear(xsknf_gpu_acl *acl, void *stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(acl->d_ctr, 0, sizeof(AclCounter) * static_cast<size_t>(acl->slots), s);
  if (e == hipSuccess) e = hipMemsetAsync(acl->d_totals, 0, sizeof(uint64_t) * kAclTotals, s);
  if (e != hipSuccess) return hip_rc(e, "ACL counters clear");
  return 0;
}

int acl_counters_device_release(xsknf_gpu_acl *acl) {
  int rc = 0;
  hipError_t e;
  if (acl->d_ctr_base && (e = hipFree(acl->d_ctr_base)) != hipSuccess) rc = hip_rc(e, "ACL counters release");
  if (acl->d_ctr_spare_base && (e = hipFree(acl->d_ctr_spare_base)) != hipSuccess) rc = hip_rc(e, "ACL counters release");
  acl->d_ctr_base = acl->d_ctr_spare_base = nullptr;
  acl->d_ctr = acl->d_ctr_spare = nullptr;
  acl->d_totals = nullptr;
  acl->d_ctr_map = nullptr;
  return rc;
}

int acl_staging_release(xsknf_gpu_acl *acl) {
  if (!acl->staging) return 0;
  int rc = 0;
  for (AclStage *st : acl->staging->stages) {
    const int r = stage_free(st);
    if (r) rc = r;
  }
  delete acl->staging;
  acl->staging = nullptr;
  return rc;
}

}  // namespace xsknf_gpu
