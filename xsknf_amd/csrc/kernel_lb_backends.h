// kernel_lb_backends.h -- an update of the load balancer's services and backends
// scattered into the device copy (include/xsknf_gpu.h
// xsknf_gpu_lb_backends_update).  Part of lb_backends_device.hip's translation
// unit (none of lb_device.hip's: the batch kernels are not rebuilt for it).
//
// Which way an update takes (lb.cpp decides, lb_backends_device.hip enqueues):
//   entries  the service slots and backend entries that differ from the device
//            copy, each once and in its final state, as 32-byte LbEntry {index,
//            16-byte record}: one async copy and the launch below;
//   table    the first update of an object (its tables move to the region that
//            has room for the maxima) and every update whose entries would be
//            no shorter than the tables themselves (2 x changed >= service
//            slots + backends): one async copy of the tables whole, no launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lb_table.h"

namespace xsknf_gpu {
namespace lb_backends {

constexpr int kThreads = 256;       // entries per block and step: one lane per entry
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

struct Args {
  const uint4 *entries;   // n LbEntry: two 16-byte words each
  uint4 *region;          // svc_slots service slots, then the backends
  uint32_t n;
  uint32_t limit;         // 16-byte entries in the region
};

// One lane per entry, grid-stride: two 16-byte loads (a wave's cover 2 KiB of
// consecutive bytes) and one 16-byte vector store to wherever the index lies.
// The entries of one launch name each index at most once (lb.cpp compares
// every index once), so no two lanes store to one place and the order of
// lanes, waves and blocks means nothing.  An index not below `limit` is
// skipped.  A record is one store: a batch beside the scatter -- which only
// another stream can run, and that is the caller's to order -- never sees half
// a service slot.  No LDS, no atomics, no block waits on another.
__global__ __launch_bounds__(kThreads) void lb_backends_scatter(const Args a) {
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
    const uint32_t index = a.entries[2 * i].x;
    const uint4 rec = a.entries[2 * i + 1];
    if (index < a.limit) a.region[index] = rec;
  }
}

}  // namespace lb_backends
}  // namespace xsknf_gpu
