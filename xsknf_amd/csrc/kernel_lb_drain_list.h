// kernel_lb_drain_list.h -- draining a list of backends from the load balancer's
// device table in one pass (include/xsknf_gpu.h xsknf_gpu_lb_drain_backends).
// Part of lb_remove_device.hip's translation unit, beside kernel_lb_remove.h,
// whose Args, flush and four compaction launches it uses as they are.
//
//   lb_drain_list    one lane per slot, grid-stride, ONE pass whatever the list's
//                    length.  A live slot names one backend (lb::drain_candidate:
//                    the value's {addr, port} for a TO_BACKEND session, the
//                    key's source for a TO_CLIENT one, with the key's protocol);
//                    the lane looks it up in the list and, on a hit, stores the
//                    tombstone.  That is the union of lb::drains over the list:
//                    drains compares exactly this candidate with one backend.
//                    A slot has one lane, so there is no race and no claim.
//
// The list arrives as the open-addressing set lb.cpp builds (lb_table.h IdSlot:
// a power of two of 8-byte slots, at most half full, acl_hash, linear probing).
//   set_slots <= kLdsSetSlots (1024 slots, 8 KiB: a list of up to 512 entries,
//   duplicates counted): every block copies the set into LDS once, one 8-byte
//   load and store per lane and step, and its lanes probe there.  8 KiB a block
//   leaves the CU's 160 KiB room for every block the other limits allow.
//   Larger sets (up to 2^18 slots, 2 MiB, for XSKNF_GPU_LB_MAX_BACKENDS
//   entries) are probed in global memory: read-only for the launch, shared by
//   every lane, and small beside the L2, where they stay.
// The bound is low on purpose: a block's copy is traffic too (2048 blocks x 8
// KiB = 16 MiB through the L2 against the 64 MiB of a 2^22-slot table).
// DESIGN 4.4.2 has what the pass costs at lists of 1 to 4096.
//
// The slot's key and value are one 16-byte load each (a wave reads 1 KiB of
// keys, then the values of its live slots); the tombstone is one 4-byte store.
// Counting is kernel_lb_remove.h's: one LDS word per block, three atomics per
// block.  No lane waits for another; the only barriers are the block's own,
// around the copy and in flush, which every lane reaches.
#pragma once
#include "kernel_lb_remove.h"

namespace xsknf_gpu {
namespace lbr {

constexpr uint32_t kLdsSetSlots = 1024;   // the largest set a block keeps in LDS

struct ListArgs {
  Args t;                    // the table: keys, vals, count, result, slots
  const lb::IdSlot *set;     // set_slots entries
  uint32_t set_slots;        // a power of two, >= 2
};

__global__ __launch_bounds__(kThreads) void lb_drain_list(const ListArgs a) {
  __shared__ uint32_t removed;
  __shared__ lb::IdSlot lds_set[kLdsSetSlots];
  const bool in_lds = a.set_slots <= kLdsSetSlots;   // (the same for every lane of the launch)
  if (threadIdx.x == 0) removed = 0;
  if (in_lds)
    for (uint32_t i = threadIdx.x; i < a.set_slots; i += kThreads) lds_set[i] = a.set[i];
  __syncthreads();
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.t.slots; s += stride) {
    const lb::Key k = a.t.keys[s];
    if (!lb::live(k)) continue;
    const lb::IdSlot c = lb::drain_candidate(k, a.t.vals[s]);
    const bool hit = in_lds ? lb::id_listed(lds_set, a.set_slots, c) : lb::id_listed(a.set, a.set_slots, c);
    if (!hit) continue;
    a.t.keys[s].p = lb::kTombstoneP;
    atomicAdd(&removed, 1u);
  }
  flush(a.t, &removed);
}

}  // namespace lbr
}  // namespace xsknf_gpu
