// kernel_acl_update.h -- an ACL update's scatter into the device table.  Part of
// acl_update_device.hip's translation unit (none of checksummer.hip's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acl_table.h"

namespace xsknf_gpu {
namespace acl_update {

constexpr int kThreads = 256;       // records per block and step: one lane per record
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

struct Args {
  const uint2 *recs;   // n AclUpdateRec, 8-byte aligned
  AclKey *keys;
  int32_t *actions;
  uint32_t n;
  uint32_t slots;
  AclCounter *counters;   // the object's hit counters, or NULL: then `slot` carries no flag
};

// One lane per record; a block takes kThreads consecutive records per step and
// every gridDim.x-th such tile.  Per record: its 24 bytes, read as 8-byte words
// (the compiler makes a 4-, a 16- and a 4-byte load of them; a wave's loads
// cover 1,536 consecutive bytes between them, every line used whole), then the
// slot's 16-byte key as one store and its 4-byte action as another, both plain
// vector stores to wherever the slot lies.
//
// The invariant the lanes rely on (acl_table.h AclUpdateRec, kept by acl.cpp):
// the records of one launch name each slot at most once, so no two lanes store
// to the same slot and the order of lanes, waves and blocks means nothing.  A
// record whose slot is not below `slots` is skipped.  The two stores of a slot
// are not one: a lookup that runs beside the scatter may see the new key with
// the old action (include/xsknf_gpu.h leaves that to the caller's ordering).
// With counters the record's kAclRecZero says that the slot's counters start
// again (acl_table.h): one more 16-byte store, to the same lane's own slot.
// No LDS, no atomics, no block waits on another.
__global__ __launch_bounds__(kThreads) void acl_scatter(const Args a) {
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t r = blockIdx.x * kThreads + threadIdx.x; r < a.n; r += stride) {
    const uint2 w0 = a.recs[3 * r], w1 = a.recs[3 * r + 1], w2 = a.recs[3 * r + 2];
    const uint32_t slot = a.counters ? w0.x & kAclRecSlotMask : w0.x;
    if (slot < a.slots) {
      *reinterpret_cast<uint4 *>(a.keys + slot) = make_uint4(w0.y, w1.x, w1.y, w2.x);
      a.actions[slot] = static_cast<int32_t>(w2.y);
      if (a.counters && (w0.x & kAclRecZero)) *reinterpret_cast<uint4 *>(a.counters + slot) = make_uint4(0, 0, 0, 0);
    }
  }
}

// A rebuild's carry: the table's new slot s holds the key that lay in slot
// from[s], or (kAclNone) a key new to the map or none.  One lane per slot:
// 4 bytes of the map read and 16 bytes of `to` written, both coalesced, and for
// a carried key 16 bytes of `cur` read from wherever it lay.  `to` and `cur`
// are different arrays, so the order of lanes means nothing; an old slot that is
// not below `slots` counts as none.
struct GatherArgs {
  const uint32_t *from;
  const AclCounter *cur;
  AclCounter *to;
  uint32_t slots;
};
__global__ __launch_bounds__(kThreads) void acl_counters_gather(const GatherArgs a) {
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.slots; s += stride) {
    const uint32_t old = a.from[s];
    uint4 c = make_uint4(0, 0, 0, 0);
    if (old < a.slots) c = *reinterpret_cast<const uint4 *>(a.cur + old);
    *reinterpret_cast<uint4 *>(a.to + s) = c;
  }
}

}  // namespace acl_update
}  // namespace xsknf_gpu
