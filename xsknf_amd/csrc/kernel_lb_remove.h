// kernel_lb_remove.h -- removing sessions from the load balancer's device table
// (include/xsknf_gpu.h xsknf_gpu_lb_sessions_remove, _drain_backend).  Part of
// lb_remove_device.hip's translation unit (none of lb_device.hip's: the batch
// kernels of kernel_lb.h are not rebuilt and know nothing of this).
//
// The host and the device table are independent and the batches fill the device
// table themselves, so the host cannot say which slots change: the device finds,
// buries and counts on its own, in stream order, and the host reads nothing back.
// One call is five launches, all enqueued every time; the last four decide from
// device memory whether they do anything (as lb_apply and lb_commit do):
//
//   lb_remove_keys   one lane per listed key.  lb::find, then ONE agent-scope
//   (or lb_drain)    atomic exchange of the slot's p word with the tombstone:
//                    the lane that gets the key's protocol back has removed the
//                    slot and counts it, every other lane of that key -- a
//                    duplicate, or a lane that came for it as a partner -- gets
//                    the tombstone back and counts nothing.  The slot's other
//                    three key words and its value stay, so a lane that still
//                    reads them sees a session that merely no longer matches.
//                    With REMOVE_PAIR the winner derives the partner key from
//                    the value it read (lb::partner_key), looks it up, checks
//                    it (lb::is_partner) and claims it the same way.
//                    lb_drain has one lane per slot and no race: the slot's
//                    lane evaluates lb::drains and stores the tombstone.
//   lb_compact_zero  if tombstones > slots / kTombstoneShare: zero the spare table
//   lb_compact_move  ... every live slot into the spare table (commit_one's
//                    compare-and-swap on p, then the other words)
//   lb_compact_back  ... the spare table over the live one, slot by slot
//   lb_compact_done  one lane: ... tombstones = 0, result[COMPACTED] = 1
// With ageing (Args::stamps: include/xsknf_gpu.h xsknf_gpu_lb_aging_enable) a
// session's last-seen stamp moves with it: lb_compact_move stores it beside the
// slot it has claimed in the spare table, lb_compact_back copies it home.  A
// stamp of a slot that holds no session means nothing and is never cleared.
//
// Why one launch gives the set semantics whatever the lane order.  A slot is
// buried only (1) by a lane whose listed key it holds or (2) as the checked
// partner of a listed key that was found; both are members of the set the
// header defines on the table as it stood.  Everything a lane reads to decide --
// a slot's words a, b, c and its value -- is written by no lane of the launch;
// only p changes, and only to the tombstone.  A lane that finds its key already
// buried was beaten by a duplicate (which does the partner's work itself) or by
// the lane of the key's own partner (is_partner is symmetric in the pair, and
// that lane's key is listed, so the pair is complete).  A lane that finds its
// partner already buried skips it: it is removed.  A stale read of p from a CU's
// L1 can only show a buried slot as live; the exchange then returns the
// tombstone and the lane loses, as above.
//
// Counting: each lane adds to one LDS word (the compiler makes that one add per
// wave), and the block's first lane issues three atomics: result[REMOVED], the
// session count down, the tombstone count up.  Never one atomic per key on one
// word.
//
// Compaction copies back (no pointer of the object changes), so calls on
// different streams stay correct as long as the streams are ordered among
// themselves; the spare table's contents mean nothing between calls.  All
// loops are grid-stride over n or over slots; no lane waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lb_table.h"

namespace xsknf_gpu {
namespace lbr {

constexpr int kThreads = 256;       // keys or slots per block and step: one lane each
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

struct Args {
  const uint4 *list;                 // n struct xsknf_gpu_lb_session_key (lb_remove_keys)
  lb::Key *keys;
  lb::Val *vals;
  lb::Key *spare_keys;
  lb::Val *spare_vals;
  uint32_t *count;                   // count[0] sessions, count[1] tombstones
  unsigned long long *result;        // 2 words, or NULL
  uint32_t n, slots, pair;
  uint32_t addr, port, proto;        // lb_drain
  // ageing; all NULL for an object without it
  uint32_t *stamps;                  // one per slot
  uint32_t *spare_stamps;            // one per slot of the spare table
  const uint32_t *clock;             // the table's clock word (lb_expire)
  uint32_t max_idle;                 // lb_expire
};

// Bury slot s, which held a key of protocol p when the lane looked.  True for
// the one lane that removed it.
__device__ __forceinline__ bool claim(const Args &a, uint32_t s, uint32_t p) {
  return __hip_atomic_exchange(&a.keys[s].p, lb::kTombstoneP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p;
}

// The block's removals: into the result, off the session count, onto the tombstones.
__device__ __forceinline__ void flush(const Args &a, uint32_t *removed) {
  __syncthreads();
  if (threadIdx.x == 0 && *removed) {
    if (a.result)
      __hip_atomic_fetch_add(&a.result[0], static_cast<unsigned long long>(*removed), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_sub(&a.count[0], *removed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&a.count[1], *removed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kThreads) void lb_remove_keys(const Args a) {
  __shared__ uint32_t removed;
  if (threadIdx.x == 0) removed = 0;
  __syncthreads();
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
    const uint4 w = a.list[i];
    const lb::Key k = {w.x, w.y, w.z, w.w & 0xff};   // (the record's pad bytes are ignored)
    if (k.p != 6 && k.p != 17) continue;
    const uint32_t s = lb::find(a.keys, a.slots, k);
    if (s == lb::kNone || !claim(a, s, k.p)) continue;
    atomicAdd(&removed, 1u);
    if (!a.pair) continue;
    const lb::Val v = a.vals[s];
    const lb::Key pk = lb::partner_key(k, v);
    const uint32_t ps = lb::find(a.keys, a.slots, pk);
    if (ps != lb::kNone && lb::is_partner(pk, a.vals[ps], k, v) && claim(a, ps, pk.p)) atomicAdd(&removed, 1u);
  }
  flush(a, &removed);
}

__global__ __launch_bounds__(kThreads) void lb_drain(const Args a) {
  __shared__ uint32_t removed;
  if (threadIdx.x == 0) removed = 0;
  __syncthreads();
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.slots; s += stride) {
    if (!lb::drains(a.keys[s], a.vals[s], a.addr, a.port, a.proto)) continue;
    a.keys[s].p = lb::kTombstoneP;
    atomicAdd(&removed, 1u);
  }
  flush(a, &removed);
}

// The same word for every lane of the four launches: only lb_compact_done, the
// last one, changes it.
__device__ __forceinline__ bool compacting(const Args &a) { return a.count[1] > a.slots / lb::kTombstoneShare; }

__global__ __launch_bounds__(kThreads) void lb_compact_zero(const Args a) {
  if (!compacting(a)) return;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.slots; s += stride) {
    *reinterpret_cast<uint4 *>(a.spare_keys + s) = make_uint4(0, 0, 0, 0);
    *reinterpret_cast<uint4 *>(a.spare_vals + s) = make_uint4(0, 0, 0, 0);
  }
}

__global__ __launch_bounds__(kThreads) void lb_compact_move(const Args a) {
  if (!compacting(a)) return;
  const uint32_t stride = gridDim.x * kThreads, mask = a.slots - 1;
  for (uint64_t i = blockIdx.x * kThreads + threadIdx.x; i < a.slots; i += stride) {
    const lb::Key k = a.keys[i];
    if (!lb::live(k)) continue;
    const lb::Val v = a.vals[i];
    uint32_t s = lb::key_hash(k) & mask;
    for (uint32_t j = 0; j < a.slots; ++j) {   // the live keys are distinct and at most half the slots
      uint32_t empty = 0;
      if (__hip_atomic_compare_exchange_strong(&a.spare_keys[s].p, &empty, k.p, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        a.spare_keys[s].a = k.a;
        a.spare_keys[s].b = k.b;
        a.spare_keys[s].c = k.c;
        a.spare_vals[s] = v;
        if (a.stamps) a.spare_stamps[s] = a.stamps[i];
        break;
      }
      s = (s + 1) & mask;
    }
  }
}

__global__ __launch_bounds__(kThreads) void lb_compact_back(const Args a) {
  if (!compacting(a)) return;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t s = blockIdx.x * kThreads + threadIdx.x; s < a.slots; s += stride) {
    *reinterpret_cast<uint4 *>(a.keys + s) = *reinterpret_cast<const uint4 *>(a.spare_keys + s);
    *reinterpret_cast<uint4 *>(a.vals + s) = *reinterpret_cast<const uint4 *>(a.spare_vals + s);
    if (a.stamps) a.stamps[s] = a.spare_stamps[s];
  }
}

__global__ __launch_bounds__(64) void lb_compact_done(const Args a) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || !compacting(a)) return;
  a.count[1] = 0;
  if (a.result) a.result[1] = 1;
}

}  // namespace lbr
}  // namespace xsknf_gpu
