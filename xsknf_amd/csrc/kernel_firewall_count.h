// kernel_firewall_count.h -- the firewall's device lookup for an ACL with hit
// counters (include/xsknf_gpu.h xsknf_gpu_acl_counters_*).  Part
// of firewall_device.hip's translation unit; kernel_firewall.h's
// firewall_lookup, the launch of every ACL without counters, is not touched by
// it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acl_table.h"
#include "desc_rules.h"
#include "kernel_acl_count.h"
#include "kernel_firewall.h"
#include "ld_bytes.h"

namespace xsknf_gpu {
namespace firewall {

struct CountArgs {
  Args f;                         // the lookup's own
  AclCounter *counters;           // one per slot
  unsigned long long *totals;     // kAclTotals
};

// Rules 0-7 for one frame, as verdict_of, with the slot instead of the action:
// kAclDecided and the verdict where rules 0-5 decide, else kAclHits and the slot
// or kAclMisses.
__device__ __forceinline__ int classify(const Args &a, uint64_t addr, uint32_t len, int32_t &verdict, uint32_t &slot) {
  const uint64_t off = desc_offset(addr);
  verdict = -1;
  if (!in_umem(off, len, a.umem_size) || len < 14) return kAclDecided;     // rules 0, 1
  if (len < 34) {                                                          // rules 2, 3
    verdict = (ld_bytes(a.umem, off + 12, 2) & 0xffff) != 0x0008 ? 0 : -1;
    return kAclDecided;
  }
  const uint32_t e = ld_bytes(a.umem, off + 12, 4);
  const uint32_t proto = ld_bytes(a.umem, off + 23, 1) & 0xff;
  const uint32_t sa = ld_bytes(a.umem, off + 26, 4), da = ld_bytes(a.umem, off + 30, 4);
  verdict = 0;
  if ((e & 0xffff) != 0x0008) return kAclDecided;                          // rule 2
  const uint32_t next = 14 + 4 * ((e >> 16) & 15);                         // rule 4
  if (proto != 6 && proto != 17) return kAclDecided;                       // rule 5
  verdict = -1;
  if (next + (proto == 6 ? 20u : 8u) > len) return kAclDecided;
  const uint32_t ports = ld_bytes(a.umem, off + next, 4);                  // rule 6
  slot = acl_find(a.keys, a.slots, sa, da, ports, proto);                  // rule 7
  verdict = 0;
  return slot != kAclNone ? kAclHits : kAclMisses;
}

// How the hits reach the counters.  kStageRepeats is the product's; the others
// are A/B shapes (`make ab`, XSKNF_ACL_COUNT_SHAPE=naive|wave|stage), measured
// against it in DESIGN 4.3.2.
enum CountShape : int {
  kStageRepeats,   // the first hit of a slot in a block adds to memory for itself, the later ones meet in LDS
  kNaive,          // every hit adds for itself
  kWave,           // kernel_acl_count.h count_hits: a wave's hits on one slot add once
  kStageAll,       // every hit goes through LDS; the block adds when it ends
};

// The block's stage: kStage entries in LDS, {slot, packets, bytes}, indexed by
// the slot's low bits.  A hit makes one compare-and-swap on its entry's slot
// word.  If it claims the entry it is the slot's first hit in this block, and
// it adds to memory for itself at once, like a lookup without a stage: traffic
// in which no rule repeats pays one LDS operation per hit and its adds go out
// while other waves still wait for their loads.  If it finds its own slot there
// the block has seen the rule before: it adds to the entry with two LDS atomics
// and touches no memory.  If another slot holds the entry it adds to memory for
// itself.  The entries live for the whole launch -- every trip of the block's
// loop adds to them -- and what they hold is added to the counters once, when
// the block ends.  So one elephant flow costs its slot two pairs of adds per
// block, however many of its frames the block sees.
constexpr int kStage = 512;
template <bool kHas>
struct Stage {
  uint32_t slot[kStage], packets[kStage];
  unsigned long long bytes[kStage];
};
template <>
struct Stage<false> {
  uint32_t slot[1], packets[1];
  unsigned long long bytes[1];
};

// firewall_lookup's launch shape and per-frame reads, the action read from the
// slot the probe returns.  The loop runs over whole tiles, so every lane of a
// wave makes the same trips (a lane past the batch's end is in no class) and
// the three ballots per trip see the whole wave; their counts stay in scalars,
// meet in LDS when the block ends, and four lanes add the four totals.  The
// counters' adds are no-return device-scope atomics to wherever the slots lie:
// they execute at the memory side, and nothing waits for them.
template <int kShape>
__global__ __launch_bounds__(kThreads) void firewall_lookup_count(const CountArgs a) {
  constexpr bool kStaged = kShape == kStageRepeats || kShape == kStageAll;
  __shared__ uint32_t tot[kAclTotals];
  __shared__ Stage<kStaged> st;
  if (threadIdx.x < kAclTotals) tot[threadIdx.x] = 0;
  if constexpr (kStaged) {
    for (int i = threadIdx.x; i < kStage; i += kThreads) {
      st.slot[i] = kAclNone;
      st.packets[i] = 0;
      st.bytes[i] = 0;
    }
  }
  __syncthreads();
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  uint32_t frames = 0, hits = 0, misses = 0;
  for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kThreads; base < a.f.n; base += stride) {
    const uint64_t f = base + threadIdx.x;
    const bool in = f < a.f.n;
    int cls = kAclTotals;   // none
    uint32_t slot = kAclNone, len = 0;
    if (in) {
      const uint4 d = a.f.descs[f];
      int32_t verdict;
      len = d.z;
      cls = classify(a.f, static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32, len, verdict, slot);
      if (cls == kAclHits) verdict = a.f.actions[slot];
      a.f.verdicts[f] = verdict;
    }
    if constexpr (kShape == kNaive) {
      acl_count::count_hits_naive(a.counters, cls == kAclHits, slot, len);
    } else if constexpr (kShape == kWave) {
      acl_count::count_hits(a.counters, cls == kAclHits, slot, len);
    } else if (cls == kAclHits) {
      const uint32_t h = slot & (kStage - 1);
      const uint32_t held = atomicCAS(&st.slot[h], kAclNone, slot);
      if (held == slot || (kShape == kStageAll && held == kAclNone)) {
        atomicAdd(&st.packets[h], 1u);
        atomicAdd(&st.bytes[h], static_cast<unsigned long long>(len));
      } else {
        acl_count::count_hits_naive(a.counters, true, slot, len);
      }
    }
    frames += static_cast<uint32_t>(__popcll(__ballot(in)));
    hits += static_cast<uint32_t>(__popcll(__ballot(cls == kAclHits)));
    misses += static_cast<uint32_t>(__popcll(__ballot(cls == kAclMisses)));
  }
  if ((threadIdx.x & 63) == 0 && frames) {
    atomicAdd(&tot[kAclFrames], frames);
    atomicAdd(&tot[kAclHits], hits);
    atomicAdd(&tot[kAclMisses], misses);
    atomicAdd(&tot[kAclDecided], frames - hits - misses);
  }
  __syncthreads();
  if constexpr (kStaged) {
    for (int i = threadIdx.x; i < kStage; i += kThreads)
      if (st.packets[i]) {   // (then st.slot[i] is a hit's slot: below a.f.slots)
        acl_count::add_agent(&a.counters[st.slot[i]].packets, st.packets[i]);
        acl_count::add_agent(&a.counters[st.slot[i]].bytes, st.bytes[i]);
      }
  }
  if (threadIdx.x < kAclTotals && tot[threadIdx.x])
    __hip_atomic_fetch_add(&a.totals[threadIdx.x], static_cast<unsigned long long>(tot[threadIdx.x]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace firewall
}  // namespace xsknf_gpu
