// acl_table.h -- the firewall's ACL as a table (include/xsknf_gpu.h, "the
// firewall NF"): the slot layout, the hash and the probe, stated once for the
// builder (acl.cpp), the host model (firewall_host.cpp) and the device lookup
// (kernel_firewall.h).  Plain C++17; no GPU call.
//
// A key slot is 16 bytes, the frame's own bytes as little-endian words:
//   a = saddr f[26..29], b = daddr f[30..33], c = sport | dport << 16
//   (f[next..next+3]), p = proto f[23]; p == 0 marks an empty slot (a stored
//   key has p 6 or 17).
// actions[s] belongs to keys[s] and is read only on a hit.
//
// The hash is ours (nothing of the reference's jhash or its chains is kept): each
// word is folded in by an xor, a multiply by an odd 32-bit constant and an
// xor-shift that brings the product's high bits down -- the table is indexed
// by the LOW bits of h, which a multiply alone leaves dependent on the low key
// bits only.  Keys that differ in one bit (tests' near misses) spread over the
// table.  A probe starts at h & (slots - 1) and walks up one slot at a time,
// wrapping, until the key or an empty slot: at most `slots` steps, and the
// builder keeps one slot empty.
//
// Updates (acl.cpp xsknf_gpu_acl_update) delete a key by overwriting its slot
// with the tombstone {0, 0, 0, kAclTombstoneP}: its p is not 0, so a probe walks
// on over it, and it is not 6 or 17, so no frame's key equals it -- acl_lookup,
// acl_find and the kernels need no word about it.  A new key goes into the first
// tombstone of its probe sequence, once the probe has reached an empty slot
// without meeting the key.  The bound: after an update's deletes at most
// slots / kAclTombstoneShare slots are tombstones, and live keys + tombstones +
// the update's new keys leave one slot empty; an update that would pass either
// limit rebuilds the table in place, tombstone-free, before it stores its puts.
// A probe therefore looks at no more than live keys + tombstones + 1 slots.
//
// Hit counters (include/xsknf_gpu.h xsknf_gpu_acl_counters_*) are a side array:
// one AclCounter per slot, in the object only once it has been asked for.  The
// key slots and the actions keep their layout; counters[s] belongs to keys[s].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "desc_rules.h"   // XSKNF_HD

namespace xsknf_gpu {

struct AclKey {
  uint32_t a, b, c, p;
};
static_assert(sizeof(AclKey) == 16, "one 16-byte load per probe");

// p of a slot: 0 empty, 6 or 17 a stored key, kAclTombstoneP a deleted one
constexpr uint32_t kAclTombstoneP = 0xffffffffu;
constexpr uint32_t kAclTombstoneShare = 4;   // at most slots / 4 tombstones outlive an update's deletes

// One slot's new contents, as an update sends them to the device (acl.cpp
// writes them, kernel_acl_update.h scatters them).  The records of one update
// name each slot AT MOST ONCE and carry its final state: the scatter's lanes
// store without looking at one another.
//
// An object with counters sets kAclRecZero in `slot` where the slot's counters
// start again at 0/0: the slot became a tombstone, or its key is new to the map
// (also a key deleted and put again by the same call, which the device could
// not tell from one that stayed).  Slot numbers stay below 2^24
// (XSKNF_GPU_ACL_MAX_SLOTS), so the bit is free; an object without counters
// never sets it.
struct AclUpdateRec {
  uint32_t slot;
  AclKey key;
  int32_t action;
};
static_assert(sizeof(AclUpdateRec) == 24 && alignof(AclUpdateRec) == 4, "three 8-byte loads per record");
constexpr uint32_t kAclRecZero = 1u << 31;
constexpr uint32_t kAclRecSlotMask = ~kAclRecZero;

// One slot's hit counters: the frames that found the slot's key and the sum of
// their descriptors' len.
struct AclCounter {
  uint64_t packets, bytes;
};
static_assert(sizeof(AclCounter) == 16, "two 8-byte adds per group of hits");
// totals (XSKNF_GPU_ACL_TOTALS)
enum AclTotal : int { kAclFrames, kAclHits, kAclMisses, kAclDecided, kAclTotals };

XSKNF_HD inline uint32_t acl_hash(uint32_t a, uint32_t b, uint32_t c, uint32_t p) {
  uint32_t h = a * 0x9E3779B1u;
  h ^= h >> 15;
  h = (h ^ b) * 0x85EBCA77u;
  h ^= h >> 13;
  h = (h ^ c) * 0xC2B2AE3Du;
  h ^= h >> 16;
  h = (h ^ p) * 0x27D4EB2Fu;
  h ^= h >> 15;
  return h;
}

// The action of key {a, b, c, p} (p != 0) in a table of `slots` slots, or 0.
XSKNF_HD inline int32_t acl_lookup(const AclKey *keys, const int32_t *actions, uint32_t slots, uint32_t a,
                                   uint32_t b, uint32_t c, uint32_t p) {
  const uint32_t mask = slots - 1;
  uint32_t s = acl_hash(a, b, c, p) & mask;
  for (uint32_t i = 0; i < slots; ++i) {   // bounded whatever the table holds
    const AclKey k = keys[s];
    if (k.p == 0) return 0;
    if (k.a == a && k.b == b && k.c == c && k.p == p) return actions[s];
    s = (s + 1) & mask;
  }
  return 0;
}

// The slot of key {a, b, c, p} (p != 0), or kAclNone: for a caller to whom an
// action of 0 is a hit like any other (the lbfw NF's gate).
constexpr uint32_t kAclNone = 0xffffffffu;
XSKNF_HD inline uint32_t acl_find(const AclKey *keys, uint32_t slots, uint32_t a, uint32_t b, uint32_t c,
                                  uint32_t p) {
  const uint32_t mask = slots - 1;
  uint32_t s = acl_hash(a, b, c, p) & mask;
  for (uint32_t i = 0; i < slots; ++i) {   // bounded whatever the table holds
    const AclKey k = keys[s];
    if (k.p == 0) return kAclNone;
    if (k.a == a && k.b == b && k.c == c && k.p == p) return s;
    s = (s + 1) & mask;
  }
  return kAclNone;
}

}  // namespace xsknf_gpu

// The object behind struct xsknf_gpu_acl: the table on the host and, unless
// built with XSKNF_ACL_HOST_ONLY (the sanitizer programs, tests/c/san_firewall.c
// and san_acl_update.c), its copy on the device current at creation: one
// allocation, the keys first.
struct xsknf_gpu_acl {
  uint32_t slots, rules, max_probe;
  xsknf_gpu::AclKey *keys;     // host, slots entries
  int32_t *actions;            // host, slots entries
  xsknf_gpu::AclKey *d_keys;   // device (NULL in a host-only build)
  int32_t *d_actions;
  uint32_t tombstones;         // slots that hold the tombstone
  uint32_t *probe_hist;        // host, slots + 1 entries: [d] = live keys found at their d-th probe (max_probe's source)
  struct xsknf_gpu_acl_staging *staging;   // acl_update_device.hip: the updates' buffers (NULL until the first one)
  // hit counters (all NULL / 0 until xsknf_gpu_acl_counters_enable).  Host: one
  // allocation, `slots` counters and behind them the totals.  Device: the same
  // in d_ctr_base; a rebuild gathers the counters into the other of two arrays
  // (d_ctr_spare, allocated by the first such rebuild together with d_ctr_map,
  // the new slots' old slots) and the two change roles
  xsknf_gpu::AclCounter *ctr;
  uint64_t *totals;
  xsknf_gpu::AclCounter *d_ctr;
  uint64_t *d_totals;
  xsknf_gpu::AclCounter *d_ctr_spare;
  uint32_t *d_ctr_map;
  void *d_ctr_base, *d_ctr_spare_base;
  uint64_t d_ctr_bytes;                    // device memory of the above, part of device_bytes
};

#ifndef XSKNF_ACL_HOST_ONLY
// acl_update_device.hip: how an update reaches the device table.  A stage is a
// pinned host buffer of at least `bytes` bytes (and, with `records`, a device
// buffer as large) that no update still in flight uses; acl.cpp fills *host_out
// and hands the stage to exactly one of the two enqueue calls, after which the
// stage is busy until `stream` has passed it.  All return 0, -ENOMEM or -EIO
// (xsknf_gpu_last_error()).
namespace xsknf_gpu {
struct AclStage;
int acl_stage_acquire(xsknf_gpu_acl *acl, size_t bytes, bool records, AclStage **stage_out, void **host_out);
// n AclUpdateRec at the stage's start: copy them over and scatter them into the table
int acl_enqueue_records(xsknf_gpu_acl *acl, AclStage *stage, uint32_t n, void *stream);
// the whole table at the stage's start, keys then actions: copy it over the device table
int acl_enqueue_table(xsknf_gpu_acl *acl, AclStage *stage, void *stream);
int acl_staging_release(xsknf_gpu_acl *acl);   // _destroy
// Counters.  _enable: the device arrays, zeroed.  _spare: the second array and
// the map, before a rebuild's host pass (nothing after it may fail for want of
// memory).  acl_enqueue_table of an object with counters expects the map, one
// uint32_t per slot, behind the table in the stage and enqueues the copy, the
// gather and the arrays' change of roles with it.
int acl_counters_device_enable(xsknf_gpu_acl *acl);
int acl_counters_spare(xsknf_gpu_acl *acl);
int acl_counters_device_clear(xsknf_gpu_acl *acl, void *stream);
int acl_counters_device_release(xsknf_gpu_acl *acl);
}  // namespace xsknf_gpu
#endif
