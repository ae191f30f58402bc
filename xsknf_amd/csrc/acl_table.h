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
#pragma once
#include <stdint.h>

#include "desc_rules.h"   // XSKNF_HD

namespace xsknf_gpu {

struct AclKey {
  uint32_t a, b, c, p;
};
static_assert(sizeof(AclKey) == 16, "one 16-byte load per probe");

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
// built with XSKNF_ACL_HOST_ONLY (the sanitizer program, tests/c/san_firewall.c),
// its copy on the device current at creation: one allocation, the keys first.
struct xsknf_gpu_acl {
  uint32_t slots, rules, max_probe;
  xsknf_gpu::AclKey *keys;     // host, slots entries
  int32_t *actions;            // host, slots entries
  xsknf_gpu::AclKey *d_keys;   // device (NULL in a host-only build)
  int32_t *d_actions;
};
