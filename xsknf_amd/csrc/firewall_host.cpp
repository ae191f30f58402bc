// firewall_host.cpp -- the firewall NF on one CPU thread (no GPU):
// include/xsknf_gpu.h xsknf_gpu_firewall_host, the model the device lookup
// (firewall_device.hip) is held to.  The reference's callback
// (examples/firewall/firewall_user.c:128-186) walks struct pointers over the
// frame; here the header's rules 0-7 are applied to the frame's bytes one by
// one, and the key goes to the ACL's host copy (acl_table.h).  Plain C++, so
// that tests/test_firewall_san.py can build it under AddressSanitizer + UBSan
// (tests/c/san_firewall.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>

#include "acl_table.h"
#include "desc_rules.h"

namespace {

inline uint32_t le32(const uint8_t *p) {
  return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
         static_cast<uint32_t>(p[3]) << 24;
}

}  // namespace

extern "C" {

int xsknf_gpu_firewall_host(const uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                            const struct xsknf_gpu_acl *acl, int32_t *verdicts) {
  if (!acl) return -EINVAL;
  if (n && (!umem || !descs || !verdicts)) return -EINVAL;
  // the ACL's host counters, if it has any (xsknf_gpu_acl_counters_enable): the
  // hits per slot, and the totals from the hits and the frames that reached the map
  xsknf_gpu::AclCounter *ctr = acl->ctr;
  uint64_t hits = 0, looked = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t off = xsknf_gpu::desc_offset(descs[i].addr);
    const uint32_t len = descs[i].len;
    verdicts[i] = -1;
    if (!xsknf_gpu::in_umem(off, len, umem_size)) continue;   // rule 0
    if (len < 14) continue;                                   // rule 1
    const uint8_t *f = umem + off;
    if (f[12] != 0x08 || f[13] != 0x00) {                     // rule 2
      verdicts[i] = 0;
      continue;
    }
    if (len < 34) continue;                                   // rule 3
    const uint32_t next = 14 + 4 * (f[14] & 15u);             // rule 4
    const uint32_t proto = f[23];
    if (proto != 6 && proto != 17) {                          // rule 5
      verdicts[i] = 0;
      continue;
    }
    if (next + (proto == 6 ? 20u : 8u) > len) continue;
    if (!ctr) {
      verdicts[i] = xsknf_gpu::acl_lookup(acl->keys, acl->actions, acl->slots, le32(f + 26), le32(f + 30),
                                          le32(f + next), proto);   // rules 6, 7
      continue;
    }
    const uint32_t s = xsknf_gpu::acl_find(acl->keys, acl->slots, le32(f + 26), le32(f + 30), le32(f + next), proto);
    ++looked;
    verdicts[i] = 0;
    if (s != xsknf_gpu::kAclNone) {
      verdicts[i] = acl->actions[s];
      ++ctr[s].packets;
      ctr[s].bytes += len;
      ++hits;
    }
  }
  if (ctr) {
    acl->totals[xsknf_gpu::kAclFrames] += n;
    acl->totals[xsknf_gpu::kAclHits] += hits;
    acl->totals[xsknf_gpu::kAclMisses] += looked - hits;
    acl->totals[xsknf_gpu::kAclDecided] += n - looked;
  }
  return 0;
}

}  // extern "C"
