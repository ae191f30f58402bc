// lbfw_host.cpp -- the lbfw NF, the firewall's ACL in front of the load
// balancer, on one CPU thread (no GPU): include/xsknf_gpu.h xsknf_gpu_lbfw_host,
// the model the device batch (lb_device.hip, xsknf_gpu_lbfw_batch) is held to.
// The reference's callback (examples/lbfw/lbfw_user.c:420-594) is the load
// balancer's with its own PASS and the ACL gate between rules 6 and 7; here it
// is lb_host.cpp's loop over the same body (lb_table.h frame()) with that PASS
// and the ACL's host copy, against the lb object's host session table.  Plain
// C++, so that tests/test_lbfw_san.py can build it under AddressSanitizer +
// UBSan (tests/c/san_lbfw.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>

#include "desc_rules.h"
#include "lb_table.h"

extern "C" {

int xsknf_gpu_lbfw_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                        uint32_t ingress_ifindex, uint32_t num_interfaces, const struct xsknf_gpu_acl *acl,
                        struct xsknf_gpu_lb *lb, int32_t *verdicts, uint64_t *stats) {
  using namespace xsknf_gpu;
  if (!lb || num_interfaces == 0) return -EINVAL;   // (the reference divides by zero)
  if (n && (!umem || !descs || !verdicts)) return -EINVAL;
  uint64_t st[lb::kStats] = {0};
  const lb::Tables t = {lb->svc,       lb->bk,    lb->keys,         lb->vals,   &lb->count,
                        lb->svc_slots, lb->slots, lb->max_sessions, lb->stamps, &lb->clock};   // (stamps: rule 11, or NULL)
  const lb::Gate gate = acl ? lb::Gate{acl->keys, acl->actions, acl->slots, acl->ctr, reinterpret_cast<unsigned long long *>(acl->totals)}
                            : lb::Gate{nullptr, nullptr, 0};
  const uint64_t hits0 = acl && acl->ctr ? acl->totals[kAclHits] : 0, misses0 = acl && acl->ctr ? acl->totals[kAclMisses] : 0;
  const int32_t pass = lb::lbfw_pass_verdict(ingress_ifindex, num_interfaces);
  st[lb::kFrames] = n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t off = desc_offset(descs[i].addr);
    const uint32_t len = descs[i].len;
    if (!in_umem(off, len, umem_size)) {   // rule 0
      verdicts[i] = -1;
      ++st[lb::kDropped];
      continue;
    }
    verdicts[i] = lb::frame(t, gate, umem + off, len, ingress_ifindex, pass, st);
  }
  if (acl && acl->ctr) {   // (lb::frame counted the hits and the misses at the gate)
    acl->totals[kAclFrames] += n;
    acl->totals[kAclDecided] += n - (acl->totals[kAclHits] - hits0) - (acl->totals[kAclMisses] - misses0);
  }
  if (stats)
    for (int k = 0; k < lb::kStats; ++k) stats[k] = st[k];
  return 0;
}

}  // extern "C"
