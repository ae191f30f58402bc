// lb_host.cpp -- the load balancer NF on one CPU thread (no GPU):
// include/xsknf_gpu.h xsknf_gpu_lb_host, the model the device batch
// (lb_device.hip) is held to.  The reference's callback
// (examples/load_balancer/load_balancer_user.c:396-553) walks struct pointers
// over the frame; here the header's rules 0-10 are applied to the frame's bytes
// one by one, in the reference's order (lb_table.h frame()), frame after frame
// against the object's host session table.  Plain C++, so that
// tests/test_lb_san.py can build it under AddressSanitizer + UBSan
// (tests/c/san_lb.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>

#include "desc_rules.h"
#include "lb_table.h"

extern "C" {

int xsknf_gpu_lb_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                      uint32_t ingress_ifindex, uint32_t num_interfaces, struct xsknf_gpu_lb *lb, int32_t *verdicts,
                      uint64_t *stats) {
  using namespace xsknf_gpu;
  if (!lb) return -EINVAL;
  if (n && (!umem || !descs || !verdicts)) return -EINVAL;
  uint64_t st[lb::kStats] = {0};
  const lb::Tables t = {lb->svc,       lb->bk,    lb->keys,         lb->vals,   &lb->count,
                        lb->svc_slots, lb->slots, lb->max_sessions, lb->stamps, &lb->clock};   // (stamps: rule 11, or NULL)
  const lb::Gate none = {nullptr, nullptr, 0};
  const int32_t pass = lb::pass_verdict(ingress_ifindex, num_interfaces);
  st[lb::kFrames] = n;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t off = desc_offset(descs[i].addr);
    const uint32_t len = descs[i].len;
    if (!in_umem(off, len, umem_size)) {   // rule 0
      verdicts[i] = -1;
      ++st[lb::kDropped];
      continue;
    }
    verdicts[i] = lb::frame(t, none, umem + off, len, ingress_ifindex, pass, st);
  }
  if (stats)
    for (int k = 0; k < lb::kStats; ++k) stats[k] = st[k];
  return 0;
}

}  // extern "C"
