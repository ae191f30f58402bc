// macswap_host.cpp -- the macswap NF on one CPU thread (no GPU):
// include/xsknf_gpu.h xsknf_gpu_macswap_host, the model the device call
// (macswap_device.hip) is held to.  The reference's callback
// (examples/macswap/macswap_user.c:34-50) exchanges the addresses through
// unsigned short pointers and, for the second swap, byte by byte (macswap.h);
// here both are byte exchanges, and a double swap carries out both.  Plain
// C++, so that tests/test_macswap_san.py can build it under AddressSanitizer +
// UBSan (tests/c/san_macswap.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>

#include "desc_rules.h"
#include "macswap_rules.h"

namespace {

inline void swap_macs(uint8_t *f) {
  for (int i = 0; i < 6; ++i) {
    const uint8_t t = f[i];
    f[i] = f[6 + i];
    f[6 + i] = t;
  }
}

}  // namespace

extern "C" {

int xsknf_gpu_macswap_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                           uint32_t ingress_ifindex, const struct xsknf_macswap_opts *opts, int32_t *verdicts) {
  int32_t fwd;
  const int rc = xsknf_gpu::macswap::forward_verdict(opts, ingress_ifindex, &fwd);
  if (rc) return rc;
  if (n && (!umem || !descs || !verdicts)) return -EINVAL;
  const bool twice = opts->double_macswap != 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t off = xsknf_gpu::desc_offset(descs[i].addr);
    const uint32_t len = descs[i].len;
    verdicts[i] = -1;
    if (!xsknf_gpu::in_umem(off, len, umem_size)) continue;   // rule 0
    if (len < 14) continue;                                   // rule 1
    swap_macs(umem + off);                                    // rule 2
    if (twice) swap_macs(umem + off);
    verdicts[i] = fwd;                                        // rule 3
  }
  return 0;
}

}  // extern "C"
