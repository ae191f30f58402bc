// route_host.cpp -- the routing of a checksummed batch on one CPU thread (no
// GPU): include/xsknf_gpu.h xsknf_gpu_route_host, the model the device router
// (route_device.hip) is held to.  The reference's batch loop files every frame
// by its verdict as it goes (src/xsknf.c:503-522, :654-672: to_drop[] and
// to_tx[verdict][], in receive order); here the lists of one batch lie one after
// another, so the frames are counted first and filed second.  Plain C++, so that
// tests/test_route.py can build it under AddressSanitizer + UBSan
// (tests/c/san_route.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

namespace {

// The bin of a verdict: an interface, or num_interfaces for a drop.  One
// interface: process_batch_1if (src/xsknf.c:663-671; xsknf_rt.c dispose_1if) --
// -1 drops, anything else is the one tx queue.  Several: xsknf_rt.c
// dispose_multi -- a verdict that names no interface drops (the reference would
// index to_tx[] with it unchecked).
inline uint32_t bin_of(int32_t v, uint32_t nif) {
  if (nif == 1) return v == -1 ? 1u : 0u;
  return v < 0 || static_cast<uint32_t>(v) >= nif ? nif : static_cast<uint32_t>(v);
}

}  // namespace

extern "C" {

int xsknf_gpu_route_host(const struct xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n,
                         uint32_t num_interfaces, struct xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs,
                         uint32_t *order, uint64_t *counts) {
  if (num_interfaces == 0 || num_interfaces > XSKNF_GPU_ROUTE_MAX_INTERFACES) return -EINVAL;
  if (n && (!descs || !verdicts || !tx_descs || !fill_addrs)) return -EINVAL;
  uint64_t at[XSKNF_GPU_ROUTE_MAX_INTERFACES + 1] = {0};   // counts, then each bin's next place
  for (uint32_t f = 0; f < n; ++f) ++at[bin_of(verdicts[f], num_interfaces)];
  for (uint32_t k = 0; counts && k <= num_interfaces; ++k) counts[k] = at[k];
  uint64_t ntx = 0;
  for (uint32_t k = 0; k < num_interfaces; ++k) {   // base_k = the frames of the interfaces before k
    const uint64_t c = at[k];
    at[k] = ntx;
    ntx += c;
  }
  at[num_interfaces] = 0;
  for (uint32_t f = 0; f < n; ++f) {
    const uint32_t b = bin_of(verdicts[f], num_interfaces);
    const uint64_t r = at[b]++;
    if (b < num_interfaces) {
      tx_descs[r].addr = descs[f].addr;   // the original address, as `orig` at src/xsknf.c:507
      tx_descs[r].len = descs[f].len;
      tx_descs[r].options = 0;            // xsknf_rt.c:586
      if (order) order[r] = f;
    } else {
      fill_addrs[r] = descs[f].addr;
      if (order) order[ntx + r] = f;
    }
  }
  return 0;
}

}  // extern "C"
