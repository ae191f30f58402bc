// forward_host.cpp -- routed frames copied into their tx interface's UMEM on
// one CPU thread (no GPU): include/xsknf_gpu.h xsknf_gpu_forward_host, the model
// the device forward (forward_device.hip) is held to, byte for byte.  The
// reference does this copy while it fills the destination's tx ring
// (src/xsknf.c:563-571, the __builtin_memcpy at :565); here the lists of a
// routed batch (route_host.cpp) are walked interface by interface, as
// xsknf_rt.c dispose_multi does with its memcpy.  Plain C++, so that
// tests/test_forward.py can build it under AddressSanitizer + UBSan
// (tests/c/san_forward.c); linked into libxsknf_gpu.so with the HIP sources.
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "../../include/xsknf_gpu.h"
#include "desc_rules.h"
#include "forward_args.h"

extern "C" {

int xsknf_gpu_forward_host(const uint8_t *rx_umem, uint64_t rx_umem_size, uint8_t *const *tx_umems,
                           const uint64_t *tx_umem_sizes, uint32_t num_interfaces,
                           const struct xsknf_gpu_desc *tx_descs, const uint64_t *counts, uint64_t *stats) {
  using namespace xsknf_gpu::forward;
  // (host arrays: the caller's counts say how many entries there are, so any
  // non-empty list needs the arrays)
  uint64_t total = 0;
  if (num_interfaces && num_interfaces <= kMaxInterfaces && counts && !(reinterpret_cast<uintptr_t>(counts) & 7))
    for (uint32_t i = 0; i < num_interfaces; ++i) total += counts[i];
  const int rc = check_args(rx_umem, rx_umem_size, tx_umems, tx_umem_sizes, num_interfaces, tx_descs, counts,
                            total ? 1u : 0u, nullptr, false);
  if (rc) return rc;
  uint64_t st[XSKNF_GPU_FORWARD_STATS] = {0, 0, 0};
  uint64_t base = 0;
  for (uint32_t i = 0; i < num_interfaces && counts; ++i) {
    const uint64_t c = counts[i];
    uint8_t *dst = tx_umems[i];
    if (dst && dst != rx_umem) {   // (else the rx UMEM is this interface's own: :572-579)
      for (uint64_t j = base; j < base + c; ++j) {
        const uint64_t off = xsknf_gpu::desc_offset(tx_descs[j].addr);
        const uint32_t len = tx_descs[j].len;
        if (!xsknf_gpu::in_umem(off, len, rx_umem_size) || !xsknf_gpu::in_umem(off, len, tx_umem_sizes[i])) {
          ++st[2];
          continue;
        }
        if (len) memcpy(dst + off, rx_umem + off, len);
        ++st[0];
        st[1] += len;
      }
    }
    base += c;
  }
  for (int k = 0; stats && k < XSKNF_GPU_FORWARD_STATS; ++k) stats[k] = st[k];
  return 0;
}

}  // extern "C"
