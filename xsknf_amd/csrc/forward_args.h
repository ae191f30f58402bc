// forward_args.h -- what the two forms of the frame forward (forward_host.cpp,
// forward_device.hip; include/xsknf_gpu.h xsknf_gpu_forward_*) share: the
// argument checks.  Plain C++, no GPU call, so that forward_host.cpp builds
// without HIP.
#pragma once
#include <errno.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

namespace xsknf_gpu {
namespace forward {

constexpr uint32_t kMaxInterfaces = XSKNF_GPU_ROUTE_MAX_INTERFACES;

inline bool overlap(uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) {
  return na && nb && a < b + nb && b < a + na;
}

// The checks of both calls, in the header's order.  0, or -EINVAL.
inline int check_args(const uint8_t *rx_umem, uint64_t rx_umem_size, uint8_t *const *tx_umems,
                      const uint64_t *tx_umem_sizes, uint32_t num_interfaces, const void *tx_descs,
                      const void *counts, uint32_t n, const void *stats_dev, bool need_stats_dev) {
  if (num_interfaces == 0 || num_interfaces > kMaxInterfaces) return -EINVAL;
  if (!tx_umems || !tx_umem_sizes) return -EINVAL;
  const uintptr_t rx = reinterpret_cast<uintptr_t>(rx_umem);
  if (rx & 15) return -EINVAL;
  for (uint32_t i = 0; i < num_interfaces; ++i) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(tx_umems[i]);
    if (p & 15) return -EINVAL;
    if (!p || p == rx) continue;   // shares the rx UMEM
    if (rx && overlap(p, tx_umem_sizes[i], rx, rx_umem_size)) return -EINVAL;
    for (uint32_t j = 0; j < i; ++j) {
      const uintptr_t q = reinterpret_cast<uintptr_t>(tx_umems[j]);
      if (q && q != rx && q != p && overlap(p, tx_umem_sizes[i], q, tx_umem_sizes[j])) return -EINVAL;
    }
  }
  if (reinterpret_cast<uintptr_t>(tx_descs) & 15) return -EINVAL;
  if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(stats_dev)) & 7) return -EINVAL;
  if (n && (!rx_umem || !tx_descs || !counts || (need_stats_dev && !stats_dev))) return -EINVAL;
  return 0;
}

}  // namespace forward
}  // namespace xsknf_gpu
