// forward_device.hip -- routed frames copied into their tx interface's UMEM on
// the device (include/xsknf_gpu.h xsknf_gpu_forward_frames): the copy of
// src/xsknf.c:563-571 for the tx lists xsknf_gpu_route_batch leaves in device
// memory.  The destination UMEMs and the stats equal forward_host.cpp's byte for
// byte.
//
// One kernel (kernel_forward.h) behind a 24-byte memset of the stats, both on
// the caller's stream.  Bytes moved: 16 B read per entry of a copied interface,
// each frame's bytes read once and written once.
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_forward.h"

namespace xsknf_gpu {

using namespace forward;

static_assert(XSKNF_GPU_FORWARD_STATS == 3, "frames, bytes, skipped");

}  // namespace xsknf_gpu

extern "C" {

int xsknf_gpu_forward_frames(const uint8_t *rx_umem, uint64_t rx_umem_size, uint8_t *const *tx_umems,
                             const uint64_t *tx_umem_sizes, uint32_t num_interfaces,
                             const struct xsknf_gpu_desc *tx_descs, const uint64_t *counts_dev, uint32_t n,
                             uint64_t *stats_dev, uint64_t *stats, void *stream) {
  using namespace xsknf_gpu;
  const int rc = check_args(rx_umem, rx_umem_size, tx_umems, tx_umem_sizes, num_interfaces, tx_descs, counts_dev, n,
                            stats_dev, true);
  if (rc) return rc;
  TxUmems tx = {};
  bool any = false;
  for (uint32_t i = 0; i < num_interfaces; ++i) {
    if (!tx_umems[i] || tx_umems[i] == rx_umem) continue;   // shares the rx UMEM: nothing to copy
    tx.base[i] = tx_umems[i];
    tx.size[i] = tx_umem_sizes[i];
    any = true;
  }
  for (int k = 0; stats && k < XSKNF_GPU_FORWARD_STATS; ++k) stats[k] = 0;
  if (n == 0) return 0;   // nothing on the device is touched
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(stats_dev, 0, sizeof(uint64_t) * XSKNF_GPU_FORWARD_STATS, s);
  if (e == hipSuccess && any) {
    const uint64_t want = (static_cast<uint64_t>(n) + kThreads - 1) / kThreads;   // a wave per 64 entries
    const unsigned grid = static_cast<unsigned>(want < kMaxBlocks ? want : kMaxBlocks);
    hipLaunchKernelGGL(forward_frames, dim3(grid), dim3(kThreads), 0, s, rx_umem, rx_umem_size, tx, num_interfaces,
                       tx_descs, counts_dev, n, reinterpret_cast<unsigned long long *>(stats_dev));
    e = hipGetLastError();
    uint64_t res[XSKNF_GPU_FORWARD_STATS];
    if (e == hipSuccess && stats) {
      e = hipMemcpyAsync(res, stats_dev, sizeof(res), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      for (int k = 0; e == hipSuccess && k < XSKNF_GPU_FORWARD_STATS; ++k) stats[k] = res[k];
    }
  }
  if (e != hipSuccess) {
    set_error(e, "device forward");
    return -EIO;
  }
  return 0;
}

}  // extern "C"
