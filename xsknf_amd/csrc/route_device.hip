// route_device.hip -- a checksummed batch routed on the device
// (include/xsknf_gpu.h xsknf_gpu_route_batch): the per-interface tx lists and
// the fill list that process_batch / process_batch_1if (src/xsknf.c:503-522,
// :654-672) build frame by frame, for verdicts and descriptors that lie in
// device memory.  The outputs equal route_host.cpp's bit for bit.
//
// Passes (kernel_route.h), all on one stream, none waiting on another block:
//   tile counts   4 B / frame read (the verdicts);
//   scan          (num_interfaces + 1) x tiles u32, read and written once;
//   scatter       4 + 16 B / frame read, 16 B per tx frame or 8 B per drop
//                 written, 4 B more with `order`.
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_route.h"
#include "route_device.h"

namespace xsknf_gpu {

using namespace route;

static_assert(XSKNF_GPU_ROUTE_MAX_INTERFACES == XSKNF_MAX_INTERFACES, "a tx list per interface of the runtime");

uint64_t route_workspace_bytes(uint32_t n, uint32_t num_interfaces) {
  const uint64_t nb = (static_cast<uint64_t>(n) + kTile - 1) / kTile;
  const uint64_t cnt = sizeof(uint32_t) * (num_interfaces + 1ull) * nb;
  return sizeof(uint64_t) * kHeaderWords + ((cnt + 7) & ~7ull);
}

int route_run(const xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n, uint32_t num_interfaces,
              xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs, uint32_t *order, uint64_t *counts, void *workspace,
              hipStream_t stream) {
  const uint64_t nb = (static_cast<uint64_t>(n) + kTile - 1) / kTile;   // (< 2^21: within a grid's x limit)
  uint64_t *hdr = static_cast<uint64_t *>(workspace);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(hdr + kHeaderWords);
  const dim3 grid(static_cast<unsigned>(nb)), block(kThreads);
  hipLaunchKernelGGL(route_tile_counts, grid, block, 0, stream, verdicts, n, num_interfaces, nb, cnt);
  hipLaunchKernelGGL(route_scan_counts, dim3(num_interfaces + 1), block, 0, stream, cnt, nb, hdr);
  hipLaunchKernelGGL(route_scatter, grid, block, 0, stream, reinterpret_cast<const uint4 *>(descs), verdicts, n,
                     num_interfaces, nb, hdr, cnt, reinterpret_cast<uint4 *>(tx_descs), fill_addrs, order);
  hipError_t e = hipGetLastError();
  uint64_t res[kMaxBins];
  if (e == hipSuccess && counts) {
    // the host's share, one small copy: the counts
    e = hipMemcpyAsync(res, hdr, sizeof(uint64_t) * (num_interfaces + 1), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
  }
  if (e != hipSuccess) {
    set_error(e, "device route");
    return -EIO;
  }
  for (uint32_t k = 0; counts && k <= num_interfaces; ++k) counts[k] = res[k];
  return 0;
}

}  // namespace xsknf_gpu

extern "C" {

int xsknf_gpu_route_workspace(uint32_t n, uint32_t num_interfaces, uint64_t *bytes) {
  if (num_interfaces == 0 || num_interfaces > XSKNF_GPU_ROUTE_MAX_INTERFACES || !bytes) return -EINVAL;
  *bytes = xsknf_gpu::route_workspace_bytes(n, num_interfaces);
  return 0;
}

int xsknf_gpu_route_batch(const struct xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n,
                          uint32_t num_interfaces, struct xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs,
                          uint32_t *order, uint64_t *counts, void *workspace, uint64_t workspace_bytes,
                          void *stream) {
  if (num_interfaces == 0 || num_interfaces > XSKNF_GPU_ROUTE_MAX_INTERFACES) return -EINVAL;
  // 16-byte loads and stores of the records, 8-byte words of addresses and workspace
  if ((reinterpret_cast<uintptr_t>(descs) | reinterpret_cast<uintptr_t>(tx_descs)) & 15) return -EINVAL;
  if ((reinterpret_cast<uintptr_t>(fill_addrs) | reinterpret_cast<uintptr_t>(workspace)) & 7) return -EINVAL;
  if ((reinterpret_cast<uintptr_t>(verdicts) | reinterpret_cast<uintptr_t>(order)) & 3) return -EINVAL;
  if (n == 0) {   // no launch; nothing is written but the caller's counts
    for (uint32_t k = 0; counts && k <= num_interfaces; ++k) counts[k] = 0;
    return 0;
  }
  if (!descs || !verdicts || !tx_descs || !fill_addrs || !workspace) return -EINVAL;
  if (workspace_bytes < xsknf_gpu::route_workspace_bytes(n, num_interfaces)) return -EINVAL;
  return xsknf_gpu::route_run(descs, verdicts, n, num_interfaces, tx_descs, fill_addrs, order, counts, workspace,
                              static_cast<hipStream_t>(stream));
}

}  // extern "C"
