// macswap_device.hip -- the macswap NF on the device (include/xsknf_gpu.h
// xsknf_gpu_macswap_batch): what the reference's callback
// (examples/macswap/macswap_user.c:34-50) does frame by frame, for a UMEM and
// descriptors that lie in device memory.  The frames and the verdicts equal
// macswap_host.cpp's byte for byte; the verdicts are what xsknf_gpu_route_batch
// consumes next on the same stream.
//
// One pass (kernel_macswap.h), one launch, nothing waiting on another block.
// A frame moves its 16 B descriptor in, the 12 address bytes in (as 3 or 4
// aligned words) and out (as 3 to 5 naturally aligned stores that cover those
// 12 bytes and no other), and its 4 B verdict out: 44 to 48 bytes.  With a
// double swap the frame is neither read nor written: 20 bytes.  A translation
// unit of its own: none of the checksummer's kernels is rebuilt for it.
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_macswap.h"
#include "macswap_rules.h"

extern "C" {

int xsknf_gpu_macswap_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                            uint32_t ingress_ifindex, const struct xsknf_macswap_opts *opts, int32_t *verdicts,
                            void *stream) {
  using namespace xsknf_gpu;
  macswap::Args a;
  const int rc = macswap::forward_verdict(opts, ingress_ifindex, &a.fwd_verdict);
  if (rc) return rc;
  // 16-byte loads of the records, aligned words of the UMEM, 4-byte verdict stores
  if ((reinterpret_cast<uintptr_t>(umem) | reinterpret_cast<uintptr_t>(descs)) & 15) return -EINVAL;
  if (reinterpret_cast<uintptr_t>(verdicts) & 3) return -EINVAL;
  if (n == 0) return 0;   // no launch
  if (!umem || !descs || !verdicts) return -EINVAL;
  a.umem = umem;
  a.umem_size = umem_size;
  a.descs = reinterpret_cast<const uint4 *>(descs);
  a.verdicts = verdicts;
  a.n = n;
  a.swap = opts->double_macswap == 0;
  const uint32_t tiles = n / macswap::kThreads + (n % macswap::kThreads != 0);   // (no sum that can wrap)
  const dim3 grid(tiles < static_cast<uint32_t>(macswap::kMaxBlocks) ? tiles : macswap::kMaxBlocks);
  hipLaunchKernelGGL(macswap::macswap_pass, grid, dim3(macswap::kThreads), 0, static_cast<hipStream_t>(stream), a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(e, "device macswap");
    return -EIO;
  }
  return 0;
}

}  // extern "C"
