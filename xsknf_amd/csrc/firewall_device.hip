// firewall_device.hip -- the firewall NF's verdicts on the device
// (include/xsknf_gpu.h xsknf_gpu_firewall_batch): what the reference's callback
// (examples/firewall/firewall_user.c:128-186) returns frame by frame, for a
// UMEM, descriptors and an ACL table (acl.cpp, acl_table.h) that lie in device
// memory.  The verdicts equal firewall_host.cpp's bit for bit and are what
// xsknf_gpu_route_batch consumes next on the same stream.
//
// One pass (kernel_firewall.h), one launch, nothing waiting on another block:
//   lookup   16 B descriptor + the frame's header sectors read, 16 B per probe
//            (+ 4 B on a hit) of the table read, 4 B verdict written per frame.
// The UMEM is only read.  A translation unit of its own: none of the
// checksummer's kernels is rebuilt for it.
// An ACL with hit counters (xsknf_gpu_acl_counters_enable) takes the counting
// twin of that launch instead (kernel_firewall_count.h): the same reads, and
// per block two 8-byte atomic adds for every distinct rule its frames hit.
#include <errno.h>
#ifdef XSKNF_AB
#include <stdlib.h>
#include <string.h>
#endif

#include "checksummer_internal.h"
#include "kernel_firewall.h"
#include "kernel_firewall_count.h"

extern "C" {

int xsknf_gpu_firewall_batch(const uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                             const struct xsknf_gpu_acl *acl, int32_t *verdicts, void *stream) {
  using namespace xsknf_gpu;
  if (!acl) return -EINVAL;
  // 16-byte loads of the records, aligned words of the UMEM, 4-byte verdict stores
  if ((reinterpret_cast<uintptr_t>(umem) | reinterpret_cast<uintptr_t>(descs)) & 15) return -EINVAL;
  if (reinterpret_cast<uintptr_t>(verdicts) & 3) return -EINVAL;
  if (n == 0) return 0;   // no launch
  if (!umem || !descs || !verdicts) return -EINVAL;
  if (!acl->d_keys) {
    set_error_text("the ACL was created without a device: it serves xsknf_gpu_firewall_host only");
    return -ENODEV;
  }
  firewall::Args a;
  a.umem = umem;
  a.umem_size = umem_size;
  a.descs = reinterpret_cast<const uint4 *>(descs);
  a.keys = acl->d_keys;
  a.actions = acl->d_actions;
  a.verdicts = verdicts;
  a.n = n;
  a.slots = acl->slots;
  const uint32_t tiles = n / firewall::kThreads + (n % firewall::kThreads != 0);   // (no sum that can wrap)
  const dim3 grid(tiles < static_cast<uint32_t>(firewall::kMaxBlocks) ? tiles : firewall::kMaxBlocks);
  if (acl->d_ctr) {
    const firewall::CountArgs c = {a, acl->d_ctr, reinterpret_cast<unsigned long long *>(acl->d_totals)};
    const hipStream_t hs = static_cast<hipStream_t>(stream);
#ifdef XSKNF_AB
    // XSKNF_ACL_COUNT_SHAPE=naive|wave|stage: the shapes the product's is compared with (kernel_firewall_count.h)
    static const char *const shape_env = getenv("XSKNF_ACL_COUNT_SHAPE");
    static const int shape = !shape_env ? firewall::kStageRepeats : !strcmp(shape_env, "naive") ? firewall::kNaive
                             : !strcmp(shape_env, "wave") ? firewall::kWave
                             : !strcmp(shape_env, "stage") ? firewall::kStageAll : firewall::kStageRepeats;
    if (shape == firewall::kNaive) hipLaunchKernelGGL(firewall::firewall_lookup_count<firewall::kNaive>, grid, dim3(firewall::kThreads), 0, hs, c);
    else if (shape == firewall::kWave) hipLaunchKernelGGL(firewall::firewall_lookup_count<firewall::kWave>, grid, dim3(firewall::kThreads), 0, hs, c);
    else if (shape == firewall::kStageAll) hipLaunchKernelGGL(firewall::firewall_lookup_count<firewall::kStageAll>, grid, dim3(firewall::kThreads), 0, hs, c);
    else
#endif
    hipLaunchKernelGGL(firewall::firewall_lookup_count<firewall::kStageRepeats>, grid, dim3(firewall::kThreads), 0, hs, c);
  } else {
    hipLaunchKernelGGL(firewall::firewall_lookup, grid, dim3(firewall::kThreads), 0, static_cast<hipStream_t>(stream), a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error(e, "device firewall");
    return -EIO;
  }
  return 0;
}

}  // extern "C"
