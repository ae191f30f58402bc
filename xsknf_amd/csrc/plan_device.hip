// plan_device.hip -- the multi-device plan computed on the root device, for a
// batch whose rx descriptors already lie in its memory (include/xsknf_gpu.h
// xsknf_gpu_shard_plan_dev; xsknf_gpu_multi_scatter_dev in multi.hip plans with
// it).  The outputs equal shard_plan.cpp's bit for bit: the cuts of
// xsknf_gpu_shard_plan, per-shard byte sums, and either the spans and rebased
// descriptors (xsknf_gpu_shard_rebase per shard) or the packed descriptors and
// sizes of xsknf_gpu_shard_pack_plan.
//
// Passes (kernel_plan.h), all on one stream, none waiting on another block:
//   span mode   block totals, scan of the totals, cuts, spans, rebase:
//               the descriptors read three times and written once, 64 B / frame;
//   packed mode block totals, scan of the totals, cuts, pack:
//               read twice, written once, 48 B / frame
// (plus, per cut, one tile of kTile descriptors).  The cut comparison is the
// host's own, in double: double(running bytes) < double(total * r) / nshards,
// with IEEE conversion and division on both sides -- build without fast-math.
// Sums are u64 throughout (a len is a full u32; descriptors outside the UMEM
// still count toward the total).
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_plan.h"
#include "plan_device.h"

namespace xsknf_gpu {

using namespace plan;

uint64_t plan_dev_workspace_bytes(uint64_t n) {
  const uint64_t nb = (n + kTile - 1) / kTile;
  return sizeof(uint64_t) * (kHeaderWords + 2 * (nb + 1));
}

int plan_dev_run(const xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_addr, uint64_t umem_size, uint32_t nshards,
                 int mode, xsknf_gpu_desc *out_descs, uint64_t *bounds, uint64_t *aux, uint64_t *frame_bytes,
                 void *workspace, hipStream_t stream) {
  const int packed = mode == XSKNF_GPU_PLAN_PACKED;
  const uint32_t naux = packed ? nshards : 2 * nshards;
  if (n == 0) {   // (shard_plan.cpp: every cut 0, every span / size 0)
    for (uint32_t k = 0; k <= nshards; ++k) bounds[k] = 0;
    for (uint32_t k = 0; aux && k < naux; ++k) aux[k] = 0;
    for (uint32_t k = 0; frame_bytes && k < nshards; ++k) frame_bytes[k] = 0;
    return 0;
  }
  const uint64_t nb = (n + kTile - 1) / kTile;
  if (nb > 0x7fffffffull) return -EINVAL;   // (a grid's x limit: 2^42 frames)
  uint64_t *ws = static_cast<uint64_t *>(workspace);
  const uint4 *in = reinterpret_cast<const uint4 *>(descs);
  uint4 *out = reinterpret_cast<uint4 *>(out_descs);
  const dim3 grid(static_cast<unsigned>(nb)), block(kThreads);
  const int N = static_cast<int>(nshards);
  hipLaunchKernelGGL(plan_block_totals, grid, block, 0, stream, in, n, umem_addr, umem_size, packed,
                     ws + kHeaderWords, ws + kHeaderWords + nb + 1);
  hipLaunchKernelGGL(plan_scan_totals, dim3(1), block, 0, stream, ws, nb, n, N, packed);
  if (N > 1)
    hipLaunchKernelGGL(plan_cuts, dim3(N - 1), block, 0, stream, in, n, umem_addr, umem_size, nb, packed, ws);
  if (packed) {
    hipLaunchKernelGGL(plan_pack, grid, block, 0, stream, in, n, umem_addr, umem_size, nb, N, ws, out);
  } else {
    hipLaunchKernelGGL(plan_spans, grid, block, 0, stream, in, n, umem_size, N, ws);
    hipLaunchKernelGGL(plan_rebase, grid, block, 0, stream, in, n, umem_size, N, ws, out);
  }
  hipError_t e = hipGetLastError();
  // the host's share, one small copy: the cuts, the byte sums, the spans or sizes
  uint64_t res[kResultWords];
  if (e == hipSuccess) e = hipMemcpyAsync(res, ws, sizeof(res), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) {
    set_error(e, "device shard plan");
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
  }
  for (uint32_t k = 0; k <= nshards; ++k) bounds[k] = res[kBounds + k];
  for (uint32_t k = 0; aux && k < naux; ++k) aux[k] = res[kAux + k];
  for (uint32_t k = 0; frame_bytes && k < nshards; ++k) frame_bytes[k] = res[kBytes + k];
  return 0;
}

}  // namespace xsknf_gpu

extern "C" {

int xsknf_gpu_shard_plan_dev_workspace(uint64_t n, uint32_t nshards, uint64_t *bytes) {
  if (nshards == 0 || nshards > xsknf_gpu::plan::kMaxShards || !bytes) return -EINVAL;
  *bytes = xsknf_gpu::plan_dev_workspace_bytes(n);
  return 0;
}

int xsknf_gpu_shard_plan_dev(const struct xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_addr, uint64_t umem_size,
                             uint32_t nshards, int mode, struct xsknf_gpu_desc *out_descs, uint64_t *bounds,
                             uint64_t *spans_or_sizes, uint64_t *frame_bytes, void *workspace,
                             uint64_t workspace_bytes, void *stream) {
  if (nshards == 0 || nshards > xsknf_gpu::plan::kMaxShards || !bounds) return -EINVAL;
  if (mode != XSKNF_GPU_PLAN_SPAN && mode != XSKNF_GPU_PLAN_PACKED) return -EINVAL;
  if (n) {
    if (!descs || !out_descs || !workspace) return -EINVAL;
    if (workspace_bytes < xsknf_gpu::plan_dev_workspace_bytes(n)) return -EINVAL;
    // 16-byte loads and stores of the records, 8-byte words of workspace
    if ((reinterpret_cast<uintptr_t>(descs) | reinterpret_cast<uintptr_t>(out_descs)) & 15) return -EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return -EINVAL;
  }
  return xsknf_gpu::plan_dev_run(descs, n, umem_addr, umem_size, nshards, mode, out_descs, bounds, spans_or_sizes,
                                 frame_bytes, workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
