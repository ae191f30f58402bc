// plan_device.h -- the device-side shard planner as the library's own sources
// call it (plan_device.hip; the public calls are in include/xsknf_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

namespace xsknf_gpu {

// Bytes of planner workspace for n descriptors (host arithmetic only).
uint64_t plan_dev_workspace_bytes(uint64_t n);

// xsknf_gpu_shard_plan_dev without its argument checks, on the current device:
// plans into out_descs (device), fills bounds[nshards + 1], aux (spans[2 *
// nshards] or sizes[nshards]; may be NULL) and frame_bytes[nshards] (may be
// NULL) in host memory, and returns once they are filled.  0, or -EIO / -ENOMEM
// with the library's error text set.
int plan_dev_run(const xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_addr, uint64_t umem_size, uint32_t nshards,
                 int mode, xsknf_gpu_desc *out_descs, uint64_t *bounds, uint64_t *aux, uint64_t *frame_bytes,
                 void *workspace, hipStream_t stream);

}  // namespace xsknf_gpu
