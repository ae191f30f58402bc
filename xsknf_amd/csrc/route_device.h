// route_device.h -- the device-side router as the library's own sources call it
// (route_device.hip; the public calls are in include/xsknf_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

namespace xsknf_gpu {

// Bytes of router workspace for n frames in num_interfaces + 1 bins (host arithmetic only).
uint64_t route_workspace_bytes(uint32_t n, uint32_t num_interfaces);

// xsknf_gpu_route_batch without its argument checks, for n > 0, on the current
// device: enqueues the three passes on `stream`; with counts (host,
// num_interfaces + 1 words) it also reads the header back and returns once they
// are filled.  0, or -EIO with the library's error text set.
int route_run(const xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n, uint32_t num_interfaces,
              xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs, uint32_t *order, uint64_t *counts, void *workspace,
              hipStream_t stream);

}  // namespace xsknf_gpu
