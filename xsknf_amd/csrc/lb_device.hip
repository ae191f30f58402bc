// lb_device.hip -- the load balancer NF on the device (include/xsknf_gpu.h
// xsknf_gpu_lb_batch, xsknf_gpu_lb_workspace): what the reference's loop over
// a batch (examples/load_balancer/load_balancer_user.c:396-553) leaves in the
// frames, the verdicts and the session table, for a UMEM, descriptors and
// tables (lb.cpp, lb_table.h) that lie in device memory.  The result equals
// lb_host.cpp's byte for byte; the verdicts are what xsknf_gpu_route_batch
// consumes next on the same stream.
// And the lbfw NF (xsknf_gpu_lbfw_batch; examples/lbfw/lbfw_user.c:420-594):
// the same batch with lbfw's PASS value and the firewall's ACL (acl.cpp) as a
// gate in front of the session lookup, equal to lbfw_host.cpp's result.
//
// Two memsets and four launches per batch (kernel_lb.h), no host read:
//   propose  parse, (lbfw: the ACL gate,) session and service lookups, the new
//            flows' keys staged
//   apply    sessions resolved, frames rewritten, verdicts
//   commit   the new sessions stored
//   ordered  one lane: the count, or the whole loop for a batch that stood down
// and, for an object with ageing alone (xsknf_gpu_lb_aging_enable), a fifth
// between commit and ordered (kernel_lb_stamp.h):
//   stamp    rule 11: the hit and the new sessions' last-seen stamps
// A translation unit of its own: none of the other kernels is rebuilt for it.
//
// Workspace: [16 header words][staging: S words, S the power of two >= 4 n, at
// least 64][state: n words, padded to 16 bytes][proposal records: 48 n bytes].
// The header and staging are zeroed per batch; the rest is written before it is
// read.
#include <errno.h>

#include "checksummer_internal.h"
#include "kernel_lb.h"
#include "kernel_lb_stamp.h"

namespace {

// Two fields of kernel_lb.h are sized by limits that include/xsknf_gpu.h sets:
// state[f] keeps a HIT's session slot in its low 24 bits (st & 0xffffff), and a
// staging word is enc(frame, kind) = (frame + 1) << 1 | kind in 32 bits.
static_assert(XSKNF_GPU_LB_MAX_SLOTS - 1 <= 0xffffffu, "a session slot must fit state[f]'s 24-bit slot field");
static_assert(((static_cast<uint64_t>(XSKNF_GPU_LB_MAX_BATCH - 1) + 1) << 1 | 1) <= 0xffffffffull,
              "enc(XSKNF_GPU_LB_MAX_BATCH - 1, 1) must fit a 32-bit staging word");

uint32_t stage_slots(uint32_t n) {
  uint32_t s = 64;
  while (s < 4ull * n) s *= 2;
  return s;
}
uint64_t state_bytes(uint32_t n) { return (4ull * n + 15) & ~15ull; }

// The argument rules both NFs share, then the batch.  gate.keys != nullptr
// selects lb_propose's gated instantiation.
int run_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n, uint32_t ingress,
              int32_t pass, const xsknf_gpu::lb::Gate &gate, struct xsknf_gpu_lb *lb, int32_t *verdicts, void *workspace,
              uint64_t workspace_bytes, uint64_t *stats_dev, void *stream, const char *what) {
  using namespace xsknf_gpu;
  hipStream_t s = static_cast<hipStream_t>(stream);
  lbk::Args a;
  a.umem = umem;
  a.umem_size = umem_size;
  a.descs = reinterpret_cast<const uint4 *>(descs);
  a.verdicts = verdicts;
  a.t = lb::Tables{lb->d_svc,     lb->d_bk,  lb->d_keys,       lb->d_vals,   lb->d_count,
                   lb->svc_slots, lb->slots, lb->max_sessions, lb->d_stamps, lb->d_clock};   // (stamps: NULL without ageing)
  a.stage_slots = stage_slots(n);
  char *w = static_cast<char *>(workspace);
  a.hdr = reinterpret_cast<uint32_t *>(w);
  a.staging = a.hdr + lbk::kHdrWords;
  a.state = a.staging + a.stage_slots;
  a.prop = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(a.state) + state_bytes(n));
  a.stats = reinterpret_cast<unsigned long long *>(stats_dev);
  a.n = n;
  a.ingress = ingress;
  a.pass = pass;
  a.gate = gate;
  hipError_t e = hipMemsetAsync(w, 0, 4ull * (lbk::kHdrWords + a.stage_slots), s);
  if (e == hipSuccess) e = hipMemsetAsync(stats_dev, 0, sizeof(uint64_t) * XSKNF_GPU_LB_STATS, s);
  if (e == hipSuccess) {
    const uint32_t tiles = n / lbk::kThreads + (n % lbk::kThreads != 0);   // (no sum that can wrap)
    const dim3 grid(tiles < static_cast<uint32_t>(lbk::kMaxBlocks) ? tiles : lbk::kMaxBlocks);
    if (gate.keys) hipLaunchKernelGGL(lbk::lb_propose<true>, grid, dim3(lbk::kThreads), 0, s, a);
    else hipLaunchKernelGGL(lbk::lb_propose<false>, grid, dim3(lbk::kThreads), 0, s, a);
    hipLaunchKernelGGL(lbk::lb_apply, grid, dim3(lbk::kThreads), 0, s, a);
    hipLaunchKernelGGL(lbk::lb_commit, grid, dim3(lbk::kThreads), 0, s, a);
    if (a.t.stamps) hipLaunchKernelGGL(lbk::lb_stamp, grid, dim3(lbk::kThreads), 0, s, a);
    hipLaunchKernelGGL(lbk::lb_ordered, dim3(1), dim3(64), 0, s, a);
    e = hipGetLastError();
  }
  if (e != hipSuccess) {
    set_error(e, what);
    return -EIO;
  }
  return 0;
}

// -EINVAL of both batch calls, before any GPU call; 1 when there is nothing to do.
int check_args(const uint8_t *umem, const struct xsknf_gpu_desc *descs, uint32_t n, const struct xsknf_gpu_lb *lb,
               const int32_t *verdicts, const void *workspace, uint64_t workspace_bytes, const uint64_t *stats_dev) {
  if (!lb || !stats_dev || n > XSKNF_GPU_LB_MAX_BATCH) return -EINVAL;
  // 16-byte loads of the records, aligned words of the UMEM, 4-byte verdict stores
  if ((reinterpret_cast<uintptr_t>(umem) | reinterpret_cast<uintptr_t>(descs) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return -EINVAL;
  if ((reinterpret_cast<uintptr_t>(verdicts) & 3) || (reinterpret_cast<uintptr_t>(stats_dev) & 7)) return -EINVAL;
  if (n == 0) return 1;   // no launch
  uint64_t need = 0;
  (void)xsknf_gpu_lb_workspace(n, &need);
  if (!umem || !descs || !verdicts || !workspace || workspace_bytes < need) return -EINVAL;
  return 0;
}

}  // namespace

extern "C" {

int xsknf_gpu_lb_workspace(uint32_t n, uint64_t *bytes) {
  using namespace xsknf_gpu;
  if (!bytes || n > XSKNF_GPU_LB_MAX_BATCH) return -EINVAL;
  *bytes = 4ull * lbk::kHdrWords + 4ull * stage_slots(n) + state_bytes(n) + 4ull * lbk::kPropWords * n;
  return 0;
}

int xsknf_gpu_lb_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                       uint32_t ingress_ifindex, uint32_t num_interfaces, struct xsknf_gpu_lb *lb, int32_t *verdicts,
                       void *workspace, uint64_t workspace_bytes, uint64_t *stats_dev, void *stream) {
  using namespace xsknf_gpu;
  const int rc = check_args(umem, descs, n, lb, verdicts, workspace, workspace_bytes, stats_dev);
  if (rc) return rc < 0 ? rc : 0;
  if (!lb->d_svc) {
    set_error_text("the load balancer was created without a device: it serves xsknf_gpu_lb_host only");
    return -ENODEV;
  }
  return run_batch(umem, umem_size, descs, n, ingress_ifindex, lb::pass_verdict(ingress_ifindex, num_interfaces),
                   lb::Gate{nullptr, nullptr, 0}, lb, verdicts, workspace, workspace_bytes, stats_dev, stream,
                   "device load balancer");
}

int xsknf_gpu_lbfw_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint32_t n,
                         uint32_t ingress_ifindex, uint32_t num_interfaces, const struct xsknf_gpu_acl *acl,
                         struct xsknf_gpu_lb *lb, int32_t *verdicts, void *workspace, uint64_t workspace_bytes,
                         uint64_t *stats_dev, void *stream) {
  using namespace xsknf_gpu;
  if (num_interfaces == 0) return -EINVAL;   // (the reference divides by zero)
  const int rc = check_args(umem, descs, n, lb, verdicts, workspace, workspace_bytes, stats_dev);
  if (rc) return rc < 0 ? rc : 0;
  if (!lb->d_svc) {
    set_error_text("the load balancer was created without a device: it serves xsknf_gpu_lbfw_host only");
    return -ENODEV;
  }
  if (acl && !acl->d_keys) {
    set_error_text("the ACL was created without a device: it serves xsknf_gpu_lbfw_host only");
    return -ENODEV;
  }
  // (d_ctr / d_totals: the ACL's hit counters, NULL unless enabled)
  const lb::Gate gate = acl ? lb::Gate{acl->d_keys, acl->d_actions, acl->slots, acl->d_ctr,
                                       reinterpret_cast<unsigned long long *>(acl->d_totals)}
                            : lb::Gate{nullptr, nullptr, 0, nullptr, nullptr};
  return run_batch(umem, umem_size, descs, n, ingress_ifindex, lb::lbfw_pass_verdict(ingress_ifindex, num_interfaces),
                   gate, lb, verdicts, workspace, workspace_bytes, stats_dev, stream, "device lbfw");
}

}  // extern "C"
