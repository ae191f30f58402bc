// macswap_rules.h -- what the macswap NF's options mean, stated once for the
// device call (macswap_device.hip) and the host model (macswap_host.cpp):
// include/xsknf_gpu.h "the macswap NF", rule 3 and the validation.
// Plain C++17, no GPU call: macswap_host.cpp builds with g++.
#pragma once
#include <errno.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"

namespace xsknf_gpu {
namespace macswap {

// 0 and the verdict of every frame that passes rules 0 and 1, or -EINVAL.
// (macswap_user.c:48-49: only DROP is tested for, so PASS redirects.)
inline int forward_verdict(const xsknf_macswap_opts *opts, uint32_t ingress_ifindex, int32_t *verdict) {
  if (!opts || opts->reserved != 0) return -EINVAL;
  if (opts->action > XSKNF_MACSWAP_ACTION_PASS) return -EINVAL;
  if (opts->action == XSKNF_MACSWAP_ACTION_DROP) {
    *verdict = -1;
    return 0;
  }
  if (opts->num_interfaces == 0) return -EINVAL;   // (the reference divides by zero)
  *verdict = static_cast<int32_t>((ingress_ifindex + 1u) % opts->num_interfaces);
  return 0;
}

}  // namespace macswap
}  // namespace xsknf_gpu
