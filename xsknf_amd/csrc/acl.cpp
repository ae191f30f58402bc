// acl.cpp -- the firewall's ACL (include/xsknf_gpu.h xsknf_gpu_acl_*): the
// reference's rule file read (init_acl, examples/firewall/firewall_user.c:53-116)
// and the rules built into the open-addressing table of acl_table.h on one host
// thread.  Plain C++; the only GPU calls are the table's allocation, upload and
// release, and a build with XSKNF_ACL_HOST_ONLY has none (the sanitizer program,
// tests/c/san_firewall.c, links this file and firewall_host.cpp alone).
#include <arpa/inet.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>

#include "acl_table.h"

#ifndef XSKNF_ACL_HOST_ONLY
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
namespace xsknf_gpu {
void set_error(hipError_t e, const char *where);   // checksummer.hip
}
#endif

namespace {

using xsknf_gpu::AclKey;

// the reference's buffers (firewall_user.c:30-32), less the terminator
constexpr size_t kIpChars = 15, kProtoChars = 3, kActionChars = 4;

// the next white-space separated token of [p, end), as fscanf's %s takes it
bool next_token(const char *&p, const char *end, const char *&tok, size_t &len) {
  while (p < end && (*p == ' ' || (*p >= '\t' && *p <= '\r'))) ++p;
  if (p == end) return false;
  tok = p;
  while (p < end && !(*p == ' ' || (*p >= '\t' && *p <= '\r'))) ++p;
  len = static_cast<size_t>(p - tok);
  return true;
}

// a decimal number below 2^32, the whole token
bool parse_u32(const char *tok, size_t len, uint32_t &out) {
  if (len == 0 || len > 10) return false;
  uint64_t v = 0;
  for (size_t i = 0; i < len; ++i) {
    if (tok[i] < '0' || tok[i] > '9') return false;
    v = v * 10 + static_cast<uint64_t>(tok[i] - '0');
  }
  if (v > 0xffffffffull) return false;
  out = static_cast<uint32_t>(v);
  return true;
}

bool parse_addr(const char *tok, size_t len, uint32_t &out) {
  if (len > kIpChars || memchr(tok, 0, len)) return false;
  char buf[kIpChars + 1];
  memcpy(buf, tok, len);
  buf[len] = 0;
  struct in_addr a;
  if (!inet_aton(buf, &a)) return false;
  out = a.s_addr;
  return true;
}

void free_acl(xsknf_gpu_acl *acl) {
  free(acl->keys);
  free(acl->actions);
  delete acl;
}

}  // namespace

extern "C" {

int xsknf_gpu_acl_parse(const char *path, struct xsknf_gpu_acl_rule *rules_out, uint32_t cap, uint32_t *n_out) {
  if (!path || !n_out || (cap && !rules_out)) return -EINVAL;
  FILE *f = fopen(path, "r");
  if (!f) return -errno;
  std::string text;
  char buf[65536];
  size_t got;
  try {
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
  } catch (const std::bad_alloc &) {
    fclose(f);
    return -ENOMEM;
  }
  const int rerr = ferror(f) ? (errno ? errno : EIO) : 0;
  fclose(f);
  if (rerr) return -rerr;

  const char *p = text.data(), *end = p + text.size(), *tok;
  size_t len;
  uint32_t count;
  if (!next_token(p, end, tok, len) || !parse_u32(tok, len, count)) return -EINVAL;
  if (count > XSKNF_GPU_ACL_MAX_RULES) return -EINVAL;
  uint32_t i = 0;
  while (next_token(p, end, tok, len)) {
    if (i == count) return -EINVAL;   // more records than the first line says
    struct xsknf_gpu_acl_rule r;
    memset(&r, 0, sizeof(r));
    uint32_t port;
    if (!parse_addr(tok, len, r.saddr)) return -EINVAL;
    if (!next_token(p, end, tok, len) || !parse_addr(tok, len, r.daddr)) return -EINVAL;
    if (!next_token(p, end, tok, len) || !parse_u32(tok, len, port)) return -EINVAL;
    r.sport = htons(static_cast<uint16_t>(port));
    if (!next_token(p, end, tok, len) || !parse_u32(tok, len, port)) return -EINVAL;
    r.dport = htons(static_cast<uint16_t>(port));
    if (!next_token(p, end, tok, len)) return -EINVAL;
    if (len == kProtoChars && !memcmp(tok, "TCP", 3)) r.proto = 6;
    else if (len == kProtoChars && !memcmp(tok, "UDP", 3)) r.proto = 17;
    else return -EINVAL;
    if (!next_token(p, end, tok, len) || len > kActionChars || memchr(tok, 0, len)) return -EINVAL;
    char act[kActionChars + 1];
    memcpy(act, tok, len);
    act[len] = 0;
    r.action = strcmp(act, "DROP") == 0 ? -1 : atoi(act);
    if (i < cap) rules_out[i] = r;
    ++i;
  }
  if (i != count) return -EINVAL;
  *n_out = count;
  return count > cap ? -ENOSPC : 0;
}

int xsknf_gpu_acl_create(struct xsknf_gpu_acl **acl_out, const struct xsknf_gpu_acl_rule *rules, uint32_t n,
                         uint32_t slots) {
  if (!acl_out || (n && !rules)) return -EINVAL;
  if (slots == 0) {
    if (n > XSKNF_GPU_ACL_MAX_SLOTS / 2) return -EINVAL;
    slots = 64;
    while (slots < 2 * n) slots *= 2;
  } else if ((slots & (slots - 1)) || slots > XSKNF_GPU_ACL_MAX_SLOTS) {
    return -EINVAL;
  }
  xsknf_gpu_acl *acl = new (std::nothrow) xsknf_gpu_acl();
  if (!acl) return -ENOMEM;
  acl->slots = slots;
  acl->keys = static_cast<AclKey *>(calloc(slots, sizeof(AclKey)));
  acl->actions = static_cast<int32_t *>(calloc(slots, sizeof(int32_t)));
  if (!acl->keys || !acl->actions) {
    free_acl(acl);
    return -ENOMEM;
  }
  const uint32_t mask = slots - 1;
  for (uint32_t i = 0; i < n; ++i) {
    const struct xsknf_gpu_acl_rule &r = rules[i];
    if (r.proto != 6 && r.proto != 17) continue;   // rule 5: no frame carries such a key to the table
    const AclKey k = {r.saddr, r.daddr, static_cast<uint32_t>(r.sport) | static_cast<uint32_t>(r.dport) << 16, r.proto};
    uint32_t s = xsknf_gpu::acl_hash(k.a, k.b, k.c, k.p) & mask, probes = 1;
    // ends: fewer than `slots` keys are ever stored
    while (acl->keys[s].p && !(acl->keys[s].a == k.a && acl->keys[s].b == k.b && acl->keys[s].c == k.c &&
                               acl->keys[s].p == k.p)) {
      s = (s + 1) & mask;
      ++probes;
    }
    if (!acl->keys[s].p) {
      if (acl->rules + 1 >= slots) {   // would take the last empty slot
        free_acl(acl);
        return -EINVAL;
      }
      acl->keys[s] = k;
      ++acl->rules;
      if (probes > acl->max_probe) acl->max_probe = probes;
    }
    acl->actions[s] = r.action;   // the last rule of a key wins
  }
#ifndef XSKNF_ACL_HOST_ONLY
  const size_t kb = sizeof(AclKey) * slots, ab = sizeof(int32_t) * slots;
  void *d = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    // a process without a device: the ACL serves xsknf_gpu_firewall_host alone
    // (xsknf_gpu_firewall_batch refuses it)
    (void)hipGetLastError();
    *acl_out = acl;
    return 0;
  }
  hipError_t e = hipMalloc(&d, kb + ab);
  if (e == hipSuccess) e = hipMemcpy(d, acl->keys, kb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(static_cast<char *>(d) + kb, acl->actions, ab, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    xsknf_gpu::set_error(e, "ACL upload");
    if (d) (void)hipFree(d);
    free_acl(acl);
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
  }
  acl->d_keys = static_cast<AclKey *>(d);
  acl->d_actions = reinterpret_cast<int32_t *>(static_cast<char *>(d) + kb);
#endif
  *acl_out = acl;
  return 0;
}

int xsknf_gpu_acl_info(const struct xsknf_gpu_acl *acl, struct xsknf_gpu_acl_info *info) {
  if (!acl || !info) return -EINVAL;
  info->rules = acl->rules;
  info->slots = acl->slots;
  info->max_probe = acl->max_probe;
  info->reserved = 0;
  info->device_bytes = acl->d_keys ? (sizeof(AclKey) + sizeof(int32_t)) * static_cast<uint64_t>(acl->slots) : 0;
  return 0;
}

int xsknf_gpu_acl_destroy(struct xsknf_gpu_acl *acl) {
  if (!acl) return -EINVAL;
  int rc = 0;
#ifndef XSKNF_ACL_HOST_ONLY
  if (acl->d_keys) {
    const hipError_t e = hipFree(acl->d_keys);
    if (e != hipSuccess) {
      xsknf_gpu::set_error(e, "ACL release");
      rc = -EIO;
    }
  }
#endif
  free_acl(acl);
  return rc;
}

}  // extern "C"
