// acl.cpp -- the firewall's ACL (include/xsknf_gpu.h xsknf_gpu_acl_*): the
// reference's rule file read (init_acl, examples/firewall/firewall_user.c:53-116)
// and the rules built into the open-addressing table of acl_table.h on one host
// thread, and the updates of a live table (xsknf_gpu_acl_update: tombstones, the
// rebuild in place, the dirty slots as records for acl_update_device.hip).
// Plain C++; the only GPU calls are the table's allocation, upload, read-back
// (_dump) and release, and a build with XSKNF_ACL_HOST_ONLY has none (the
// sanitizer programs, tests/c/san_firewall.c and san_acl_update.c, link this
// file and firewall_host.cpp alone).
#include <arpa/inet.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

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
  free(acl->probe_hist);
  free(acl->ctr);   // (the totals lie behind the counters)
  delete acl;
}

// ---- updates ------------------------------------------------------------------

using xsknf_gpu::AclCounter;
using xsknf_gpu::kAclNone;
using xsknf_gpu::kAclTombstoneP;

constexpr AclKey kTombstone = {0, 0, 0, kAclTombstoneP};
static_assert(xsknf_gpu::kAclTotals == XSKNF_GPU_ACL_TOTALS, "the totals of include/xsknf_gpu.h");
static_assert(XSKNF_GPU_ACL_MAX_SLOTS <= xsknf_gpu::kAclRecSlotMask, "a slot number leaves AclUpdateRec's flag bit free");

inline AclKey key_of(const struct xsknf_gpu_acl_rule &r) {
  return AclKey{r.saddr, r.daddr, static_cast<uint32_t>(r.sport) | static_cast<uint32_t>(r.dport) << 16, r.proto};
}
inline bool same(const AclKey &x, const AclKey &y) { return x.a == y.a && x.b == y.b && x.c == y.c && x.p == y.p; }
inline bool live(const AclKey &k) { return k.p != 0 && k.p != kAclTombstoneP; }

// Where key k is, or where it would go: the probe runs to the key or to an
// empty slot (one always remains) and remembers the first tombstone on its way.
struct Place {
  bool found;
  uint32_t slot, probes;   // the key's slot, or the first tombstone's, or else the empty slot's
};
Place place_of(const xsknf_gpu_acl *acl, const AclKey &k) {
  const uint32_t mask = acl->slots - 1;
  uint32_t s = xsknf_gpu::acl_hash(k.a, k.b, k.c, k.p) & mask, tomb = kAclNone, tomb_probes = 0;
  for (uint32_t probes = 1;; ++probes, s = (s + 1) & mask) {
    const AclKey &e = acl->keys[s];
    if (e.p == 0) return tomb != kAclNone ? Place{false, tomb, tomb_probes} : Place{false, s, probes};
    if (e.p == kAclTombstoneP) {
      if (tomb == kAclNone) {
        tomb = s;
        tomb_probes = probes;
      }
    } else if (same(e, k)) {
      return Place{true, s, probes};
    }
  }
}

// The same slot count, the live rules reinserted in ascending slot order of the
// old table, no tombstone left.  live_k / live_a: room for acl->rules entries.
// With counters, live_c and live_s as well: every key's counters go with it,
// and from[s] (`slots` entries) becomes the old slot of new slot s's key, or
// kAclNone -- the map the device's counters are carried by.
void rebuild_in_place(xsknf_gpu_acl *acl, AclKey *live_k, int32_t *live_a, AclCounter *live_c, uint32_t *live_s,
                      uint32_t *from) {
  uint32_t n = 0;
  for (uint32_t s = 0; s < acl->slots; ++s)
    if (live(acl->keys[s])) {
      live_k[n] = acl->keys[s];
      if (acl->ctr) {
        live_c[n] = acl->ctr[s];
        live_s[n] = s;
      }
      live_a[n++] = acl->actions[s];
    }
  memset(acl->keys, 0, sizeof(AclKey) * acl->slots);
  memset(acl->actions, 0, sizeof(int32_t) * acl->slots);
  if (acl->ctr) {
    memset(acl->ctr, 0, sizeof(AclCounter) * acl->slots);
    for (uint32_t s = 0; s < acl->slots; ++s) from[s] = kAclNone;
  }
  memset(acl->probe_hist, 0, sizeof(uint32_t) * (static_cast<size_t>(acl->max_probe) + 1));
  acl->max_probe = 0;
  acl->tombstones = 0;
  const uint32_t mask = acl->slots - 1;
  for (uint32_t i = 0; i < n; ++i) {
    const AclKey &k = live_k[i];
    uint32_t s = xsknf_gpu::acl_hash(k.a, k.b, k.c, k.p) & mask, probes = 1;
    while (acl->keys[s].p) {   // (the keys are distinct and fewer than the slots)
      s = (s + 1) & mask;
      ++probes;
    }
    acl->keys[s] = k;
    acl->actions[s] = live_a[i];
    if (acl->ctr) {
      acl->ctr[s] = live_c[i];
      from[s] = live_s[i];
    }
    ++acl->probe_hist[probes];
    if (probes > acl->max_probe) acl->max_probe = probes;
  }
}

// the live rules of a table, ascending by key
// (and, with ctr, each rule's counters into ctr_out)
int dump_table(const AclKey *keys, const int32_t *actions, uint32_t slots, struct xsknf_gpu_acl_rule *out, uint32_t cap,
               uint32_t *n_out, const AclCounter *ctr = nullptr, struct xsknf_gpu_acl_counter *ctr_out = nullptr) {
  std::vector<uint32_t> used;
  try {
    for (uint32_t s = 0; s < slots; ++s)
      if (live(keys[s])) used.push_back(s);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  std::sort(used.begin(), used.end(), [keys](uint32_t x, uint32_t y) {
    const AclKey &a = keys[x], &b = keys[y];
    if (a.a != b.a) return a.a < b.a;
    if (a.b != b.b) return a.b < b.b;
    if (a.c != b.c) return a.c < b.c;
    return a.p < b.p;
  });
  *n_out = static_cast<uint32_t>(used.size());
  for (uint32_t i = 0; i < used.size() && i < cap; ++i) {
    const AclKey &k = keys[used[i]];
    struct xsknf_gpu_acl_rule r;
    memset(&r, 0, sizeof(r));
    r.saddr = k.a;
    r.daddr = k.b;
    r.sport = static_cast<uint16_t>(k.c);
    r.dport = static_cast<uint16_t>(k.c >> 16);
    r.proto = static_cast<uint8_t>(k.p);
    r.action = actions[used[i]];
    out[i] = r;
    if (ctr) ctr_out[i] = {ctr[used[i]].packets, ctr[used[i]].bytes};
  }
  return used.size() > cap ? -ENOSPC : 0;
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
  acl->probe_hist = static_cast<uint32_t *>(calloc(static_cast<size_t>(slots) + 1, sizeof(uint32_t)));
  if (!acl->keys || !acl->actions || !acl->probe_hist) {
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
      ++acl->probe_hist[probes];
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
  info->tombstones = acl->tombstones;
  info->device_bytes = acl->d_keys ? (sizeof(AclKey) + sizeof(int32_t)) * static_cast<uint64_t>(acl->slots) + acl->d_ctr_bytes : 0;
  return 0;
}

int xsknf_gpu_acl_destroy(struct xsknf_gpu_acl *acl) {
  if (!acl) return -EINVAL;
  int rc = 0;
#ifndef XSKNF_ACL_HOST_ONLY
  if (acl->d_keys) {
    rc = xsknf_gpu::acl_staging_release(acl);
    if (xsknf_gpu::acl_counters_device_release(acl)) rc = -EIO;
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

int xsknf_gpu_acl_update(struct xsknf_gpu_acl *acl, const struct xsknf_gpu_acl_op *ops, uint32_t n, void *stream) {
  if (!acl || (n && !ops)) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (ops[i].op != XSKNF_GPU_ACL_PUT && ops[i].op != XSKNF_GPU_ACL_DELETE) return -EINVAL;
  if (n == 0) return 0;
  const uint32_t slots = acl->slots, mask = slots - 1;

  // Pass 1, nothing changed yet.  The last op of a key stands for the key: the
  // ops are walked backwards and a key seen before (in a scratch table of op
  // indices) is skipped.  What is left splits into the slots to delete and the
  // puts; both are applied in ascending op order, the deletes first, so the
  // table never holds more keys than before or after the call.
  // With counters a PUT whose key is in the map keeps the key's counters unless
  // an earlier op of the call deleted the key: again[i] marks such a final PUT.
  std::vector<uint32_t> seen, dels, puts, dirty;
  std::vector<uint8_t> again;
  uint32_t n_new = 0;
  AclKey *live_k = nullptr;
  int32_t *live_a = nullptr;
  AclCounter *live_c = nullptr;
  uint32_t *live_s = nullptr, *from = nullptr;
  bool rebuild = false;
  const auto drop = [&] {
    free(live_k);
    free(live_a);
    free(live_c);
    free(live_s);
    free(from);
  };
  try {
    if (acl->ctr) again.assign(n, 0);
    size_t cap = 16;
    while (cap < 2 * static_cast<size_t>(n)) cap *= 2;
    seen.assign(cap, kAclNone);
    for (uint32_t i = n; i-- > 0;) {
      const struct xsknf_gpu_acl_rule &r = ops[i].rule;
      if (r.proto != 6 && r.proto != 17) continue;   // rule 5: never in the table
      const AclKey k = key_of(r);
      size_t s = xsknf_gpu::acl_hash(k.a, k.b, k.c, k.p) & (cap - 1);
      while (seen[s] != kAclNone && !same(key_of(ops[seen[s]].rule), k)) s = (s + 1) & (cap - 1);
      if (seen[s] != kAclNone) {
        if (acl->ctr && ops[i].op == XSKNF_GPU_ACL_DELETE) again[seen[s]] = 1;
        continue;
      }
      seen[s] = i;
      const uint32_t at = xsknf_gpu::acl_find(acl->keys, slots, k.a, k.b, k.c, k.p);
      if (ops[i].op == XSKNF_GPU_ACL_DELETE) {
        if (at != kAclNone) dels.push_back(at);
      } else {
        puts.push_back(i);
        n_new += at == kAclNone;
      }
    }
    std::vector<uint32_t>().swap(seen);
    std::reverse(dels.begin(), dels.end());
    std::reverse(puts.begin(), puts.end());
    const uint64_t after = static_cast<uint64_t>(acl->rules) - dels.size() + n_new;
    if (after >= slots || after > XSKNF_GPU_ACL_MAX_RULES) return -ENOSPC;
    if (dels.empty() && puts.empty()) return 0;
    // the bound of acl_table.h, taken where the deletes are in and the puts are not
    const uint64_t tombs = static_cast<uint64_t>(acl->tombstones) + dels.size();
    rebuild = tombs > slots / xsknf_gpu::kAclTombstoneShare || after + tombs > slots - 1;
    if (rebuild) {
      const size_t keep = acl->rules - dels.size();
      live_k = static_cast<AclKey *>(malloc(sizeof(AclKey) * (keep ? keep : 1)));
      live_a = static_cast<int32_t *>(malloc(sizeof(int32_t) * (keep ? keep : 1)));
      if (!live_k || !live_a) throw std::bad_alloc();
      if (acl->ctr) {
        live_c = static_cast<AclCounter *>(malloc(sizeof(AclCounter) * (keep ? keep : 1)));
        live_s = static_cast<uint32_t *>(malloc(sizeof(uint32_t) * (keep ? keep : 1)));
        from = static_cast<uint32_t *>(malloc(sizeof(uint32_t) * slots));
        if (!live_c || !live_s || !from) throw std::bad_alloc();
      }
    } else {
      dirty.reserve(dels.size() + puts.size());
    }
  } catch (const std::bad_alloc &) {
    drop();
    return -ENOMEM;
  }
  void *staged = nullptr;
#ifndef XSKNF_ACL_HOST_ONLY
  xsknf_gpu::AclStage *stage = nullptr;
  if (acl->d_keys) {
    // (with counters a rebuild sends the new slots' old slots behind the table)
    const size_t bytes = rebuild ? (sizeof(AclKey) + sizeof(int32_t) + (acl->d_ctr ? sizeof(uint32_t) : 0)) * static_cast<size_t>(slots)
                                 : sizeof(xsknf_gpu::AclUpdateRec) * (dels.size() + puts.size());
    int rc = xsknf_gpu::acl_stage_acquire(acl, bytes, !rebuild, &stage, &staged);
    if (!rc && rebuild && acl->d_ctr) rc = xsknf_gpu::acl_counters_spare(acl);
    if (rc) {
      drop();
      return rc;
    }
  }
#else
  (void)stream;
#endif

  // Pass 2: the host table.  Nothing below can fail.
  for (const uint32_t s : dels) {
    const AclKey &k = acl->keys[s];
    const uint32_t probes = ((s - (xsknf_gpu::acl_hash(k.a, k.b, k.c, k.p) & mask)) & mask) + 1;
    --acl->probe_hist[probes];
    acl->keys[s] = kTombstone;
    acl->actions[s] = 0;
    if (acl->ctr) acl->ctr[s] = AclCounter{0, 0};
    if (!rebuild) dirty.push_back(acl->ctr ? s | xsknf_gpu::kAclRecZero : s);   // (reserved above)
  }
  acl->rules -= static_cast<uint32_t>(dels.size());
  acl->tombstones += static_cast<uint32_t>(dels.size());
  while (acl->max_probe && !acl->probe_hist[acl->max_probe]) --acl->max_probe;
  if (rebuild) {
    rebuild_in_place(acl, live_k, live_a, live_c, live_s, from);
    free(live_k);
    free(live_a);
    free(live_c);
    free(live_s);
  }
  for (const uint32_t i : puts) {
    const AclKey k = key_of(ops[i].rule);
    const Place at = place_of(acl, k);
    if (!at.found) {
      if (acl->keys[at.slot].p == kAclTombstoneP) --acl->tombstones;
      acl->keys[at.slot] = k;
      ++acl->rules;
      ++acl->probe_hist[at.probes];
      if (at.probes > acl->max_probe) acl->max_probe = at.probes;
    }
    acl->actions[at.slot] = ops[i].rule.action;
    // a key new to the map starts at 0/0 (its slot held no live key: the counters
    // there are 0 already, on the host), and so does one the call deleted first
    const bool fresh = acl->ctr && (!at.found || again[i]);
    if (fresh) {
      acl->ctr[at.slot] = AclCounter{0, 0};
      if (rebuild) from[at.slot] = kAclNone;
    }
    if (!rebuild) dirty.push_back(fresh ? at.slot | xsknf_gpu::kAclRecZero : at.slot);
  }

#ifndef XSKNF_ACL_HOST_ONLY
  // Pass 3: the device table, on the stream.
  if (!acl->d_keys) {
    free(from);
    return 0;
  }
  if (rebuild) {
    memcpy(staged, acl->keys, sizeof(AclKey) * slots);
    memcpy(static_cast<char *>(staged) + sizeof(AclKey) * slots, acl->actions, sizeof(int32_t) * slots);
    if (from) memcpy(static_cast<char *>(staged) + (sizeof(AclKey) + sizeof(int32_t)) * slots, from, sizeof(uint32_t) * slots);
    free(from);
    return xsknf_gpu::acl_enqueue_table(acl, stage, stream);
  }
  // a put may have taken a slot this call's delete left: each slot once, as it is
  // now.  (With counters an entry may carry kAclRecZero above its slot: ordered
  // by the slot alone, a slot's entries or-ed into one.)
  std::sort(dirty.begin(), dirty.end(), [](uint32_t x, uint32_t y) {
    return (x & xsknf_gpu::kAclRecSlotMask) < (y & xsknf_gpu::kAclRecSlotMask);
  });
  size_t nd = 0;
  for (size_t i = 0; i < dirty.size(); ++i) {
    if (nd && ((dirty[nd - 1] ^ dirty[i]) & xsknf_gpu::kAclRecSlotMask) == 0) dirty[nd - 1] |= dirty[i];
    else dirty[nd++] = dirty[i];
  }
  dirty.resize(nd);
  xsknf_gpu::AclUpdateRec *rec = static_cast<xsknf_gpu::AclUpdateRec *>(staged);
  for (size_t i = 0; i < dirty.size(); ++i) {
    const uint32_t s = dirty[i] & xsknf_gpu::kAclRecSlotMask;
    rec[i] = xsknf_gpu::AclUpdateRec{dirty[i], acl->keys[s], acl->actions[s]};
  }
  return xsknf_gpu::acl_enqueue_records(acl, stage, static_cast<uint32_t>(dirty.size()), stream);
#else
  (void)staged;
  free(from);
  return 0;
#endif
}

int xsknf_gpu_acl_dump(const struct xsknf_gpu_acl *acl, int which, struct xsknf_gpu_acl_rule *rules_out, uint32_t cap,
                       uint32_t *n_out) {
  if (!acl || !n_out || (cap && !rules_out)) return -EINVAL;
  if (which == XSKNF_GPU_ACL_HOST_TABLE) return dump_table(acl->keys, acl->actions, acl->slots, rules_out, cap, n_out);
  if (which != XSKNF_GPU_ACL_DEVICE_TABLE) return -EINVAL;
  if (!acl->d_keys) return -ENODEV;
#ifndef XSKNF_ACL_HOST_ONLY
  const size_t kb = sizeof(AclKey) * static_cast<size_t>(acl->slots), ab = sizeof(int32_t) * static_cast<size_t>(acl->slots);
  char *tmp = static_cast<char *>(malloc(kb + ab));
  if (!tmp) return -ENOMEM;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(tmp, acl->d_keys, kb + ab, hipMemcpyDeviceToHost);
  int rc;
  if (e == hipSuccess) {
    rc = dump_table(reinterpret_cast<AclKey *>(tmp), reinterpret_cast<int32_t *>(tmp + kb), acl->slots, rules_out, cap, n_out);
  } else {
    xsknf_gpu::set_error(e, "ACL dump");
    rc = -EIO;
  }
  free(tmp);
  return rc;
#else
  return -ENODEV;
#endif
}

int xsknf_gpu_acl_counters_enable(struct xsknf_gpu_acl *acl) {
  if (!acl) return -EINVAL;
  if (acl->ctr) return 0;
  // one allocation: the counters, then the totals
  void *h = calloc(1, sizeof(AclCounter) * static_cast<size_t>(acl->slots) + sizeof(uint64_t) * XSKNF_GPU_ACL_TOTALS);
  if (!h) return -ENOMEM;
#ifndef XSKNF_ACL_HOST_ONLY
  if (acl->d_keys) {
    const int rc = xsknf_gpu::acl_counters_device_enable(acl);
    if (rc) {
      free(h);
      return rc;
    }
  }
#endif
  acl->ctr = static_cast<AclCounter *>(h);
  acl->totals = reinterpret_cast<uint64_t *>(acl->ctr + acl->slots);
  return 0;
}

int xsknf_gpu_acl_counters_dump(const struct xsknf_gpu_acl *acl, int which, struct xsknf_gpu_acl_rule *rules_out,
                                struct xsknf_gpu_acl_counter *counters_out, uint32_t cap, uint32_t *n_out,
                                uint64_t *totals_out) {
  if (!acl || !acl->ctr || !n_out || (cap && (!rules_out || !counters_out))) return -EINVAL;
  if (which == XSKNF_GPU_ACL_HOST_TABLE) {
    const int rc = dump_table(acl->keys, acl->actions, acl->slots, rules_out, cap, n_out, acl->ctr, counters_out);
    if (totals_out && rc != -ENOMEM) memcpy(totals_out, acl->totals, sizeof(uint64_t) * XSKNF_GPU_ACL_TOTALS);
    return rc;
  }
  if (which != XSKNF_GPU_ACL_DEVICE_TABLE) return -EINVAL;
  if (!acl->d_keys) return -ENODEV;
#ifndef XSKNF_ACL_HOST_ONLY
  const size_t kb = sizeof(AclKey) * static_cast<size_t>(acl->slots), ab = sizeof(int32_t) * static_cast<size_t>(acl->slots);
  const size_t cb = sizeof(AclCounter) * static_cast<size_t>(acl->slots);
  char *tmp = static_cast<char *>(malloc(cb + kb + ab));   // (the counters first: 8-byte aligned)
  if (!tmp) return -ENOMEM;
  uint64_t tot[XSKNF_GPU_ACL_TOTALS];
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(tmp, acl->d_ctr, cb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(tmp + cb, acl->d_keys, kb + ab, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(tot, acl->d_totals, sizeof(tot), hipMemcpyDeviceToHost);
  int rc;
  if (e == hipSuccess) {
    rc = dump_table(reinterpret_cast<AclKey *>(tmp + cb), reinterpret_cast<int32_t *>(tmp + cb + kb), acl->slots, rules_out,
                    cap, n_out, reinterpret_cast<AclCounter *>(tmp), counters_out);
    if (totals_out && rc != -ENOMEM) memcpy(totals_out, tot, sizeof(tot));
  } else {
    xsknf_gpu::set_error(e, "ACL counters dump");
    rc = -EIO;
  }
  free(tmp);
  return rc;
#else
  return -ENODEV;
#endif
}

int xsknf_gpu_acl_counters_clear(struct xsknf_gpu_acl *acl, int which, void *stream) {
  if (!acl || !acl->ctr) return -EINVAL;
  if (which == XSKNF_GPU_ACL_HOST_TABLE) {
    memset(acl->ctr, 0, sizeof(AclCounter) * static_cast<size_t>(acl->slots) + sizeof(uint64_t) * XSKNF_GPU_ACL_TOTALS);
    return 0;
  }
  if (which != XSKNF_GPU_ACL_DEVICE_TABLE) return -EINVAL;
  if (!acl->d_keys) return -ENODEV;
#ifndef XSKNF_ACL_HOST_ONLY
  return xsknf_gpu::acl_counters_device_clear(acl, stream);
#else
  (void)stream;
  return -ENODEV;
#endif
}

}  // extern "C"
