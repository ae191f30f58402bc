// lb.cpp -- the load balancer's object (include/xsknf_gpu.h xsknf_gpu_lb_create,
// _info, _destroy, _sessions_put, _sessions_dump): the service and backend
// tables of lb_table.h built on one host thread, and the two session tables;
// and the removal of sessions (_sessions_remove, _drain_backend, _sessions_clear):
// the host table's here, the device table's checked here and handed to
// lb_remove_device.hip.
// Plain C++; the only GPU calls are the allocation, the uploads, the table's
// copies for _sessions_put and _sessions_dump and the release, and a build with
// XSKNF_LB_HOST_ONLY has none (the sanitizer programs, tests/c/san_lb.c and
// san_lb_remove.c, link this file and lb_host.cpp alone).
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "lb_table.h"

#ifndef XSKNF_LB_HOST_ONLY
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>
namespace xsknf_gpu {
void set_error(hipError_t e, const char *where);   // checksummer.hip
}
#endif

namespace {

using namespace xsknf_gpu::lb;

void free_lb(xsknf_gpu_lb *lb) {
  free(lb->svc);
  free(lb->bk);
  free(lb->keys);
  free(lb->vals);
  free(lb->live_k);
  free(lb->live_v);
  delete lb;
}

inline uint32_t mac_lo(const uint8_t *m) { return rd32(m); }
inline uint32_t mac_hi(const uint8_t *m) { return rd16(m + 4); }

Key key_of(const xsknf_gpu_lb_session_key &k) {
  return Key{k.saddr, k.daddr, static_cast<uint32_t>(k.sport) | static_cast<uint32_t>(k.dport) << 16, k.proto};
}
Val val_of(const xsknf_gpu_lb_session_value &v) {
  return Val{v.addr, static_cast<uint32_t>(v.port) | static_cast<uint32_t>(v.ifindex) << 16, mac_lo(v.mac),
             mac_hi(v.mac) | static_cast<uint32_t>(v.dir) << 16};
}

// the sessions of a table, ascending by key
int dump_table(const Key *keys, const Val *vals, uint32_t slots, xsknf_gpu_lb_session_key *ko,
               xsknf_gpu_lb_session_value *vo, uint32_t cap, uint32_t *n_out) {
  std::vector<uint32_t> used;
  try {
    for (uint32_t s = 0; s < slots; ++s)
      if (live(keys[s])) used.push_back(s);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  std::sort(used.begin(), used.end(), [keys](uint32_t x, uint32_t y) {
    const Key &a = keys[x], &b = keys[y];
    if (a.a != b.a) return a.a < b.a;
    if (a.b != b.b) return a.b < b.b;
    if (a.c != b.c) return a.c < b.c;
    return a.p < b.p;
  });
  *n_out = static_cast<uint32_t>(used.size());
  for (uint32_t i = 0; i < used.size() && i < cap; ++i) {
    const Key &k = keys[used[i]];
    const Val &v = vals[used[i]];
    xsknf_gpu_lb_session_key kk;
    xsknf_gpu_lb_session_value vv;
    memset(&kk, 0, sizeof(kk));
    memset(&vv, 0, sizeof(vv));
    kk.saddr = k.a;
    kk.daddr = k.b;
    kk.sport = static_cast<uint16_t>(k.c);
    kk.dport = static_cast<uint16_t>(k.c >> 16);
    kk.proto = static_cast<uint8_t>(k.p);
    vv.addr = v.addr;
    vv.port = static_cast<uint16_t>(v.pi);
    vv.ifindex = static_cast<uint16_t>(v.pi >> 16);
    for (int b = 0; b < 4; ++b) vv.mac[b] = static_cast<uint8_t>(v.m0 >> (8 * b));
    vv.mac[4] = static_cast<uint8_t>(v.m1);
    vv.mac[5] = static_cast<uint8_t>(v.m1 >> 8);
    vv.dir = static_cast<uint8_t>(v.m1 >> 16);
    ko[i] = kk;
    vo[i] = vv;
  }
  return used.size() > cap ? -ENOSPC : 0;
}

// n sessions into one table, in order; -ENOSPC at the first new key that does not fit
int put_all(const Tables &t, const xsknf_gpu_lb_session_key *keys, const xsknf_gpu_lb_session_value *values,
            uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (put(t, key_of(keys[i]), val_of(values[i])) < 0) return -ENOSPC;
  return 0;
}

// ---- removal from the host table --------------------------------------------------
// The same tombstones as on the device (lb_table.h), not a backward-shift
// delete: the two tables then agree on when a rebuild happens, so one model
// serves both, and a removal never moves a session that it does not remove.

constexpr uint32_t kRemoveFlags = XSKNF_GPU_LB_REMOVE_PAIR;

// The scratch of a rebuild, made by the first removal so that none can fail
// half way: count <= max_sessions always (put and the kernels refuse beyond it).
int want_scratch(xsknf_gpu_lb *lb) {
  if (lb->live_k) return 0;
  const size_t room = lb->max_sessions ? lb->max_sessions : 1;
  Key *k = static_cast<Key *>(malloc(sizeof(Key) * room));
  Val *v = static_cast<Val *>(malloc(sizeof(Val) * room));
  if (!k || !v) {
    free(k);
    free(v);
    return -ENOMEM;
  }
  lb->live_k = k;
  lb->live_v = v;
  return 0;
}

void bury(xsknf_gpu_lb *lb, uint32_t s) {
  lb->keys[s].p = kTombstoneP;
  --lb->count;
  ++lb->tombstones;
}

// After a removal: past the bound the live sessions are reinserted, in
// ascending slot order, into the emptied table.  Returns 1 if it rebuilt.
uint64_t settle(xsknf_gpu_lb *lb) {
  if (lb->tombstones <= lb->slots / kTombstoneShare) return 0;
  uint32_t n = 0;
  for (uint32_t s = 0; s < lb->slots; ++s)
    if (live(lb->keys[s])) {
      lb->live_k[n] = lb->keys[s];
      lb->live_v[n++] = lb->vals[s];
    }
  memset(lb->keys, 0, sizeof(Key) * lb->slots);
  memset(lb->vals, 0, sizeof(Val) * lb->slots);
  const uint32_t mask = lb->slots - 1;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t s = key_hash(lb->live_k[i]) & mask;
    while (lb->keys[s].p) s = (s + 1) & mask;   // (the keys are distinct and at most half the slots)
    lb->keys[s] = lb->live_k[i];
    lb->vals[s] = lb->live_v[i];
  }
  lb->tombstones = 0;
  return 1;
}

void report(uint64_t *result, uint64_t removed, uint64_t compacted) {
  if (!result) return;
  result[XSKNF_GPU_LB_REMOVED] = removed;
  result[XSKNF_GPU_LB_COMPACTED] = compacted;
}

#ifndef XSKNF_LB_HOST_ONLY
int hip_rc(hipError_t e, const char *where) {
  xsknf_gpu::set_error(e, where);
  return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}
#endif

}  // namespace

extern "C" {

int xsknf_gpu_lb_create(struct xsknf_gpu_lb **lb_out, const struct xsknf_gpu_lb_backend *backends, uint32_t n,
                        uint32_t max_sessions, uint32_t slots) {
  if (!lb_out || (n && !backends)) return -EINVAL;
  if (n > XSKNF_GPU_LB_MAX_BACKENDS || max_sessions > XSKNF_GPU_LB_MAX_SESSIONS) return -EINVAL;
  if (slots == 0) {
    slots = 64;
    while (slots < 2 * max_sessions) slots *= 2;
  } else if ((slots & (slots - 1)) || slots > XSKNF_GPU_LB_MAX_SLOTS || slots < 2 * max_sessions) {
    return -EINVAL;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (backends[i].proto != 6 && backends[i].proto != 17) return -EINVAL;
  xsknf_gpu_lb *lb = new (std::nothrow) xsknf_gpu_lb();
  if (!lb) return -ENOMEM;
  lb->slots = slots;
  lb->max_sessions = max_sessions;
  lb->svc_slots = 2 * XSKNF_GPU_LB_MAX_SERVICES;   // at most half full
  lb->backends = n;
  lb->svc = static_cast<Service *>(calloc(lb->svc_slots, sizeof(Service)));
  lb->bk = static_cast<Backend *>(calloc(n ? n : 1, sizeof(Backend)));
  lb->keys = static_cast<Key *>(calloc(slots, sizeof(Key)));
  lb->vals = static_cast<Val *>(calloc(slots, sizeof(Val)));
  uint32_t *order = static_cast<uint32_t *>(calloc(XSKNF_GPU_LB_MAX_SERVICES, sizeof(uint32_t)));
  if (!lb->svc || !lb->bk || !lb->keys || !lb->vals || !order) {
    free(order);
    free_lb(lb);
    return -ENOMEM;
  }
  // pass 1: the services in the order they first appear, with their backend counts
  const uint32_t smask = lb->svc_slots - 1;
  auto slot_of = [&](const xsknf_gpu_lb_backend &r, uint32_t vp) {
    uint32_t s = xsknf_gpu::acl_hash(r.vaddr, vp, 0, 0) & smask;
    while (lb->svc[s].count && !(lb->svc[s].vaddr == r.vaddr && lb->svc[s].vp == vp)) s = (s + 1) & smask;
    return s;
  };
  for (uint32_t i = 0; i < n; ++i) {
    const xsknf_gpu_lb_backend &r = backends[i];
    const uint32_t vp = static_cast<uint32_t>(r.vport) | static_cast<uint32_t>(r.proto) << 16;
    const uint32_t s = slot_of(r, vp);
    if (!lb->svc[s].count) {
      if (lb->services == XSKNF_GPU_LB_MAX_SERVICES) {
        free(order);
        free_lb(lb);
        return -EINVAL;
      }
      lb->svc[s].vaddr = r.vaddr;
      lb->svc[s].vp = vp;
      order[lb->services++] = s;
    }
    ++lb->svc[s].count;
  }
  // each service's first backend; then pass 2 places the records (count is
  // rebuilt as the fill level)
  uint32_t first = 0;
  for (uint32_t k = 0; k < lb->services; ++k) {
    Service &e = lb->svc[order[k]];
    e.first = first;
    first += e.count;
    e.count = 0;
  }
  free(order);
  for (uint32_t i = 0; i < n; ++i) {
    const xsknf_gpu_lb_backend &r = backends[i];
    const uint32_t vp = static_cast<uint32_t>(r.vport) | static_cast<uint32_t>(r.proto) << 16;
    // (probe by the key alone: every service is stored, and vp != 0 is no empty slot's)
    uint32_t s = xsknf_gpu::acl_hash(r.vaddr, vp, 0, 0) & smask;
    while (!(lb->svc[s].vaddr == r.vaddr && lb->svc[s].vp == vp)) s = (s + 1) & smask;
    Service &e = lb->svc[s];
    lb->bk[e.first + e.count++] = Backend{r.addr, static_cast<uint32_t>(r.port) | static_cast<uint32_t>(r.ifindex) << 16,
                                          mac_lo(r.mac), mac_hi(r.mac)};
  }
#ifndef XSKNF_LB_HOST_ONLY
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    // a process without a device: the object serves xsknf_gpu_lb_host alone
    (void)hipGetLastError();
    *lb_out = lb;
    return 0;
  }
  const size_t sb = sizeof(Service) * lb->svc_slots, bb = sizeof(Backend) * (n ? n : 1);
  const size_t kb = sizeof(Key) * static_cast<size_t>(slots), vb = sizeof(Val) * static_cast<size_t>(slots);
  const size_t total = sb + bb + kb + vb + 16;
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, total);
  char *p = static_cast<char *>(d);
  if (e == hipSuccess) e = hipMemcpy(p, lb->svc, sb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p + sb, lb->bk, bb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(p + sb + bb, 0, kb + vb + 16);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = hip_rc(e, "load balancer upload");
    if (d) (void)hipFree(d);
    free_lb(lb);
    return rc;
  }
  lb->d_svc = reinterpret_cast<Service *>(p);
  lb->d_bk = reinterpret_cast<Backend *>(p + sb);
  lb->d_keys = reinterpret_cast<Key *>(p + sb + bb);
  lb->d_vals = reinterpret_cast<Val *>(p + sb + bb + kb);
  lb->d_count = reinterpret_cast<uint32_t *>(p + sb + bb + kb + vb);
  lb->device_bytes = total;
#endif
  *lb_out = lb;
  return 0;
}

int xsknf_gpu_lb_info(const struct xsknf_gpu_lb *lb, struct xsknf_gpu_lb_info *info) {
  if (!lb || !info) return -EINVAL;
  memset(info, 0, sizeof(*info));
  info->services = lb->services;
  info->backends = lb->backends;
  info->max_sessions = lb->max_sessions;
  info->slots = lb->slots;
  info->host_sessions = lb->count;
  info->device_bytes = lb->device_bytes;
#ifndef XSKNF_LB_HOST_ONLY
  if (lb->d_svc) {
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&info->device_sessions, lb->d_count, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_rc(e, "load balancer info");
  }
#endif
  return 0;
}

int xsknf_gpu_lb_destroy(struct xsknf_gpu_lb *lb) {
  if (!lb) return -EINVAL;
  int rc = 0;
#ifndef XSKNF_LB_HOST_ONLY
  if (lb->d_svc) {
    rc = xsknf_gpu::lb_remove_release(lb);
    const hipError_t e = hipFree(lb->d_svc);
    if (e != hipSuccess) rc = hip_rc(e, "load balancer release");
  }
#endif
  free_lb(lb);
  return rc;
}

int xsknf_gpu_lb_sessions_remove_host(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_session_key *keys, uint32_t n,
                                      uint32_t flags, uint64_t *result) {
  if (!lb || (n && !keys) || (flags & ~kRemoveFlags)) return -EINVAL;
  report(result, 0, 0);
  if (n == 0) return 0;
  const int rc = want_scratch(lb);
  if (rc) return rc;
  // In list order.  This is the set semantics: what a key or a partner check
  // reads of a slot -- its key words and its value -- no removal changes, and a
  // slot is only ever buried by a listed key or by a partner that passed.
  uint64_t removed = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (keys[i].proto != 6 && keys[i].proto != 17) continue;
    const Key k = key_of(keys[i]);
    const uint32_t s = find(lb->keys, lb->slots, k);
    if (s == kNone) continue;
    const Val v = lb->vals[s];
    bury(lb, s);
    ++removed;
    if (!(flags & XSKNF_GPU_LB_REMOVE_PAIR)) continue;
    const Key pk = partner_key(k, v);
    const uint32_t ps = find(lb->keys, lb->slots, pk);
    if (ps != kNone && is_partner(pk, lb->vals[ps], k, v)) {
      bury(lb, ps);
      ++removed;
    }
  }
  report(result, removed, settle(lb));
  return 0;
}

int xsknf_gpu_lb_drain_backend_host(struct xsknf_gpu_lb *lb, uint32_t addr, uint16_t port, uint8_t proto,
                                    uint64_t *result) {
  if (!lb || (proto != 6 && proto != 17)) return -EINVAL;
  report(result, 0, 0);
  const int rc = want_scratch(lb);
  if (rc) return rc;
  uint64_t removed = 0;
  for (uint32_t s = 0; s < lb->slots; ++s)
    if (drains(lb->keys[s], lb->vals[s], addr, port, proto)) {
      bury(lb, s);
      ++removed;
    }
  report(result, removed, settle(lb));
  return 0;
}

int xsknf_gpu_lb_sessions_remove(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_session_key *keys, uint32_t n,
                                 uint32_t flags, uint64_t *result_dev, void *stream) {
  if (!lb || (n && !keys) || (flags & ~kRemoveFlags) || (reinterpret_cast<uintptr_t>(result_dev) & 7)) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  return xsknf_gpu::lb_remove_enqueue(lb, keys, n, (flags & XSKNF_GPU_LB_REMOVE_PAIR) != 0, result_dev, stream);
#else
  (void)stream;
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_drain_backend(struct xsknf_gpu_lb *lb, uint32_t addr, uint16_t port, uint8_t proto,
                               uint64_t *result_dev, void *stream) {
  if (!lb || (proto != 6 && proto != 17) || (reinterpret_cast<uintptr_t>(result_dev) & 7)) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  return xsknf_gpu::lb_drain_enqueue(lb, addr, port, proto, result_dev, stream);
#else
  (void)addr, (void)port, (void)stream;
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_sessions_clear(struct xsknf_gpu_lb *lb, int which, void *stream) {
  if (!lb || (which != XSKNF_GPU_LB_HOST_TABLE && which != XSKNF_GPU_LB_DEVICE_TABLE)) return -EINVAL;
  if (which == XSKNF_GPU_LB_HOST_TABLE) {
    memset(lb->keys, 0, sizeof(Key) * lb->slots);
    memset(lb->vals, 0, sizeof(Val) * lb->slots);
    lb->count = 0;
    lb->tombstones = 0;
    return 0;
  }
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  return xsknf_gpu::lb_clear_enqueue(lb, stream);
#else
  (void)stream;
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_sessions_put(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_session_key *keys,
                              const struct xsknf_gpu_lb_session_value *values, uint32_t n) {
  if (!lb || (n && (!keys || !values))) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (values[i].dir > 1) return -EINVAL;
    if (keys[i].proto != 6 && keys[i].proto != 17) return -EINVAL;
  }
  if (n == 0) return 0;
  int rc = put_all(Tables{lb->svc, lb->bk, lb->keys, lb->vals, &lb->count, lb->svc_slots, lb->slots, lb->max_sessions},
                   keys, values, n);
#ifndef XSKNF_LB_HOST_ONLY
  if (lb->d_svc) {
    // the device table through a host copy: the same insert, the same order
    const size_t kb = sizeof(Key) * static_cast<size_t>(lb->slots), vb = sizeof(Val) * static_cast<size_t>(lb->slots);
    char *tmp = static_cast<char *>(malloc(kb + vb + 16));
    if (!tmp) return -ENOMEM;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(tmp, lb->d_keys, kb + vb + 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
      const int drc = put_all(Tables{lb->svc, lb->bk, reinterpret_cast<Key *>(tmp), reinterpret_cast<Val *>(tmp + kb),
                                     reinterpret_cast<uint32_t *>(tmp + kb + vb), lb->svc_slots, lb->slots,
                                     lb->max_sessions},
                              keys, values, n);
      if (!rc) rc = drc;
      e = hipMemcpy(lb->d_keys, tmp, kb + vb + 16, hipMemcpyHostToDevice);
    }
    free(tmp);
    if (e != hipSuccess) return hip_rc(e, "load balancer sessions_put");
  }
#endif
  return rc;
}

int xsknf_gpu_lb_sessions_dump(const struct xsknf_gpu_lb *lb, int which, struct xsknf_gpu_lb_session_key *keys,
                               struct xsknf_gpu_lb_session_value *values, uint32_t cap, uint32_t *n_out) {
  if (!lb || !n_out || (cap && (!keys || !values))) return -EINVAL;
  if (which == XSKNF_GPU_LB_HOST_TABLE) return dump_table(lb->keys, lb->vals, lb->slots, keys, values, cap, n_out);
  if (which != XSKNF_GPU_LB_DEVICE_TABLE) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  const size_t kb = sizeof(Key) * static_cast<size_t>(lb->slots), vb = sizeof(Val) * static_cast<size_t>(lb->slots);
  char *tmp = static_cast<char *>(malloc(kb + vb));
  if (!tmp) return -ENOMEM;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(tmp, lb->d_keys, kb + vb, hipMemcpyDeviceToHost);
  int rc = e == hipSuccess ? dump_table(reinterpret_cast<Key *>(tmp), reinterpret_cast<Val *>(tmp + kb), lb->slots, keys,
                                        values, cap, n_out)
                           : hip_rc(e, "load balancer sessions_dump");
  free(tmp);
  return rc;
#else
  return -ENODEV;
#endif
}

}  // extern "C"
