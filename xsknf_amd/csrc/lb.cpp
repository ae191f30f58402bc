// lb.cpp -- the load balancer's object (include/xsknf_gpu.h xsknf_gpu_lb_create,
// _info, _destroy, _sessions_put, _sessions_dump): the service and backend
// tables of lb_table.h built on one host thread, and the two session tables;
// and the removal of sessions (_sessions_remove, _drain_backend, _sessions_clear):
// the host table's here, the device table's checked here and handed to
// lb_remove_device.hip; and the services and backends of a live object
// (_backends_update, _backends_dump) and the list drain (_drain_backends): the
// ordered list is edited and the tables rebuilt here, what changed goes to
// lb_backends_device.hip; and ageing (_aging_enable, _clock, _sessions_expire,
// _sessions_ages): the stamps' allocation and the host table's expiry here, the
// device table's in lb_remove_device.hip.
// Plain C++; the only GPU calls are the allocation, the uploads, the table's
// copies for _sessions_put and _sessions_dump and the release, and a build with
// XSKNF_LB_HOST_ONLY has none (the sanitizer programs, tests/c/san_lb.c and
// san_lb_remove.c, link this file and lb_host.cpp alone).
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <unordered_map>
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

// The record list the object stands for: the services in the order they came to
// be (a service that lost its last backend and returns comes last), each with
// its backends by number.  The order of the services shows in the layout of
// svc and bk alone, never in a result.
struct xsknf_gpu_lb_list {
  struct Svc {
    uint32_t vaddr, vp;
    std::vector<xsknf_gpu::lb::Backend> bk;
  };
  std::vector<Svc> svcs;
};

namespace {

using namespace xsknf_gpu::lb;

void free_lb(xsknf_gpu_lb *lb) {
  free(lb->svc);
  free(lb->bk);
  delete lb->list;
  free(lb->keys);
  free(lb->vals);
  free(lb->live_k);
  free(lb->live_v);
  free(lb->stamps);
  free(lb->live_s);
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

// the host session table as a batch, _sessions_put and the removals see it
Tables host_tables(xsknf_gpu_lb *lb) {
  return Tables{lb->svc,       lb->bk,    lb->keys,         lb->vals,   &lb->count,
                lb->svc_slots, lb->slots, lb->max_sessions, lb->stamps, &lb->clock};
}

// the sessions of a table, ascending by key; with `ao` (xsknf_gpu_lb_sessions_ages)
// each one's clock - stamp in place of its value
int dump_table(const Key *keys, const Val *vals, uint32_t slots, xsknf_gpu_lb_session_key *ko,
               xsknf_gpu_lb_session_value *vo, uint32_t cap, uint32_t *n_out, const uint32_t *stamps = nullptr,
               uint32_t clock = 0, uint32_t *ao = nullptr) {
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
    xsknf_gpu_lb_session_key kk;
    memset(&kk, 0, sizeof(kk));
    kk.saddr = k.a;
    kk.daddr = k.b;
    kk.sport = static_cast<uint16_t>(k.c);
    kk.dport = static_cast<uint16_t>(k.c >> 16);
    kk.proto = static_cast<uint8_t>(k.p);
    ko[i] = kk;
    if (ao) {
      ao[i] = clock - stamps[used[i]];
      continue;
    }
    const Val &v = vals[used[i]];
    xsknf_gpu_lb_session_value vv;
    memset(&vv, 0, sizeof(vv));
    vv.addr = v.addr;
    vv.port = static_cast<uint16_t>(v.pi);
    vv.ifindex = static_cast<uint16_t>(v.pi >> 16);
    for (int b = 0; b < 4; ++b) vv.mac[b] = static_cast<uint8_t>(v.m0 >> (8 * b));
    vv.mac[4] = static_cast<uint8_t>(v.m1);
    vv.mac[5] = static_cast<uint8_t>(v.m1 >> 8);
    vv.dir = static_cast<uint8_t>(v.m1 >> 16);
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
// With ageing the stamps have their room too (_aging_enable adds it where the
// scratch already exists).
int want_scratch(xsknf_gpu_lb *lb) {
  if (lb->live_k) return 0;
  const size_t room = lb->max_sessions ? lb->max_sessions : 1;
  Key *k = static_cast<Key *>(malloc(sizeof(Key) * room));
  Val *v = static_cast<Val *>(malloc(sizeof(Val) * room));
  uint32_t *st = lb->stamps ? static_cast<uint32_t *>(malloc(sizeof(uint32_t) * room)) : nullptr;
  if (!k || !v || (lb->stamps && !st)) {
    free(k);
    free(v);
    free(st);
    return -ENOMEM;
  }
  lb->live_k = k;
  lb->live_v = v;
  lb->live_s = st;
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
      if (lb->stamps) lb->live_s[n] = lb->stamps[s];   // a session's stamp moves with it
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
    if (lb->stamps) lb->stamps[s] = lb->live_s[i];
  }
  lb->tombstones = 0;
  return 1;
}

void report(uint64_t *result, uint64_t removed, uint64_t compacted) {
  if (!result) return;
  result[XSKNF_GPU_LB_REMOVED] = removed;
  result[XSKNF_GPU_LB_COMPACTED] = compacted;
}

// ---- the services and backends ------------------------------------------------------
inline uint32_t vp_of(const xsknf_gpu_lb_backend &r) {
  return static_cast<uint32_t>(r.vport) | static_cast<uint32_t>(r.proto) << 16;
}
inline uint64_t svc_id(uint32_t vaddr, uint32_t vp) { return static_cast<uint64_t>(vaddr) << 32 | vp; }
inline Backend backend_of_record(const xsknf_gpu_lb_backend &r) {
  return Backend{r.addr, static_cast<uint32_t>(r.port) | static_cast<uint32_t>(r.ifindex) << 16, mac_lo(r.mac),
                 mac_hi(r.mac)};
}
inline uint32_t total_of(const xsknf_gpu_lb_list &l) {
  size_t t = 0;
  for (const auto &s : l.svcs) t += s.bk.size();
  return static_cast<uint32_t>(t);   // (the callers have bounded it)
}

// The two tables of a list (at most half of svc_slots services): every service,
// in the list's order, into the first empty slot from its home, its backends
// behind those of the services before it.  Nothing else decides the layout, so
// an object made from a list and one edited into it hold the same tables.
bool build_tables(const xsknf_gpu_lb_list &l, uint32_t svc_slots, Service **svc_out, Backend **bk_out) {
  const uint32_t total = total_of(l);
  Service *svc = static_cast<Service *>(calloc(svc_slots, sizeof(Service)));
  Backend *bk = static_cast<Backend *>(calloc(total ? total : 1, sizeof(Backend)));
  if (!svc || !bk) {
    free(svc);
    free(bk);
    return false;
  }
  const uint32_t mask = svc_slots - 1;
  uint32_t first = 0;
  for (const auto &e : l.svcs) {
    uint32_t s = xsknf_gpu::acl_hash(e.vaddr, e.vp, 0, 0) & mask;
    while (svc[s].count) s = (s + 1) & mask;
    const uint32_t count = static_cast<uint32_t>(e.bk.size());
    svc[s] = Service{e.vaddr, e.vp, first, count};
    memcpy(bk + first, e.bk.data(), sizeof(Backend) * count);
    first += count;
  }
  *svc_out = svc;
  *bk_out = bk;
  return true;
}

// The records of a pair of tables, ascending by service, a service's by number.
int dump_services(const Service *svc, uint32_t svc_slots, const Backend *bk, uint32_t total,
                  xsknf_gpu_lb_backend *out, uint32_t cap, uint32_t *n_out) {
  std::vector<Service> used;
  try {
    for (uint32_t s = 0; s < svc_slots; ++s)
      if (svc[s].count) used.push_back(svc[s]);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  std::sort(used.begin(), used.end(), [](const Service &x, const Service &y) {
    return x.vaddr != y.vaddr ? x.vaddr < y.vaddr : x.vp < y.vp;
  });
  uint64_t n = 0;
  for (const Service &e : used) {
    if (e.first > total || e.count > total - e.first) return -EIO;   // not a table of this object
    for (uint32_t k = 0; k < e.count; ++k, ++n) {
      if (n >= cap) continue;
      const Backend &b = bk[e.first + k];
      xsknf_gpu_lb_backend r;
      memset(&r, 0, sizeof(r));
      r.vaddr = e.vaddr;
      r.vport = static_cast<uint16_t>(e.vp);
      r.proto = static_cast<uint8_t>(e.vp >> 16);
      r.addr = b.addr;
      r.port = static_cast<uint16_t>(b.pi);
      r.ifindex = static_cast<uint16_t>(b.pi >> 16);
      for (int i = 0; i < 4; ++i) r.mac[i] = static_cast<uint8_t>(b.m0 >> (8 * i));
      r.mac[4] = static_cast<uint8_t>(b.m1);
      r.mac[5] = static_cast<uint8_t>(b.m1 >> 8);
      out[n] = r;
    }
  }
  *n_out = static_cast<uint32_t>(n);
  return n > cap ? -ENOSPC : 0;
}

// The ops on a copy of the list, in index order (the caller has validated them).
void edit_list(xsknf_gpu_lb_list &l, const xsknf_gpu_lb_backend_op *ops, uint32_t n) {
  std::unordered_map<uint64_t, uint32_t> at;
  for (uint32_t k = 0; k < l.svcs.size(); ++k) at.emplace(svc_id(l.svcs[k].vaddr, l.svcs[k].vp), k);
  for (uint32_t i = 0; i < n; ++i) {
    const xsknf_gpu_lb_backend &r = ops[i].backend;
    const uint32_t vp = vp_of(r);
    const auto it = at.find(svc_id(r.vaddr, vp));
    const auto is_it = [&r](const Backend &b) { return b.addr == r.addr && (b.pi & 0xffff) == r.port; };
    if (ops[i].op == XSKNF_GPU_LB_BACKEND_REMOVE) {
      if (it == at.end()) continue;
      auto &bk = l.svcs[it->second].bk;
      bk.erase(std::remove_if(bk.begin(), bk.end(), is_it), bk.end());
      if (bk.empty()) at.erase(it);   // the service is gone: an ADD makes a new one, last
      continue;
    }
    const Backend nb = backend_of_record(r);
    if (it == at.end()) {
      at.emplace(svc_id(r.vaddr, vp), static_cast<uint32_t>(l.svcs.size()));
      l.svcs.push_back(xsknf_gpu_lb_list::Svc{r.vaddr, vp, {nb}});
      continue;
    }
    auto &bk = l.svcs[it->second].bk;
    bool found = false;
    for (Backend &b : bk)
      if (is_it(b)) {
        b = nb;
        found = true;
      }
    if (!found) bk.push_back(nb);
  }
  l.svcs.erase(std::remove_if(l.svcs.begin(), l.svcs.end(), [](const xsknf_gpu_lb_list::Svc &s) { return s.bk.empty(); }),
               l.svcs.end());
}

// The listed backends as lb_table.h's set; duplicates fall together.
void id_set_of(const xsknf_gpu_lb_backend_id *list, uint32_t n, std::vector<IdSlot> &set) {
  uint32_t slots = 2;
  while (slots < 2 * n) slots *= 2;
  set.assign(slots, IdSlot{0, 0});
  for (uint32_t i = 0; i < n; ++i) {
    const IdSlot c = {list[i].addr, static_cast<uint32_t>(list[i].port) | static_cast<uint32_t>(list[i].proto) << 16};
    uint32_t s = xsknf_gpu::acl_hash(c.addr, c.pw, 0, 0) & (slots - 1);
    while (set[s].pw && !(set[s].addr == c.addr && set[s].pw == c.pw)) s = (s + 1) & (slots - 1);
    set[s] = c;
  }
}

int drain_list_args(const xsknf_gpu_lb *lb, const xsknf_gpu_lb_backend_id *list, uint32_t n) {
  if (!lb || (n && !list) || n > XSKNF_GPU_LB_MAX_BACKENDS) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i)
    if (list[i].proto != 6 && list[i].proto != 17) return -EINVAL;
  return 0;
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
  lb->keys = static_cast<Key *>(calloc(slots, sizeof(Key)));
  lb->vals = static_cast<Val *>(calloc(slots, sizeof(Val)));
  lb->list = new (std::nothrow) xsknf_gpu_lb_list();
  if (!lb->keys || !lb->vals || !lb->list) {
    free_lb(lb);
    return -ENOMEM;
  }
  // the services in the order they first appear, each with its records in order
  try {
    std::unordered_map<uint64_t, uint32_t> at;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t vp = vp_of(backends[i]);
      const auto it = at.find(svc_id(backends[i].vaddr, vp));
      uint32_t k;
      if (it != at.end()) {
        k = it->second;
      } else {
        if (lb->list->svcs.size() == XSKNF_GPU_LB_MAX_SERVICES) {
          free_lb(lb);
          return -EINVAL;
        }
        k = static_cast<uint32_t>(lb->list->svcs.size());
        at.emplace(svc_id(backends[i].vaddr, vp), k);
        lb->list->svcs.push_back(xsknf_gpu_lb_list::Svc{backends[i].vaddr, vp, {}});
      }
      lb->list->svcs[k].bk.push_back(backend_of_record(backends[i]));
    }
  } catch (const std::bad_alloc &) {
    free_lb(lb);
    return -ENOMEM;
  }
  if (!build_tables(*lb->list, lb->svc_slots, &lb->svc, &lb->bk)) {
    free_lb(lb);
    return -ENOMEM;
  }
  lb->services = static_cast<uint32_t>(lb->list->svcs.size());
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
  lb->d_base = d;
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
    rc = xsknf_gpu::lb_backends_release(lb);
    const int rrc = xsknf_gpu::lb_remove_release(lb);
    if (rrc) rc = rrc;
    hipError_t e = hipFree(lb->d_base);
    if (e != hipSuccess) rc = hip_rc(e, "load balancer release");
    e = lb->d_stamps ? hipFree(lb->d_stamps) : hipSuccess;
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
  int rc = put_all(host_tables(lb), keys, values, n);
#ifndef XSKNF_LB_HOST_ONLY
  if (lb->d_svc) {
    // the device table through a host copy: the same insert, the same order; with
    // ageing its stamps and its clock word (d_stamps' allocation) make the same trip
    const size_t kb = sizeof(Key) * static_cast<size_t>(lb->slots), vb = sizeof(Val) * static_cast<size_t>(lb->slots);
    const size_t sb = lb->d_stamps ? sizeof(uint32_t) * (static_cast<size_t>(lb->slots) + 1) : 0;
    char *tmp = static_cast<char *>(malloc(kb + vb + 16 + sb));
    if (!tmp) return -ENOMEM;
    uint32_t *st = sb ? reinterpret_cast<uint32_t *>(tmp + kb + vb + 16) : nullptr;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(tmp, lb->d_keys, kb + vb + 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sb) e = hipMemcpy(st, lb->d_stamps, sb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
      const int drc = put_all(Tables{lb->svc, lb->bk, reinterpret_cast<Key *>(tmp), reinterpret_cast<Val *>(tmp + kb),
                                     reinterpret_cast<uint32_t *>(tmp + kb + vb), lb->svc_slots, lb->slots,
                                     lb->max_sessions, st, st ? st + lb->slots : nullptr},
                              keys, values, n);
      if (!rc) rc = drc;
      e = hipMemcpy(lb->d_keys, tmp, kb + vb + 16, hipMemcpyHostToDevice);
      if (e == hipSuccess && sb) e = hipMemcpy(lb->d_stamps, st, sb - sizeof(uint32_t), hipMemcpyHostToDevice);
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

int xsknf_gpu_lb_backends_update(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_backend_op *ops, uint32_t n,
                                 void *stream) {
  if (!lb || (n && !ops)) return -EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (ops[i].op != XSKNF_GPU_LB_BACKEND_ADD && ops[i].op != XSKNF_GPU_LB_BACKEND_REMOVE) return -EINVAL;
    if (ops[i].backend.proto != 6 && ops[i].backend.proto != 17) return -EINVAL;
  }
  if (n == 0) return 0;
  // Everything that can fail for want of room or memory happens on copies; the
  // object changes only behind the line "commit".
  std::unique_ptr<xsknf_gpu_lb_list> work;
  Service *svc = nullptr;
  Backend *bk = nullptr;
  uint32_t total = 0;
  try {
    work.reset(new xsknf_gpu_lb_list(*lb->list));
    edit_list(*work, ops, n);
    size_t t = 0;
    for (const auto &s : work->svcs) t += s.bk.size();
    if (t > XSKNF_GPU_LB_MAX_BACKENDS || work->svcs.size() > XSKNF_GPU_LB_MAX_SERVICES) return -ENOSPC;
    total = static_cast<uint32_t>(t);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  if (!build_tables(*work, lb->svc_slots, &svc, &bk)) return -ENOMEM;
#ifndef XSKNF_LB_HOST_ONLY
  xsknf_gpu::LbStage *stage = nullptr;
  uint32_t entries = 0;
  if (lb->d_svc) {
    // What the device copy lacks: the slots and entries that differ from the
    // host copy it mirrors -- or everything, where it has to move to the region
    // of the first update, or where the entries would be no shorter (32 bytes
    // each against 16 of the table).
    const bool first = static_cast<void *>(lb->d_svc) != lb->d_region || !lb->d_region;
    const uint32_t all = lb->svc_slots + total;
    uint32_t changed = 0;
    for (uint32_t s = 0; s < lb->svc_slots; ++s) changed += memcmp(&svc[s], &lb->svc[s], sizeof(Service)) != 0;
    for (uint32_t i = 0; i < total; ++i)
      changed += i >= lb->backends || memcmp(&bk[i], &lb->bk[i], sizeof(Backend)) != 0;
    const bool whole = first || 2 * static_cast<uint64_t>(changed) >= all;
    if (whole || changed) {
      void *host = nullptr;
      const size_t bytes = whole ? sizeof(Backend) * static_cast<size_t>(all) : sizeof(xsknf_gpu::LbEntry) * changed;
      const int rc = xsknf_gpu::lb_backends_prepare(lb, bytes, &stage, &host);
      if (rc) {
        free(svc);
        free(bk);
        return rc;
      }
      if (whole) {
        memcpy(host, svc, sizeof(Service) * lb->svc_slots);
        memcpy(static_cast<char *>(host) + sizeof(Service) * lb->svc_slots, bk, sizeof(Backend) * total);
      } else {
        xsknf_gpu::LbEntry *e = static_cast<xsknf_gpu::LbEntry *>(host);
        for (uint32_t s = 0; s < lb->svc_slots; ++s)
          if (memcmp(&svc[s], &lb->svc[s], sizeof(Service))) {
            *e = xsknf_gpu::LbEntry{s, {0, 0, 0}, {svc[s].vaddr, svc[s].vp, svc[s].first, svc[s].count}};
            ++e;
          }
        for (uint32_t i = 0; i < total; ++i)
          if (i >= lb->backends || memcmp(&bk[i], &lb->bk[i], sizeof(Backend))) {
            *e = xsknf_gpu::LbEntry{lb->svc_slots + i, {0, 0, 0}, {bk[i].addr, bk[i].pi, bk[i].m0, bk[i].m1}};
            ++e;
          }
        entries = changed;
      }
    }
  }
#endif
  // commit
  free(lb->svc);
  free(lb->bk);
  delete lb->list;
  lb->svc = svc;
  lb->bk = bk;
  lb->list = work.release();
  lb->services = static_cast<uint32_t>(lb->list->svcs.size());
  lb->backends = total;
#ifndef XSKNF_LB_HOST_ONLY
  if (stage) return xsknf_gpu::lb_backends_enqueue(lb, stage, entries, stream);
#else
  (void)stream;
#endif
  return 0;
}

int xsknf_gpu_lb_backends_dump(const struct xsknf_gpu_lb *lb, int which, struct xsknf_gpu_lb_backend *records,
                               uint32_t cap, uint32_t *n_out) {
  if (!lb || !n_out || (cap && !records)) return -EINVAL;
  if (which == XSKNF_GPU_LB_HOST_TABLE)
    return dump_services(lb->svc, lb->svc_slots, lb->bk, lb->backends, records, cap, n_out);
  if (which != XSKNF_GPU_LB_DEVICE_TABLE) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  const size_t sb = sizeof(Service) * lb->svc_slots, bb = sizeof(Backend) * static_cast<size_t>(lb->backends);
  char *tmp = static_cast<char *>(malloc(sb + bb + 1));
  if (!tmp) return -ENOMEM;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(tmp, lb->d_svc, sb, hipMemcpyDeviceToHost);
  if (e == hipSuccess && bb) e = hipMemcpy(tmp + sb, lb->d_bk, bb, hipMemcpyDeviceToHost);
  const int rc = e == hipSuccess ? dump_services(reinterpret_cast<Service *>(tmp), lb->svc_slots,
                                                 reinterpret_cast<Backend *>(tmp + sb), lb->backends, records, cap, n_out)
                                 : hip_rc(e, "load balancer backends_dump");
  free(tmp);
  return rc;
#else
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_drain_backends_host(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_backend_id *list, uint32_t n,
                                     uint64_t *result) {
  int rc = drain_list_args(lb, list, n);
  if (rc) return rc;
  report(result, 0, 0);
  if (n == 0) return 0;
  std::vector<IdSlot> set;
  try {
    id_set_of(list, n, set);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  rc = want_scratch(lb);
  if (rc) return rc;
  uint64_t removed = 0;
  for (uint32_t s = 0; s < lb->slots; ++s)
    if (live(lb->keys[s]) && id_listed(set.data(), static_cast<uint32_t>(set.size()), drain_candidate(lb->keys[s], lb->vals[s]))) {
      bury(lb, s);
      ++removed;
    }
  report(result, removed, settle(lb));
  return 0;
}

int xsknf_gpu_lb_drain_backends(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_backend_id *list, uint32_t n,
                                uint64_t *result_dev, void *stream) {
  const int rc = drain_list_args(lb, list, n);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(result_dev) & 7) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  std::vector<IdSlot> set;
  try {
    if (n) id_set_of(list, n, set);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  return xsknf_gpu::lb_drain_list_enqueue(lb, set.data(), static_cast<uint32_t>(set.size()), result_dev, stream);
#else
  (void)stream;
  return -ENODEV;
#endif
}

// ---- ageing ---------------------------------------------------------------------------
int xsknf_gpu_lb_aging_enable(struct xsknf_gpu_lb *lb) {
  if (!lb) return -EINVAL;
  if (lb->stamps) return 0;
  // Everything is allocated before the object changes.  calloc's zeros are the
  // stamps: every session already stored carries its table's clock, 0.
  uint32_t *st = static_cast<uint32_t *>(calloc(lb->slots, sizeof(uint32_t)));
  uint32_t *ls = lb->live_k ? static_cast<uint32_t *>(malloc(sizeof(uint32_t) * (lb->max_sessions ? lb->max_sessions : 1)))
                            : nullptr;
  if (!st || (lb->live_k && !ls)) {
    free(st);
    free(ls);
    return -ENOMEM;
  }
#ifndef XSKNF_LB_HOST_ONLY
  if (lb->d_svc) {
    // the stamps and, behind them, 16 bytes whose first word is the clock
    const size_t bytes = sizeof(uint32_t) * static_cast<size_t>(lb->slots) + 16;
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // (no batch is in flight: the caller's word; a removal may be)
    if (e == hipSuccess) e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      const int rc = hip_rc(e, "load balancer ageing");
      if (d) (void)hipFree(d);
      free(st);
      free(ls);
      return rc;
    }
    lb->d_stamps = static_cast<uint32_t *>(d);
    lb->d_clock = lb->d_stamps + lb->slots;
    lb->device_bytes += bytes;
    if (lb->d_spare) {
      const int rc = xsknf_gpu::lb_want_spare(lb);   // the spare table's stamps
      if (rc) {
        (void)hipFree(d);
        lb->d_stamps = lb->d_clock = nullptr;
        lb->device_bytes -= bytes;
        free(st);
        free(ls);
        return rc;
      }
    }
  }
#endif
  lb->stamps = st;
  lb->live_s = ls;
  lb->clock = 0;
  return 0;
}

int xsknf_gpu_lb_clock(struct xsknf_gpu_lb *lb, int which, uint32_t now, void *stream) {
  if (!lb || !lb->stamps || (which != XSKNF_GPU_LB_HOST_TABLE && which != XSKNF_GPU_LB_DEVICE_TABLE)) return -EINVAL;
  if (which == XSKNF_GPU_LB_HOST_TABLE) {
    lb->clock = now;
    return 0;
  }
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  // one 4-byte fill in stream order: nothing of the caller's is referenced later
  const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(lb->d_clock), static_cast<int>(now), 1,
                                         static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_rc(e, "load balancer clock");
  return 0;
#else
  (void)stream;
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_sessions_expire_host(struct xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result) {
  if (!lb || !lb->stamps) return -EINVAL;
  report(result, 0, 0);
  const int rc = want_scratch(lb);
  if (rc) return rc;
  // One pass in slot order gives the set semantics, as one launch does on the
  // device (kernel_lb_expire.h): nothing a decision reads -- the stamps, a slot's
  // key words a, b, c and its value -- changes here; only p does, to the
  // tombstone.  So a session can miss its partner only where the partner has
  // just been buried, which took both halves idle: this session's own verdict.
  uint64_t removed = 0;
  for (uint32_t s = 0; s < lb->slots; ++s) {
    const Key k = lb->keys[s];
    if (!live(k) || !idle(lb->clock, lb->stamps[s], max_idle)) continue;
    const Val v = lb->vals[s];
    const Key pk = partner_key(k, v);
    const uint32_t ps = find(lb->keys, lb->slots, pk);
    if (ps != kNone && is_partner(pk, lb->vals[ps], k, v) && !idle(lb->clock, lb->stamps[ps], max_idle)) continue;
    bury(lb, s);
    ++removed;
  }
  report(result, removed, settle(lb));
  return 0;
}

int xsknf_gpu_lb_sessions_expire(struct xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result_dev, void *stream) {
  if (!lb || !lb->stamps || (reinterpret_cast<uintptr_t>(result_dev) & 7)) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  return xsknf_gpu::lb_expire_enqueue(lb, max_idle, result_dev, stream);
#else
  (void)max_idle, (void)stream;
  return -ENODEV;
#endif
}

int xsknf_gpu_lb_sessions_ages(const struct xsknf_gpu_lb *lb, int which, struct xsknf_gpu_lb_session_key *keys,
                               uint32_t *ages, uint32_t cap, uint32_t *n_out, uint32_t *clock_out) {
  if (!lb || !lb->stamps || !n_out || (cap && (!keys || !ages))) return -EINVAL;
  if (which == XSKNF_GPU_LB_HOST_TABLE) {
    if (clock_out) *clock_out = lb->clock;
    return dump_table(lb->keys, lb->vals, lb->slots, keys, nullptr, cap, n_out, lb->stamps, lb->clock, ages);
  }
  if (which != XSKNF_GPU_LB_DEVICE_TABLE) return -EINVAL;
  if (!lb->d_svc) return -ENODEV;
#ifndef XSKNF_LB_HOST_ONLY
  const size_t kb = sizeof(Key) * static_cast<size_t>(lb->slots);
  const size_t sb = sizeof(uint32_t) * (static_cast<size_t>(lb->slots) + 1);   // the stamps and the clock behind them
  char *tmp = static_cast<char *>(malloc(kb + sb));
  if (!tmp) return -ENOMEM;
  uint32_t *st = reinterpret_cast<uint32_t *>(tmp + kb);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(tmp, lb->d_keys, kb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(st, lb->d_stamps, sb, hipMemcpyDeviceToHost);
  int rc;
  if (e == hipSuccess) {
    if (clock_out) *clock_out = st[lb->slots];
    rc = dump_table(reinterpret_cast<Key *>(tmp), nullptr, lb->slots, keys, nullptr, cap, n_out, st, st[lb->slots], ages);
  } else {
    rc = hip_rc(e, "load balancer sessions_ages");
  }
  free(tmp);
  return rc;
#else
  return -ENODEV;
#endif
}

}  // extern "C"
