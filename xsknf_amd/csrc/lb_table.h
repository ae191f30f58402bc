// lb_table.h -- the load balancer's tables and per-frame arithmetic
// (include/xsknf_gpu.h, "the load balancer NF"), stated once for the builder
// (lb.cpp), the host model (lb_host.cpp) and the device kernels (kernel_lb.h):
// the slot layouts, the probes, the backend choice (jhash) and the reference's
// rewrite (examples/load_balancer/load_balancer_user.c:521-550) byte by byte.
// Plain C++17; no GPU call.
//
// All values are the frame's own bytes read as little-endian numbers, which is
// what the reference's struct fields hold on the little-endian hosts it runs on.
//
// The session table is open addressing with linear probing over a power-of-two
// number of slots, the ACL's layout and hash (acl_table.h): keys[s] is 16 bytes
//   a = saddr, b = daddr, c = sport | dport << 16, p = proto (0: empty slot)
// and vals[s], 16 bytes, belongs to it:
//   addr, pi = port | ifindex << 16, m0 = mac[0..3], m1 = mac[4..5] | dir << 16.
// A probe ends at the key or at the first empty slot, and the builder keeps
// slots >= 2 * max_sessions.
//
// Removal (xsknf_gpu_lb_sessions_remove, _drain_backend; lb.cpp on the host,
// kernel_lb_remove.h on the device) overwrites a slot's p with kTombstoneP, the
// ACL's tombstone, and leaves its other words: p is not 0, so find, put and the
// batch kernels walk on over it, and it is not 6 or 17, so no key equals it --
// none of them has a word about it.  put and the kernels' commit_one take empty
// slots only, so tombstones pile up until a removal leaves more than slots /
// kTombstoneShare of them; that removal rebuilds the table tombstone-free.
// Live sessions (<= max_sessions <= slots / 2) plus tombstones (<= slots / 4)
// thus never pass 3/4 of the slots: every probe sequence keeps an empty slot.
// The services are a table of the same kind, {vaddr, vport | proto << 16} ->
// {first, count}: the service's backends are bk[first .. first + count) in the
// order their records were given.  It has no tombstone: an update rebuilds it
// (lb.cpp), so a probe that ends at count == 0 has seen every service.
#pragma once
#include <stdint.h>

#include "acl_table.h"   // acl_hash, XSKNF_HD

namespace xsknf_gpu {
namespace lb {

constexpr uint32_t kToClient = 0, kToBackend = 1;   // enum direction, load_balancer.h:41-44
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kTombstoneP = kAclTombstoneP;   // p of a removed slot
constexpr uint32_t kTombstoneShare = 4;            // a removal that leaves more than slots / 4 tombstones rebuilds

struct Key {
  uint32_t a, b, c, p;
};
struct Val {
  uint32_t addr, pi, m0, m1;
};
struct Service {
  uint32_t vaddr, vp, first, count;   // count == 0: empty slot
};
struct Backend {
  uint32_t addr, pi, m0, m1;          // a forward session's Val less the direction
};
static_assert(sizeof(Key) == 16 && sizeof(Val) == 16 && sizeof(Service) == 16 && sizeof(Backend) == 16,
              "one 16-byte load per record");

XSKNF_HD inline bool same(const Key &x, const Key &y) {
  return x.a == y.a && x.b == y.b && x.c == y.c && x.p == y.p;
}
XSKNF_HD inline uint32_t key_hash(const Key &k) { return acl_hash(k.a, k.b, k.c, k.p); }

// The tables one batch works on (host pointers or device pointers).
struct Tables {
  const Service *svc;
  const Backend *bk;
  Key *keys;
  Val *vals;
  uint32_t *count;          // sessions stored
  uint32_t svc_slots, slots, max_sessions;
  // ageing (rule 11; xsknf_gpu_lb_aging_enable): one last-seen stamp per slot, a
  // side array, and the table's clock word.  stamps == nullptr: no ageing.
  uint32_t *stamps;
  const uint32_t *clock;
};
// Rule 11: slot s has been used, or stored into, at the table's clock.
XSKNF_HD inline void stamp(const Tables &t, uint32_t s) {
  if (t.stamps) t.stamps[s] = *t.clock;
}

// The slot that holds k, or kNone.
XSKNF_HD inline uint32_t find(const Key *keys, uint32_t slots, const Key &k) {
  const uint32_t mask = slots - 1;
  uint32_t s = key_hash(k) & mask;
  for (uint32_t i = 0; i < slots; ++i) {   // bounded whatever the table holds
    const Key t = keys[s];
    if (t.p == 0) return kNone;
    if (same(t, k)) return s;
    s = (s + 1) & mask;
  }
  return kNone;
}

// khashmap_update_elem on one thread: the value of a stored key is replaced; a
// new key is stored unless the table already holds max_sessions (-1).  Returns
// 1 for a new key, 0 for a replaced value.  With ageing either one stamps the
// slot (rule 11); a refused key stamps nothing.
XSKNF_HD inline int put(const Tables &t, const Key &k, const Val &v) {
  const uint32_t mask = t.slots - 1;
  uint32_t s = key_hash(k) & mask;
  for (uint32_t i = 0; i < t.slots; ++i) {
    const Key h = t.keys[s];
    if (h.p == 0) {
      if (*t.count >= t.max_sessions) return -1;
      t.keys[s] = k;
      t.vals[s] = v;
      ++*t.count;
      stamp(t, s);
      return 1;
    }
    if (same(h, k)) {
      t.vals[s] = v;
      stamp(t, s);
      return 0;
    }
    s = (s + 1) & mask;
  }
  return -1;
}

// ---- removal: what lb.cpp and kernel_lb_remove.h share ---------------------------
XSKNF_HD inline bool live(const Key &k) { return k.p != 0 && k.p != kTombstoneP; }
XSKNF_HD inline uint32_t dir_of(const Val &v) { return v.m1 >> 16 & 0xff; }
// The key of the other half of the flow that session {k -> v} belongs to: for a
// TO_BACKEND session {saddr, daddr, sport, dport} -> {addr, port} it is
// backward_key's {addr, saddr, port, sport}, for a TO_CLIENT one {daddr, addr,
// dport, port}.  k.p is the session's protocol (6 or 17), also where the slot
// itself has just been made a tombstone.
XSKNF_HD inline Key partner_key(const Key &k, const Val &v) {
  const uint32_t port = v.pi & 0xffff;
  if (dir_of(v) == kToBackend) return Key{v.addr, k.a, port | (k.c & 0xffff) << 16, k.p};
  return Key{k.b, v.addr, (k.c >> 16) | port << 16, k.p};
}
// Whether the stored session {pk -> pv} is the partner of {k -> v}, given that
// pk == partner_key(k, v): the opposite direction, and its own partner is k.
// An unpaired sessions_put entry, or a backward session that another flow has
// replaced, fails this and stays.
XSKNF_HD inline bool is_partner(const Key &pk, const Val &pv, const Key &k, const Val &v) {
  return dir_of(pv) != dir_of(v) && same(partner_key(pk, pv), k);
}
// drain_backend's predicate for one slot: both halves of every flow of backend
// {addr, port, proto} (proto is 6 or 17, so an empty slot and a tombstone fail).
XSKNF_HD inline bool drains(const Key &k, const Val &v, uint32_t addr, uint32_t port, uint32_t proto) {
  if (k.p != proto) return false;
  return dir_of(v) == kToBackend ? v.addr == addr && (v.pi & 0xffff) == port : k.a == addr && (k.c & 0xffff) == port;
}

// drain_backends' form of the same predicate.  A live slot names one backend,
// the one `drains` compares with: {addr, port | proto << 16}, the value's for a
// TO_BACKEND session, the key's source for a TO_CLIENT one.  The list is an
// open-addressing set of such pairs (lb.cpp builds it: a power of two, at most
// half full, linear probing from acl_hash(addr, pw, 0, 0); pw == 0 is an empty
// slot, which no backend's is: its proto is 6 or 17).
struct IdSlot {
  uint32_t addr, pw;
};
// xsknf_gpu_lb_sessions_expire's idle(k): unsigned, so a clock that has wrapped
// past a stamp still gives the ticks between them.
XSKNF_HD inline bool idle(uint32_t clock, uint32_t stamp_of, uint32_t max_idle) {
  return static_cast<uint32_t>(clock - stamp_of) > max_idle;
}
XSKNF_HD inline IdSlot drain_candidate(const Key &k, const Val &v) {
  return dir_of(v) == kToBackend ? IdSlot{v.addr, (v.pi & 0xffff) | k.p << 16} : IdSlot{k.a, (k.c & 0xffff) | k.p << 16};
}
XSKNF_HD inline bool id_listed(const IdSlot *set, uint32_t set_slots, const IdSlot &c) {
  const uint32_t mask = set_slots - 1;
  uint32_t s = acl_hash(c.addr, c.pw, 0, 0) & mask;
  for (uint32_t i = 0; i < set_slots; ++i) {   // bounded whatever the set holds
    const IdSlot e = set[s];
    if (e.pw == 0) return false;
    if (e.addr == c.addr && e.pw == c.pw) return true;
    s = (s + 1) & mask;
  }
  return false;
}

// The service {vaddr, vport, proto}, or NULL.
XSKNF_HD inline const Service *find_service(const Service *svc, uint32_t slots, uint32_t vaddr, uint32_t vp) {
  const uint32_t mask = slots - 1;
  uint32_t s = acl_hash(vaddr, vp, 0, 0) & mask;
  for (uint32_t i = 0; i < slots; ++i) {
    const Service *e = &svc[s];
    if (e->count == 0) return nullptr;
    if (e->vaddr == vaddr && e->vp == vp) return e;
    s = (s + 1) & mask;
  }
  return nullptr;
}

XSKNF_HD inline uint32_t rol(uint32_t w, uint32_t by) { return (w << by) | (w >> (32 - by)); }

// jhash(&sid, 13, 0) of the packed struct session_id: Bob Jenkins' lookup3 as
// the kernel shapes it.  The three lanes start at 0xdeadbeef + length +
// initval; the first twelve bytes enter as three little-endian words and are
// mixed; the thirteenth byte, the protocol, is added to the first lane; the
// final avalanche leaves the hash in the third.  The rotation counts are the
// algorithm: one differing bit picks another backend.
XSKNF_HD inline uint32_t session_jhash(const Key &k) {
  uint32_t x = 0xdeadbeefu + 13u, y = x, z = x;
  x += k.a;
  y += k.b;
  z += k.c;
  x -= z; x ^= rol(z, 4);  z += y;
  y -= x; y ^= rol(x, 6);  x += z;
  z -= y; z ^= rol(y, 8);  y += x;
  x -= z; x ^= rol(z, 16); z += y;
  y -= x; y ^= rol(x, 19); x += z;
  z -= y; z ^= rol(y, 4);  y += x;
  x += k.p & 0xff;
  z ^= y; z -= rol(y, 14);
  x ^= z; x -= rol(z, 11);
  y ^= x; y -= rol(x, 25);
  z ^= y; z -= rol(y, 16);
  x ^= z; x -= rol(z, 4);
  y ^= x; y -= rol(x, 14);
  z ^= y; z -= rol(y, 24);
  return z;
}

// The forward session of a flow: a function of its key and the service alone.
XSKNF_HD inline uint32_t backend_of(const Service &s, const Key &sid) { return s.first + session_jhash(sid) % s.count; }
XSKNF_HD inline Val forward_val(const Backend &b) { return Val{b.addr, b.pi, b.m0, b.m1 | kToBackend << 16}; }
// The backward session a new flow `sid` stores: its key and, with the frame's
// source MAC as two words and the batch's ingress interface, its value.
XSKNF_HD inline Key backward_key(const Backend &b, const Key &sid) {
  return Key{b.addr, sid.a, (b.pi & 0xffff) | (sid.c & 0xffff) << 16, sid.p};
}
XSKNF_HD inline Val backward_val(const Key &sid, uint32_t mac0, uint32_t mac1, uint32_t ingress) {
  return Val{sid.b, (sid.c >> 16) | (ingress & 0xffff) << 16, mac0, (mac1 & 0xffff) | kToClient << 16};
}

// load_balancer.h:54-70 -- the sum with end-around carry, and the TWO-fold
// csum_fold (the checksummer's restatement folds once: not interchangeable).
XSKNF_HD inline uint32_t csum_add(uint32_t csum, uint32_t addend) {
  csum += addend;
  return csum + (csum < addend);
}
XSKNF_HD inline uint32_t csum_fold(uint32_t csum) {
  csum = (csum & 0xffff) + (csum >> 16);
  csum = (csum & 0xffff) + (csum >> 16);
  return ~csum & 0xffff;
}
// The new value of a 16-bit check `check` (lines 539-542 with port == false,
// 545-550 with the ports).  ~check and ~old_port are complements AFTER the
// promotion to 32 bits: 0xffff0000 | the 16-bit complement.
XSKNF_HD inline uint32_t check_update(uint32_t check, uint32_t old_addr, uint32_t new_addr, bool port,
                                      uint32_t old_port, uint32_t new_port) {
  uint32_t csum = ~(check & 0xffff);
  csum = csum_add(csum, ~old_addr);
  csum = csum_add(csum, new_addr);
  if (port) {
    csum = csum_add(csum, ~(old_port & 0xffff));
    csum = csum_add(csum, new_port & 0xffff);
  }
  return csum_fold(csum);
}

XSKNF_HD inline uint32_t rd16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }
XSKNF_HD inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
XSKNF_HD inline void wr16(uint8_t *p, uint32_t v) {
  p[0] = static_cast<uint8_t>(v);
  p[1] = static_cast<uint8_t>(v >> 8);
}
XSKNF_HD inline void wr32(uint8_t *p, uint32_t v) {
  wr16(p, v);
  wr16(p + 2, v >> 16);
}

// What the parse decides about a frame of len bytes inside the UMEM.
enum Parse : int { kDrop = 0, kPass = 1, kCandidate = 2 };
XSKNF_HD inline int32_t pass_verdict(uint32_t ingress, uint32_t nif) {
  return nif > 1 ? static_cast<int32_t>((ingress + 1) % nif) : -1;
}
// The lbfw NF's PASS (examples/lbfw/lbfw_user.c:435, 476, 518): no -1 for one
// interface.  nif != 0 is the caller's to refuse.
XSKNF_HD inline int32_t lbfw_pass_verdict(uint32_t ingress, uint32_t nif) {
  return static_cast<int32_t>((ingress + 1) % nif);
}
// load_balancer_user.c:398-446 on bytes; for a candidate `next` and `proto` are set.
XSKNF_HD inline Parse parse(const uint8_t *f, uint32_t len, uint32_t &next, uint32_t &proto) {
  if (len < 14) return kDrop;
  if (f[12] != 0x08 || f[13] != 0x00) return kPass;
  if (len < 34) return kDrop;
  next = 14 + 4 * (f[14] & 15u);
  proto = f[23];
  if (proto != 6 && proto != 17) return kPass;
  if (next + (proto == 6 ? 20u : 8u) > len) return kDrop;
  return kCandidate;
}
XSKNF_HD inline Key session_key(const uint8_t *f, uint32_t next, uint32_t proto) {
  return Key{rd32(f + 26), rd32(f + 30), rd32(f + next), proto};
}

// Lines 521-550 in the reference's order, one byte at a time: for ihl < 5 the
// ports and the L4 check lie inside the IP header, and what a later line reads
// is what an earlier line wrote.  Returns the verdict.
XSKNF_HD inline int32_t rewrite(uint8_t *f, uint32_t next, uint32_t proto, const Val &v) {
  const uint32_t new_port = v.pi & 0xffff;
  uint32_t old_addr, old_port;
  if ((v.m1 >> 16 & 0xff) == kToBackend) {
    old_addr = rd32(f + 30);
    wr32(f + 30, v.addr);
    old_port = rd16(f + next + 2);
    wr16(f + next + 2, new_port);
  } else {
    old_addr = rd32(f + 26);
    wr32(f + 26, v.addr);
    old_port = rd16(f + next);
    wr16(f + next, new_port);
  }
  for (int i = 0; i < 6; ++i) f[6 + i] = f[i];
  wr32(f, v.m0);
  wr16(f + 4, v.m1);
  wr16(f + 24, check_update(rd16(f + 24), old_addr, v.addr, false, 0, 0));
  uint8_t *l4 = f + next + (proto == 6 ? 16 : 6);
  wr16(l4, check_update(rd16(l4), old_addr, v.addr, true, old_port, new_port));
  return static_cast<int32_t>(v.pi >> 16);
}

// stats words (XSKNF_GPU_LB_STATS)
enum Stat : int { kFrames, kRewritten, kPassed, kDropped, kCreated, kFailed, kOrdered, kGated, kStats };

// The lbfw NF's gate (rule 6a): an ACL table (acl_table.h) on the host or the
// device.  keys == nullptr: no gate -- the load balancer, and lbfw with
// acl == NULL.
// counters / totals: the ACL's hit counters (include/xsknf_gpu.h
// xsknf_gpu_acl_counters_*), or NULL: no counting.
struct Gate {
  const AclKey *keys;
  const int32_t *actions;
  uint32_t slots;
  AclCounter *counters;
  unsigned long long *totals;
};

// One frame of the reference's loop against the tables, the inserts included;
// counts everything but kFrames and kOrdered.  One body for both NFs: the load
// balancer (load_balancer_user.c:396-553) gives its PASS and no gate, lbfw
// (examples/lbfw/lbfw_user.c:420-594) its own PASS and the ACL.  `pass` is the
// batch's PASS verdict, computed once by the caller.
template <typename Counter>
XSKNF_HD inline int32_t frame(const Tables &t, const Gate &gate, uint8_t *f, uint32_t len, uint32_t ingress,
                              int32_t pass, Counter *stats) {
  uint32_t next = 0, proto = 0;
  const Parse p = parse(f, len, next, proto);
  if (p == kDrop) {
    ++stats[kDropped];
    return -1;
  }
  if (p == kPass) {
    ++stats[kPassed];
    return pass;
  }
  const Key sid = session_key(f, next, proto);
  if (gate.keys) {   // rule 6a: the rule's action, 0 included; no byte and no session touched
    const uint32_t g = acl_find(gate.keys, gate.slots, sid.a, sid.b, sid.c, sid.p);
    if (g != kAclNone) {
      ++stats[kGated];
      if (gate.counters) {   // (the host model; on the device lb_propose<true> has counted the frame)
        ++gate.counters[g].packets;
        gate.counters[g].bytes += len;
        ++gate.totals[kAclHits];
      }
      return gate.actions[g];
    }
    if (gate.counters) ++gate.totals[kAclMisses];
  }
  Val rep;
  const uint32_t s = find(t.keys, t.slots, sid);
  if (s != kNone) {
    rep = t.vals[s];
    stamp(t, s);   // rule 11
  } else {
    const Service *svc = find_service(t.svc, t.svc_slots, sid.b, (sid.c >> 16) | proto << 16);
    if (!svc) {
      ++stats[kPassed];
      return pass;
    }
    const Backend b = t.bk[backend_of(*svc, sid)];
    rep = forward_val(b);
    const int fwd = put(t, sid, rep);
    if (fwd < 0) {
      ++stats[kFailed];   // the reference's goto UPDATE: the backward session is skipped
    } else {
      stats[kCreated] += static_cast<Counter>(fwd);
      const int bwd = put(t, backward_key(b, sid), backward_val(sid, rd32(f + 6), rd16(f + 10), ingress));
      if (bwd < 0) ++stats[kFailed];
      else stats[kCreated] += static_cast<Counter>(bwd);
    }
  }
  ++stats[kRewritten];
  return rewrite(f, next, proto, rep);
}

}  // namespace lb
}  // namespace xsknf_gpu

// The object behind struct xsknf_gpu_lb: the services and backends and a session
// table on the host and, unless built with XSKNF_LB_HOST_ONLY (the sanitizer
// programs, tests/c/san_lb.c), on the device current at creation.  The two
// session tables are independent: the host call works on one, the device call
// on the other.  The services and backends change through
// xsknf_gpu_lb_backends_update (lb.cpp): `list` is the ordered record list the
// object stands for, svc / bk are rebuilt from it by every update (the builder
// _create uses), and the device copy follows in stream order
// (lb_backends_device.hip).
struct xsknf_gpu_lb_list;              // lb.cpp: the services in the order they came to be, each with its backends
struct xsknf_gpu_lb {
  uint32_t slots, max_sessions, svc_slots, services, backends;
  xsknf_gpu::lb::Service *svc;         // svc_slots slots; replaced by an update
  xsknf_gpu::lb::Backend *bk;          // `backends` entries, service after service; replaced by an update
  xsknf_gpu_lb_list *list;
  xsknf_gpu::lb::Key *keys;
  xsknf_gpu::lb::Val *vals;
  uint32_t count;
  uint32_t tombstones;                 // host table: slots that hold kTombstoneP
  xsknf_gpu::lb::Key *live_k;          // host: room for max_sessions sessions while the table is rebuilt
  xsknf_gpu::lb::Val *live_v;          //   (NULL until the first host removal)
  // ageing (all NULL / 0 until xsknf_gpu_lb_aging_enable): the host table's
  // stamps, one per slot, its clock, and the stamps' room in a rebuild
  uint32_t *stamps;
  uint32_t clock;
  uint32_t *live_s;
  // device (all NULL in a host-only object): d_base is creation's one
  // allocation -- services, backends, keys, values, counters.  d_svc / d_bk
  // point into it until the first update, then into d_region
  void *d_base;
  xsknf_gpu::lb::Service *d_svc;
  xsknf_gpu::lb::Backend *d_bk;
  xsknf_gpu::lb::Key *d_keys;
  xsknf_gpu::lb::Val *d_vals;
  uint32_t *d_count;                   // d_count[1]: the device table's tombstones
  uint64_t device_bytes;
  // lb_backends_device.hip (NULL until the first update): svc_slots service
  // slots and XSKNF_GPU_LB_MAX_BACKENDS backends, one array of 16-byte entries
  void *d_region;
  // lb_remove_device.hip (NULL until the first device removal): the spare table
  // a compaction rebuilds into, keys then values; and the pinned buffers of the
  // calls in flight (removals, list drains, updates)
  xsknf_gpu::lb::Key *d_spare;
  struct xsknf_gpu_lb_staging *staging;
  // ageing on the device (NULL until _aging_enable): one allocation, `slots`
  // stamps and behind them the clock word; and the spare table's stamps (with
  // d_spare, once both ageing and a device removal have happened)
  uint32_t *d_stamps;
  uint32_t *d_clock;
  uint32_t *d_spare_stamps;
};

#ifndef XSKNF_LB_HOST_ONLY
// lb_remove_device.hip: the removals on the device table, enqueued on `stream`
// (lb.cpp has validated the arguments and the object has a device half).  All
// return 0, -ENOMEM or -EIO (xsknf_gpu_last_error()).
namespace xsknf_gpu {
int lb_remove_enqueue(xsknf_gpu_lb *lb, const void *keys, uint32_t n, bool pair, uint64_t *result_dev, void *stream);
int lb_drain_enqueue(xsknf_gpu_lb *lb, uint32_t addr, uint32_t port, uint32_t proto, uint64_t *result_dev, void *stream);
// The list drain: `set` is lb.cpp's open-addressing set of set_slots entries
// {addr, port | proto << 16} (a power of two, at most half full, second word 0:
// empty), host memory that is copied before the call returns.
int lb_drain_list_enqueue(xsknf_gpu_lb *lb, const void *set, uint32_t set_slots, uint64_t *result_dev, void *stream);
int lb_clear_enqueue(xsknf_gpu_lb *lb, void *stream);
// Ageing (the object has stamps): the expiry pass over the device table and the
// four compaction launches; the spare table with the stamps' part, where it is
// missing (_aging_enable calls it when a spare table already exists).
int lb_expire_enqueue(xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result_dev, void *stream);
int lb_want_spare(xsknf_gpu_lb *lb);
int lb_remove_release(xsknf_gpu_lb *lb);   // _destroy

// lb_backends_device.hip: an update's way to the device copy.  _prepare makes
// sure of the region and of a pinned buffer of `bytes` bytes (*host_out), and
// changes nothing else; after it lb.cpp fills the buffer and commits the host
// copy, and _enqueue cannot fail for want of memory.  entries > 0: the buffer
// holds that many LbEntry, scattered by one launch; entries == 0: it holds the
// table whole, svc_slots + lb->backends 16-byte entries, copied over the region.
struct LbStage;
struct LbEntry {
  uint32_t index, pad[3];   // below svc_slots: a service slot; from there: backend index - svc_slots
  uint32_t w[4];            // the Service or the Backend
};
int lb_backends_prepare(xsknf_gpu_lb *lb, size_t bytes, LbStage **stage_out, void **host_out);
int lb_backends_enqueue(xsknf_gpu_lb *lb, LbStage *stage, uint32_t entries, void *stream);
int lb_backends_release(xsknf_gpu_lb *lb);   // _destroy, before lb_remove_release
}  // namespace xsknf_gpu
#endif
