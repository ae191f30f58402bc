// kernel_lb.h -- the load balancer's device kernels, and the lbfw NF's: the same
// four launches with the batch's own PASS value (Args::pass) and, in
// lb_propose<true>, the ACL gate.  Part of lb_device.hip's translation unit
// (none of checksummer.hip's).
//
// A batch must give exactly what the reference's loop gives, frame after frame
// against one table, without one thread doing the work.  Four launches, all
// enqueued every time; they decide from device memory what they do:
//
//   lb_propose  one lane per frame.  Parses; a frame the parse decides gets its
//               verdict and is done.  A candidate whose key is in the session
//               table (the state before the batch: nothing inserts here) is a
//               HIT.  A candidate that misses and hits a service proposes the
//               two keys the loop would store, forward S and backward B, into
//               the batch's staging table; any other candidate is a MISS.
//   lb_apply    one lane per frame, unless the batch stands down (below).  A
//               candidate takes its session from the session table (HIT) or
//               from staging if the key's creator -- the lowest frame index
//               that proposed it -- is not later than the frame; otherwise it
//               passes.  Then the rewrite and the verdict.
//   lb_commit   under the same condition every creator stores its keys in the
//               session table.  A launch of its own: no lookup ever sees a
//               half-written slot.
//   lb_ordered  one lane.  If the batch stood down it walks the loop over the
//               batch (lb_table.h frame(), the host model's code): exact and
//               SLOW, for the rare batches below.  Otherwise it only adds the
//               new keys to the session count.
//
// The batch stands down when the ordered flag is set or the new keys do not
// all fit (sessions + new_keys > max_sessions: the loop's failing inserts depend
// on its order).  lb_propose sets the flag when
//   - two proposers of one key differ in (sid, kind): two flows that store the
//     same backward key, or a forward key that is another flow's backward key
//     (a service address acting as a client), or
//   - a proposed B is already in the session table (the loop would replace a
//     session that earlier frames of the batch still use).
// These are the only ways the loop's result depends on more than "the lowest
// index creates": frames of one flow propose identical keys, S is absent from
// the table by construction, and a HIT's session can only change through a B.
//
// Staging: open addressing over a power of two >= 4 n words, zeroed per batch.
// A word is 0 (empty) or (frame + 1) << 1 | kind of the lowest frame that
// proposed the slot's key so far.  The key itself, the backend and the frame's
// source MAC lie in that frame's 48-byte proposal record, which its lane writes
// BEFORE it publishes the index: a slot is claimed by one compare-and-swap
// (acq_rel, agent scope) and lowered by fetch_min, so whoever reads an index
// can read that frame's record, and nobody ever waits for another lane.  All
// holders of a slot carry the same key.  The record's words are stored and
// loaded as relaxed agent-scope atomics: they cross CUs and XCDs within the
// launch.
//
// Stores into frames cover only bytes the rewrite changes, as byte stores or
// 2-byte stores at even addresses inside [off, off + len): in the packed layout
// a neighbour's last bytes share an aligned word with this frame's first, and
// another lane is rewriting them.  Reads are whole aligned words (ld_bytes).
// For ihl >= 5 the fields are disjoint and the new values are computed in
// registers; below, rewrite() of lb_table.h runs byte by byte in the
// reference's order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "desc_rules.h"
#include "kernel_acl_count.h"
#include "lb_table.h"
#include "ld_bytes.h"

namespace xsknf_gpu {
namespace lbk {

constexpr int kThreads = 256;       // frames per block and step: one lane per frame
constexpr int kMaxBlocks = 2048;    // 8 four-wave blocks on each of 256 CUs; the rest by grid stride

// workspace header words
enum Hdr : int { kOrderedFlag = 0, kNewKeys = 1, kHdrWords = 16 };
// state[f]: what lb_propose found; bits 31..30 the class, 29 TCP, 28..25 the ihl,
// 23..0 a HIT's session slot
constexpr uint32_t kDone = 0, kHit = 1u << 30, kProposer = 2u << 30, kMiss = 3u << 30, kClassMask = 3u << 30;
// a frame's proposal record: 12 words
enum Prop : int { kSa, kSb, kSc, kProto, kBa, kBb, kBc, kBackend, kMac0, kMac1, kSlotS, kSlotB, kPropWords };

struct Args {
  uint8_t *umem;
  uint64_t umem_size;
  const uint4 *descs;
  int32_t *verdicts;
  lb::Tables t;
  uint32_t *hdr;
  uint32_t *staging;
  uint32_t *state;
  uint32_t *prop;
  unsigned long long *stats;
  uint32_t n, ingress, stage_slots;
  int32_t pass;        // the batch's PASS verdict (the NF's own: lb_table.h), computed once on the host
  lb::Gate gate;       // lbfw's ACL on the device; read by lb_propose<true> alone
};

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t enc(uint32_t frame, uint32_t kind) { return (frame + 1) << 1 | kind; }

// The key of kind `kind` in frame j's proposal record.
__device__ __forceinline__ lb::Key prop_key(const uint32_t *prop, uint32_t j, uint32_t kind) {
  const uint32_t *r = prop + static_cast<uint64_t>(j) * kPropWords;
  const uint32_t *k = r + (kind ? kBa : kSa);
  return lb::Key{ld_agent(k), ld_agent(k + 1), ld_agent(k + 2), ld_agent(r + kProto)};
}

// Propose `key` (kind 0: forward, 1: backward) for frame f, whose own key is
// sid.  Returns the staging slot.
__device__ __forceinline__ uint32_t stage(const Args &a, const lb::Key &key, const lb::Key &sid, uint32_t f,
                                          uint32_t kind) {
  const uint32_t mask = a.stage_slots - 1, mine = enc(f, kind);
  uint32_t s = lb::key_hash(key) & mask;
  for (uint32_t i = 0; i < a.stage_slots; ++i) {   // at most 2 n keys in >= 4 n slots
    uint32_t cur = 0;
    if (__hip_atomic_compare_exchange_strong(&a.staging[s], &cur, mine, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
      __hip_atomic_fetch_add(&a.hdr[kNewKeys], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return s;
    }
    const uint32_t j = (cur >> 1) - 1, kj = cur & 1;
    if (lb::same(prop_key(a.prop, j, kj), key)) {
      if (kj != kind || !lb::same(prop_key(a.prop, j, 0), sid))
        __hip_atomic_fetch_or(&a.hdr[kOrderedFlag], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_min(&a.staging[s], mine, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      return s;
    }
    s = (s + 1) & mask;
  }
  return s;   // not reached: the table is never full
}

// The holder of `key` in staging after lb_propose (a plain read: an earlier
// launch wrote it), or 0.
__device__ __forceinline__ uint32_t staged(const Args &a, const lb::Key &key) {
  const uint32_t mask = a.stage_slots - 1;
  uint32_t s = lb::key_hash(key) & mask;
  for (uint32_t i = 0; i < a.stage_slots; ++i) {
    const uint32_t cur = a.staging[s];
    if (cur == 0) return 0;
    if (lb::same(prop_key(a.prop, (cur >> 1) - 1, cur & 1), key)) return cur;
    s = (s + 1) & mask;
  }
  return 0;
}

// Whether lb_apply and lb_commit run (the same words for every lane of the
// batch: only lb_ordered, the last launch, changes the count).
__device__ __forceinline__ bool parallel_path(const Args &a) {
  return a.hdr[kOrderedFlag] == 0 &&
         static_cast<uint64_t>(*a.t.count) + a.hdr[kNewKeys] <= static_cast<uint64_t>(a.t.max_sessions);
}

// per-block counters in LDS, added to the batch's stats by the block's first lanes
__device__ __forceinline__ void count(uint32_t *c, int which) { atomicAdd(&c[which], 1u); }
__device__ __forceinline__ void flush(const Args &a, uint32_t *c) {
  __syncthreads();
  if (threadIdx.x < lb::kStats && c[threadIdx.x])
    __hip_atomic_fetch_add(&a.stats[threadIdx.x], static_cast<unsigned long long>(c[threadIdx.x]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// kGate: the lbfw NF (rule 6a).  A candidate whose sid the ACL holds gets the
// rule's action as its verdict here and is kDone: no table is touched for it,
// nothing is proposed, and the later launches never see it.  The gate reads
// only the frame's own sid and the immutable ACL, so it needs no order.  The
// two probes run one after the other: a variant that issued the ACL's and the
// session table's home-slot loads together measured no faster.
// An ACL with hit counters (a.gate.counters) counts the frame here, at the one
// place a gated frame is decided -- the later launches, the ordered path among
// them, see it as kDone -- with the firewall's combine: the candidates of a
// wave are at the probe together, the lanes the parse decided have left for
// the loop's next trip and are in nobody's group.  The ACL's totals come from
// the block's own counts when it flushes: in this launch kPassed and kDropped
// are exactly the frames decided before the lookup.
// The load balancer's instantiation, kGate false, carries none of this.
template <bool kGate>
__global__ __launch_bounds__(kThreads) void lb_propose(const Args a) {
  __shared__ uint32_t c[lb::kStats];
  if (threadIdx.x < lb::kStats) c[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t f = blockIdx.x * kThreads + threadIdx.x; f < a.n; f += stride) {
    const uint4 d = a.descs[f];
    const uint64_t off = desc_offset(static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32);
    const uint32_t len = d.z;
    count(c, lb::kFrames);
    int32_t verdict = -1;
    bool pass = false, cand = false;
    uint32_t e = 0, proto = 0, sa = 0, da = 0, next = 0;
    if (in_umem(off, len, a.umem_size) && len >= 14) {                       // rules 0, 1
      if (len < 34) {                                                        // rules 2, 3
        pass = (ld_bytes(a.umem, off + 12, 2) & 0xffff) != 0x0008;
      } else {
        e = ld_bytes(a.umem, off + 12, 4);
        proto = ld_bytes(a.umem, off + 23, 1) & 0xff;
        sa = ld_bytes(a.umem, off + 26, 4);
        da = ld_bytes(a.umem, off + 30, 4);
        next = 14 + 4 * ((e >> 16) & 15);                                    // rule 4
        if ((e & 0xffff) != 0x0008) pass = true;                             // rule 2
        else if (proto != 6 && proto != 17) pass = true;                     // rule 5
        else cand = next + (proto == 6 ? 20u : 8u) <= len;
      }
    }
    if (!cand) {
      if (pass) verdict = a.pass;
      count(c, pass ? lb::kPassed : lb::kDropped);
      a.verdicts[f] = verdict;
      a.state[f] = kDone;
      continue;
    }
    const uint32_t shape = (proto == 6 ? 1u << 29 : 0u) | ((e >> 16) & 15) << 25;
    const lb::Key sid = {sa, da, ld_bytes(a.umem, off + next, 4), proto};    // rule 6
    if constexpr (kGate) {
      const uint32_t g = acl_find(a.gate.keys, a.gate.slots, sid.a, sid.b, sid.c, sid.p);
      if (a.gate.counters) acl_count::count_hits(a.gate.counters, g != kAclNone, g, len);
      if (g != kAclNone) {                                                   // rule 6a
        count(c, lb::kGated);
        a.verdicts[f] = a.gate.actions[g];
        a.state[f] = kDone;
        continue;
      }
    }
    const uint32_t slot = lb::find(a.t.keys, a.t.slots, sid);                // rule 7
    if (slot != lb::kNone) {
      a.state[f] = kHit | shape | slot;
      continue;
    }
    const lb::Service *svc = lb::find_service(a.t.svc, a.t.svc_slots, da, (sid.c >> 16) | proto << 16);
    if (!svc) {                                                              // rule 8, unless staging holds the key
      a.state[f] = kMiss | shape;
      continue;
    }
    const uint32_t bi = lb::backend_of(*svc, sid);                           // rule 9
    const lb::Backend b = a.t.bk[bi];
    const lb::Key back = lb::backward_key(b, sid);
    uint32_t *r = a.prop + f * kPropWords;
    st_agent(r + kSa, sid.a);
    st_agent(r + kSb, sid.b);
    st_agent(r + kSc, sid.c);
    st_agent(r + kProto, proto);
    st_agent(r + kBa, back.a);
    st_agent(r + kBb, back.b);
    st_agent(r + kBc, back.c);
    st_agent(r + kBackend, bi);
    st_agent(r + kMac0, ld_bytes(a.umem, off + 6, 4));
    st_agent(r + kMac1, ld_bytes(a.umem, off + 10, 2) & 0xffff);
    if (lb::find(a.t.keys, a.t.slots, back) != lb::kNone)
      __hip_atomic_fetch_or(&a.hdr[kOrderedFlag], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (the compare-and-swap's release orders the record before the index)
    r[kSlotS] = stage(a, sid, sid, static_cast<uint32_t>(f), 0);
    r[kSlotB] = stage(a, back, sid, static_cast<uint32_t>(f), 1);
    a.state[f] = kProposer | shape;
  }
  flush(a, c);
  if constexpr (kGate) {
    if (a.gate.counters && threadIdx.x < kAclTotals) {   // (flush's barrier stands before this)
      const uint32_t decided = c[lb::kPassed] + c[lb::kDropped];
      const uint32_t t = threadIdx.x == kAclFrames ? c[lb::kFrames] : threadIdx.x == kAclHits ? c[lb::kGated]
                         : threadIdx.x == kAclDecided ? decided : c[lb::kFrames] - c[lb::kGated] - decided;
      if (t) __hip_atomic_fetch_add(&a.gate.totals[threadIdx.x], static_cast<unsigned long long>(t), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// `nb` = 2 or 4 bytes of v at pos: 2-byte stores at even addresses, else bytes.
__device__ __forceinline__ void st_bytes(uint8_t *umem, uint64_t pos, uint32_t v, uint32_t nb) {
  if ((pos & 1) == 0) {
    for (uint32_t i = 0; i < nb; i += 2) *reinterpret_cast<uint16_t *>(umem + pos + i) = static_cast<uint16_t>(v >> (8 * i));
  } else {
    for (uint32_t i = 0; i < nb; ++i) umem[pos + i] = static_cast<uint8_t>(v >> (8 * i));
  }
}

// Rule 10 for ihl >= 5: the fields are disjoint, every read precedes every store.
__device__ __forceinline__ void rewrite_regs(uint8_t *umem, uint64_t off, uint32_t next, bool tcp, const lb::Val &v) {
  const bool to_backend = (v.m1 >> 16 & 0xff) == lb::kToBackend;
  const uint64_t apos = off + (to_backend ? 30 : 26), ppos = off + next + (to_backend ? 2 : 0);
  const uint64_t cpos = off + next + (tcp ? 16 : 6);
  const uint32_t old_addr = ld_bytes(umem, apos, 4), old_port = ld_bytes(umem, ppos, 2) & 0xffff;
  const uint32_t dmac0 = ld_bytes(umem, off, 4), dmac1 = ld_bytes(umem, off + 4, 2) & 0xffff;
  const uint32_t ipc = ld_bytes(umem, off + 24, 2), l4c = ld_bytes(umem, cpos, 2);
  const uint32_t new_port = v.pi & 0xffff;
  st_bytes(umem, apos, v.addr, 4);
  st_bytes(umem, ppos, new_port, 2);
  st_bytes(umem, off + 6, dmac0, 4);
  st_bytes(umem, off + 10, dmac1, 2);
  st_bytes(umem, off, v.m0, 4);
  st_bytes(umem, off + 4, v.m1 & 0xffff, 2);
  st_bytes(umem, off + 24, lb::check_update(ipc, old_addr, v.addr, false, 0, 0), 2);
  st_bytes(umem, cpos, lb::check_update(l4c, old_addr, v.addr, true, old_port, new_port), 2);
}

__global__ __launch_bounds__(kThreads) void lb_apply(const Args a) {
  if (!parallel_path(a)) return;
  __shared__ uint32_t c[lb::kStats];
  if (threadIdx.x < lb::kStats) c[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t f = blockIdx.x * kThreads + threadIdx.x; f < a.n; f += stride) {
    const uint32_t st = a.state[f], cls = st & kClassMask;
    if (cls == kDone) continue;
    const uint4 d = a.descs[f];
    const uint64_t off = desc_offset(static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32);
    const bool tcp = st >> 29 & 1;
    const uint32_t ihl = st >> 25 & 15, next = 14 + 4 * ihl;
    lb::Val v;
    bool have = true;
    if (cls == kHit) {
      v = a.t.vals[st & 0xffffff];
    } else if (cls == kProposer) {
      // the flow's creator is this frame or an earlier one of the same sid:
      // the forward session is a function of the sid
      v = lb::forward_val(a.t.bk[a.prop[f * kPropWords + kBackend]]);
    } else {
      const lb::Key sid = {ld_bytes(a.umem, off + 26, 4), ld_bytes(a.umem, off + 30, 4),
                           ld_bytes(a.umem, off + next, 4), tcp ? 6u : 17u};
      const uint32_t cur = staged(a, sid);
      const uint32_t j = (cur >> 1) - 1;
      have = cur != 0 && j <= f;   // created by an earlier frame of this batch
      if (have) {
        const uint32_t *r = a.prop + static_cast<uint64_t>(j) * kPropWords;
        if (cur & 1) v = lb::backward_val(lb::Key{r[kSa], r[kSb], r[kSc], r[kProto]}, r[kMac0], r[kMac1], a.ingress);
        else v = lb::forward_val(a.t.bk[r[kBackend]]);
      }
    }
    if (!have) {
      a.verdicts[f] = a.pass;
      count(c, lb::kPassed);
      continue;
    }
    if (ihl >= 5) rewrite_regs(a.umem, off, next, tcp, v);
    else (void)lb::rewrite(a.umem + off, next, tcp ? 6 : 17, v);
    a.verdicts[f] = static_cast<int32_t>(v.pi >> 16);
    count(c, lb::kRewritten);
  }
  flush(a, c);
}

// Store a key that the table does not hold and no other lane stores: claim the
// first empty slot from its hash on.
__device__ __forceinline__ void commit_one(const Args &a, const lb::Key &k, const lb::Val &v) {
  const uint32_t mask = a.t.slots - 1;
  uint32_t s = lb::key_hash(k) & mask;
  for (uint32_t i = 0; i < a.t.slots; ++i) {   // sessions <= max_sessions <= slots / 2
    uint32_t empty = 0;
    if (__hip_atomic_compare_exchange_strong(&a.t.keys[s].p, &empty, k.p, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
      a.t.keys[s].a = k.a;
      a.t.keys[s].b = k.b;
      a.t.keys[s].c = k.c;
      a.t.vals[s] = v;
      return;
    }
    s = (s + 1) & mask;
  }
}

__global__ __launch_bounds__(kThreads) void lb_commit(const Args a) {
  if (!parallel_path(a)) return;
  const uint32_t stride = gridDim.x * kThreads;
  for (uint64_t f = blockIdx.x * kThreads + threadIdx.x; f < a.n; f += stride) {
    if ((a.state[f] & kClassMask) != kProposer) continue;
    const uint32_t *r = a.prop + f * kPropWords;
    const lb::Key sid = {r[kSa], r[kSb], r[kSc], r[kProto]};
    if (a.staging[r[kSlotS]] == enc(static_cast<uint32_t>(f), 0)) commit_one(a, sid, lb::forward_val(a.t.bk[r[kBackend]]));
    if (a.staging[r[kSlotB]] == enc(static_cast<uint32_t>(f), 1))
      commit_one(a, lb::Key{r[kBa], r[kBb], r[kBc], r[kProto]}, lb::backward_val(sid, r[kMac0], r[kMac1], a.ingress));
  }
}

// The slow, exact path: ONE lane walks the candidates of the batch in index
// order with the host model's own code (the parse decided the others in
// lb_propose, whatever the table holds).  Each frame costs a chain of
// dependent device-memory reads, microseconds, and nothing overlaps: it is
// for the rare batches the header names, not a way to run traffic.
__global__ __launch_bounds__(64) void lb_ordered(const Args a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (parallel_path(a)) {
    const uint32_t created = a.hdr[kNewKeys];
    *a.t.count += created;
    a.stats[lb::kCreated] += created;
    return;
  }
  a.stats[lb::kOrdered] += 1;
  const lb::Gate none = {nullptr, nullptr, 0};   // (a frame the gate decided is kDone)
  for (uint32_t f = 0; f < a.n; ++f) {
    if ((a.state[f] & kClassMask) == kDone) continue;
    const uint4 d = a.descs[f];
    const uint64_t off = desc_offset(static_cast<uint64_t>(d.x) | static_cast<uint64_t>(d.y) << 32);
    a.verdicts[f] = lb::frame(a.t, none, a.umem + off, d.z, a.ingress, a.pass, a.stats);
  }
}

}  // namespace lbk
}  // namespace xsknf_gpu
