// csum_device.h -- device code every kernel family of checksummer.hip shares:
// LDS / load / store helpers, the chunk and group sums, frame references, the
// header parse / verdict / check, what becomes of a finished check, the record
// counters.  Part of checksummer.hip's one translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "checksummer_internal.h"
#include "desc_rules.h"

namespace xsknf_gpu {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kHdrChunks = 7;    // window chunks 0..6 hold frame bytes [0, 97) at any 16-B phase
constexpr int kSlotBytes = 128;  // register kernel: per-group LDS header window

// ---- small device helpers ---------------------------------------------------

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) uint8_t lds_u8;

__device__ __forceinline__ void compiler_barrier() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p));
}

// may be unaligned: gfx950 LDS serves unaligned dword reads
__device__ __forceinline__ uint32_t lds_u32(uint32_t a) {
  return *reinterpret_cast<const __attribute__((address_space(3))) uint32_t *>(static_cast<uintptr_t>(a));
}

__device__ __forceinline__ uint4 lds_u128(uint32_t a) {
  const u32x4 x = *reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(static_cast<uintptr_t>(a));
  return make_uint4(x.x, x.y, x.z, x.w);
}

__device__ __forceinline__ void lds_store_u128(uint32_t a, uint4 v) {
  u32x4 x = {v.x, v.y, v.z, v.w};
  *reinterpret_cast<__attribute__((address_space(3))) u32x4 *>(static_cast<uintptr_t>(a)) = x;
}

__device__ __forceinline__ void lds_store_u8(uint32_t a, uint8_t v) {
  *reinterpret_cast<lds_u8 *>(static_cast<uintptr_t>(a)) = v;
}

__device__ __forceinline__ void lds_store_i32(uint32_t a, int32_t v) {
  *reinterpret_cast<__attribute__((address_space(3))) int32_t *>(static_cast<uintptr_t>(a)) = v;
}

__device__ __forceinline__ void lds_store_u32(uint32_t a, uint32_t v) {
  *reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(static_cast<uintptr_t>(a)) = v;
}

__device__ __forceinline__ int32_t lds_i32(uint32_t a) {
  return *reinterpret_cast<const __attribute__((address_space(3))) int32_t *>(static_cast<uintptr_t>(a));
}

#ifdef XSKNF_GUARD
// Debug instrument (`make guard`, tools/guard_run.py): every UMEM access of the
// split kernel's paths is checked against the ranges the host put in
// g_guard[1..6] (umem, descriptors, verdicts); an access outside them is
// recorded (source line, thread, address) and skipped -- a load reads the
// descriptor array's first 16 bytes instead -- so a bad address is found
// without faulting the GPU.  Not in the product library.
__device__ unsigned long long *g_guard;
template <typename P>
__device__ __forceinline__ bool guard_ok(P p, uint32_t bytes, int site) {
  unsigned long long *g = g_guard;
  if (!g) return true;
  const unsigned long long x = reinterpret_cast<uintptr_t>(p);
  const bool ok = (x >= g[1] && x + bytes <= g[2]) || (x >= g[3] && x + bytes <= g[4]) ||
                  (x >= g[5] && x + bytes <= g[6]);
  if (!ok) {
    const unsigned long long i = atomicAdd(g, 1ull);
    if (i < 2048) {
      g[8 + 2 * i] = (static_cast<unsigned long long>(site) << 32) | (blockIdx.x * 256u + threadIdx.x);
      g[9 + 2 * i] = x;
    }
  }
  return ok;
}
template <typename P>
__device__ __forceinline__ P guard_ld(P p, uint32_t bytes, int site) {
  return guard_ok(p, bytes, site) ? p : reinterpret_cast<P>(static_cast<uintptr_t>(g_guard[3]));
}
#define XSKNF_SITE , int site = __builtin_LINE()
#define XSKNF_GLD(p, bytes) guard_ld(p, bytes, __LINE__)
#define XSKNF_GST(p, bytes) if (guard_ok(p, bytes, __LINE__))
#else
#define XSKNF_SITE
#define XSKNF_GLD(p, bytes) (p)
#define XSKNF_GST(p, bytes)
#endif

// non-temporal 16-byte global load (streamed once)
__device__ __forceinline__ uint4 load_nt(const uint4 *p XSKNF_SITE) {
#ifdef XSKNF_GUARD
  p = guard_ld(p, 16, site);
#endif
  const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
  return make_uint4(x.x, x.y, x.z, x.w);
}

__device__ __forceinline__ void store_nt16(uint8_t *p, uint4 v XSKNF_SITE) {
#ifdef XSKNF_GUARD
  if (!guard_ok(p, 16, site)) return;
#endif
  u32x4 x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(p));
}

// v with byte i (0..15) replaced by b; i outside 0..15 leaves v unchanged
__device__ __forceinline__ uint4 put_byte(uint4 v, int i, uint32_t b) {
  const uint32_t sh = 8u * (i & 3);
  const uint32_t keep = ~(0xffu << sh), put = (b & 0xffu) << sh;
  const int w = i >> 2;
  if (i >= 0 && i < 16) {
    v.x = w == 0 ? ((v.x & keep) | put) : v.x;
    v.y = w == 1 ? ((v.y & keep) | put) : v.y;
    v.z = w == 2 ? ((v.z & keep) | put) : v.z;
    v.w = w == 3 ? ((v.w & keep) | put) : v.w;
  }
  return v;
}

// 0x01 in every byte b of the dword at window offset x with lo <= x+b < hi
// (bytes [a, b) of a dword, a/b clamped to 0..4: two 64-bit shifts of 0x01010101).
__device__ __forceinline__ uint32_t byte_ones(int lo, int hi, int x) {
  const int a8 = min(max(8 * (lo - x), 0), 32);
  const int b8 = min(max(8 * (hi - x), 0), 32);
  const uint32_t below_b = static_cast<uint32_t>((0x01010101ull << b8) >> 32);
  const uint32_t from_a = static_cast<uint32_t>(0x01010101ull << a8);
  return below_b & from_a;
}

// Bytes of one 16-byte chunk inside [lo, hi) (window offsets), summed by weight
// class: wl = bytes low in their 16-bit word, wh = high.
__device__ __forceinline__ void chunk_sum(const uint4 v, int x, int lo, int hi, uint32_t wl,
                                          uint32_t wh, uint32_t &acc_lo, uint32_t &acc_hi) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t m = byte_ones(lo, hi, x + 4 * j);
    acc_lo = __builtin_amdgcn_udot4(w[j], m & wl, acc_lo, false);
    acc_hi = __builtin_amdgcn_udot4(w[j], m & wh, acc_hi, false);
  }
}

// chunk_sum with a wave-uniform fast path: a chunk entirely inside or outside
// [lo, hi) needs no byte mask, only an include predicate on the weights.  Only
// when some lane of the wave holds a frame's head or tail chunk (at most two
// chunk slots per frame) does the wave run the per-byte masks.
__device__ __forceinline__ void chunk_sum_fast(const uint4 v, int x, int lo, int hi, uint32_t wl,
                                               uint32_t wh, uint32_t &acc_lo, uint32_t &acc_hi) {
  const bool inside = x >= lo && x + 16 <= hi;
  const bool outside = x + 16 <= lo || x >= hi;
  if (__builtin_amdgcn_ballot_w64(!inside && !outside)) {
    chunk_sum(v, x, lo, hi, wl, wh, acc_lo, acc_hi);
  } else {
    const uint32_t l = inside ? wl : 0u, h = inside ? wh : 0u;
    acc_lo = __builtin_amdgcn_udot4(v.x, l, acc_lo, false);
    acc_hi = __builtin_amdgcn_udot4(v.x, h, acc_hi, false);
    acc_lo = __builtin_amdgcn_udot4(v.y, l, acc_lo, false);
    acc_hi = __builtin_amdgcn_udot4(v.y, h, acc_hi, false);
    acc_lo = __builtin_amdgcn_udot4(v.z, l, acc_lo, false);
    acc_hi = __builtin_amdgcn_udot4(v.z, h, acc_hi, false);
    acc_lo = __builtin_amdgcn_udot4(v.w, l, acc_lo, false);
    acc_hi = __builtin_amdgcn_udot4(v.w, h, acc_hi, false);
  }
}

// Group sum via DPP (all lanes active): the total lands in the group's LAST lane.
template <int LPF>
__device__ __forceinline__ uint32_t group_sum_last(uint32_t v) {
  v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, true);   // row_shr:2
  if constexpr (LPF >= 8) v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, true);   // row_shr:4
  if constexpr (LPF >= 16) v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, true);  // row_shr:8
  if constexpr (LPF >= 32) v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false); // row_bcast:15
  if constexpr (LPF >= 64) v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false); // row_bcast:31
  return v;
}

__device__ __forceinline__ int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// The group's last lane's value on every lane of the group.
template <int LPF>
__device__ __forceinline__ uint32_t group_bcast_last(uint32_t v, int lane) {
  return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute((lane | (LPF - 1)) << 2, static_cast<int>(v)));
}

// ---- kernel arguments, frame references, descriptors -----------------------

// struct KernelArgs, and the check record a summing pass parks in verdicts[f]
// (make_record / is_record / ...): checksummer_internal.h

// Where a frame's bytes are and which 16-byte chunks cover them.  Frames that
// need no bytes (len < 14, or a descriptor outside the UMEM) point at a dummy
// 16-byte block so that every chunk load can be unconditional.
struct FrameRef {
  const uint4 *cp;   // 16-byte aligned window start (cp <= fp)
  uint8_t *fp;       // first byte of the frame
  int rs;            // fp - cp, 0..15
  int len;
  int nch;           // chunks in the window, >= 1
  bool exists;       // index < n
  bool live;         // exists, in range and len >= 14
};

__device__ __forceinline__ FrameRef make_ref(const KernelArgs &a, uint64_t addr, uint32_t len, bool exists) {
  FrameRef r;
  const uint64_t off = desc_offset(addr);
  // (frames of 2 GiB and more are treated as out of range: lengths are ints here)
  const bool in_range = in_umem(off, len, a.umem_size) && len < 0x80000000u;
  r.exists = exists;
  r.live = exists && in_range && len >= 14;
  r.len = static_cast<int>(len);
  if (r.live) {
    r.fp = a.umem + off;
    r.rs = static_cast<int>(reinterpret_cast<uintptr_t>(r.fp) & 15);
    r.cp = reinterpret_cast<const uint4 *>(r.fp - r.rs);
    r.nch = (r.rs + r.len + 15) >> 4;
  } else {
    r.fp = a.umem;
    r.rs = 0;
    r.cp = a.dummy;
    r.nch = 1;
  }
  return r;
}

// Descriptors travel per tile: the 64 descriptors of a tile (1 KiB, contiguous)
// are staged in LDS once, and each group reads its frame's descriptor there.
__device__ __forceinline__ FrameRef ref_from_lds(const KernelArgs &a, uint32_t dslot, uint32_t f) {
  const uint4 d = lds_u128(dslot);          // {addr lo, addr hi, len, options}
  return make_ref(a, (static_cast<uint64_t>(d.y) << 32) | d.x, d.z, f < a.n);
}

// ---- per-frame parse / verdict / check (shared by both kernel families) -----

struct Header {
  int u;              // udp header offset 14 + 4*ihl (ihl unvalidated, :52)
  bool ipv4, udp;
  uint32_t pseudo;    // :57-65, read before the check is cleared
  uint32_t old_check; // f[u+6..u+7], counted as 0 (:68)
};

// Frame byte i is at LDS address hb + i (hb may be unaligned).
__device__ __forceinline__ Header parse_header(uint32_t hb) {
  Header h;
  const uint32_t w12 = lds_u32(hb + 12);   // f[12..15]
  const uint32_t w20 = lds_u32(hb + 20);   // f[20..23]
  const uint32_t w24 = lds_u32(hb + 24);   // f[24..27]
  const uint32_t w28 = lds_u32(hb + 28);   // f[28..31]
  const uint32_t w32 = lds_u32(hb + 32);   // f[32..35]
  h.u = 14 + 4 * ((w12 >> 16) & 0x0f);
  const uint32_t wu = lds_u32(hb + h.u + 4);  // f[u+4..u+7]
  h.ipv4 = (w12 & 0xffffu) == 0x0008u;        // f[12..13] == 08 00
  h.udp = (w20 >> 24) == 17u;                 // f[23]
  // le16(26) + le16(28) + le16(30) + le16(32) + 17<<8 + le16(u+4)
  h.pseudo = (w24 >> 16) + (w28 & 0xffffu) + (w28 >> 16) + (w32 & 0xffffu) + 0x1100u + (wu & 0xffffu);
  h.old_check = wu >> 16;
  return h;
}

// checksummer_user.c:34-55 and :110-111
__device__ __forceinline__ int32_t verdict_of(const FrameRef &r, const Header &h, int32_t fwd, bool &do_sum) {
  do_sum = false;
  if (!r.live) return -1;                 // :34-37 (and out-of-range descriptors)
  if (!h.ipv4) return 0;                  // :39-41
  if (r.len < 34) return -1;              // :43-46
  if (!h.udp) return 0;                   // :48-50
  if (h.u + 8 > r.len) return -1;         // :53-55
  do_sum = true;
  return fwd;                             // :110-111
}

// :105-106, the one fold with the carry dropped
__device__ __forceinline__ uint16_t fold_check(uint32_t s) {
  return static_cast<uint16_t>(~static_cast<uint16_t>((s & 0xffffu) + (s >> 16)));
}

// :92-108 given the reduced payload sum P (old check still included)
__device__ __forceinline__ uint16_t check_of(const Header &h, uint32_t P, uint32_t mult) {
  return fold_check(h.pseudo + mult * (P - h.old_check));
}

// Whether the new check c must be written.  :68 clears the check and :108
// stores c: when c is the value the frame already holds (a NIC filled in the
// UDP checksum, tests/gen-traffic.lua:120 -- the reference's own traffic), the
// frame ends with the bytes it began with, and neither its sector nor a record
// is written.  (old_check is the same 2 bytes read as a little-endian u16.)
__device__ __forceinline__ bool check_changes(const KernelArgs &a, const Header &h, uint16_t c) {
  return c != static_cast<uint16_t>(h.old_check) || a.store_unchanged;
}

// kNoDefer (defer_min_len: every check in-line): checksummer_internal.h
constexpr uint32_t kDeferTileK = 2;   // a tile defers when K * (long frames) >= live frames
constexpr uint32_t kDeferMinLen = 1024;        // hybrid default (tools/tune.py: 64 B, 570 B
                                               // and IMIX prefer in-line, 1500 B deferred)

// Records per launch, for the scatter pass to pick its shape and to skip
// itself when nothing was parked (per device: a __device__ variable exists once
// per GPU).  Launch `seq` publishes into set seq % kCountSlots, 64 counter words
// on separate 64-byte lines (block b adds to word b % 64: one shared address
// would serialize the publishing atomics in one L2 channel).  A word is
// {launch seq (high 32 bits), records (low 32)}: a wave adds to it while it
// carries its own seq and restarts it (CAS) while it carries an older one.  The
// scatter pass sums the words tagged with its seq; words tagged older are a
// zero of this launch; a word tagged NEWER means a launch kCountSlots later
// reused the set while this one was in flight, and the count is unknown (the
// pass then scans every frame).  So "no records" is exact when it is reported.
constexpr uint32_t kCountSlots = 64;
constexpr uint32_t kCountLanes = 64;
constexpr uint32_t kCountStride = 8;           // u64 words = 64 bytes
constexpr uint32_t kCountUnknown = 0xffffffffu;
__device__ unsigned long long g_rec_count[kCountSlots][kCountLanes][kCountStride];

// Store a tile's result word (lane's frame); returns the tile's record count
// (wave-uniform), which the wave adds up and publishes once, at exit: an
// atomic per tile would hold every following vmcnt wait on its L2 round trip.
__device__ __forceinline__ uint32_t store_result(const KernelArgs &a, uint32_t f, bool valid, int32_t v) {
  if (valid) {
    XSKNF_GST(a.verdicts + f, 4) a.verdicts[f] = v;
  }
  if (!a.count_records) return 0;
  return static_cast<uint32_t>(__builtin_popcountll(
      __builtin_amdgcn_ballot_w64(valid && is_record(static_cast<uint32_t>(v)))));
}

__device__ __forceinline__ void publish_records(const KernelArgs &a, uint32_t nrec, int lane) {
  if (!a.count_records || lane != 0 || !nrec) return;
  unsigned long long *w = &g_rec_count[a.seq % kCountSlots][blockIdx.x % kCountLanes][0];
  unsigned long long old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const uint32_t tag = static_cast<uint32_t>(old >> 32);
    if (tag == a.seq) { atomicAdd(w, static_cast<unsigned long long>(nrec)); return; }
    if (static_cast<int32_t>(tag - a.seq) > 0) return;   // a newer launch owns the word
    const unsigned long long mine = (static_cast<unsigned long long>(a.seq) << 32) | nrec;
    const unsigned long long prev = atomicCAS(w, old, mine);
    if (prev == old) return;
    old = prev;
  }
}

// The launch's record count on every lane (kCountUnknown if the set was reused).
__device__ __forceinline__ uint32_t launch_records(const KernelArgs &a) {
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long w = __hip_atomic_load(&g_rec_count[a.seq % kCountSlots][lane % kCountLanes][0],
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t tag = static_cast<uint32_t>(w >> 32);
  uint32_t c = tag == a.seq ? static_cast<uint32_t>(w) : 0u;
  const bool newer = tag != a.seq && static_cast<int32_t>(tag - a.seq) > 0;
  if (__builtin_amdgcn_ballot_w64(newer)) return kCountUnknown;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += static_cast<uint32_t>(__shfl_xor(static_cast<int>(c), o, kWave));
  return c;
}

// Write a finished tile's results (LDS rec[0..63]) as one coalesced store.
__device__ __forceinline__ uint32_t flush_tile(const KernelArgs &a, uint32_t rec, uint32_t tile_f0, int lane) {
  compiler_barrier();
  const int32_t v = lds_i32(rec + 4 * lane);
  const uint32_t nrec = store_result(a, tile_f0 + lane, tile_f0 + lane < a.n, v);
  compiler_barrier();
  return nrec;
}

// ---- a frame owned by one lane (lane kernel, split kernel phases A and C) ------

constexpr int kLaneSlot = 16 * kHdrChunks;   // per-lane LDS header window

// Default-policy loads: a lane's chunks of one frame arrive in NCH separate
// (uncoalesced) instructions, and the line must stay in L2 between them (and
// for the sector store that follows); non-temporal loads refetch it.
// Chunks 4 and up are loaded only when some frame of the wave's step reaches
// them (a wave-uniform branch): a step of 16-byte-aligned 64 B frames then
// issues 4 load instructions of a 5-chunk window, not 5 (the fifth re-read
// the fourth chunk: one more instruction's worth of requests per frame), and a
// step with frames at odd starts still loads its 5 chunks at once.
template <int NCH>
__device__ __forceinline__ void load_lane(const FrameRef &r, uint4 (&v)[NCH]) {
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    if (k < 4 || __builtin_amdgcn_ballot_w64(k < r.nch))
      v[k] = *XSKNF_GLD(r.cp + min(k, r.nch - 1), 16);
    else
      v[k] = make_uint4(0, 0, 0, 0);   // past every frame of the step: outside every sum and parse
  }
}

#ifdef XSKNF_TIMELINE
// A/B instrument (tools/timeline.py): per wave of the split and lane kernels, the
// constant 100 MHz clock at its start, after its last tile, after its patches,
// and its tile count, so the step can be split into stream and patch time.
__device__ unsigned long long *g_timeline;
// 8 u64 per wave: start, stream done, patches done, tiles, then the clock
// summed over the wave's tiles in phase A (window loads until they are in
// LDS), phase A's parse, and phase B (payload items)
__device__ __forceinline__ void timeline_put(uint32_t wave, int lane, unsigned long long t0, unsigned long long t1,
                                             int tiles, unsigned long long sa, unsigned long long sp,
                                             unsigned long long sb) {
  const unsigned long long t2 = wall_clock64();
  unsigned long long *p = g_timeline;
  const unsigned long long v[8] = {t0, t1, t2, static_cast<unsigned long long>(tiles), sa, sp, sb, 0ull};
  unsigned long long x = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) x = lane == k ? v[k] : x;
  if (p && lane < 8) p[8ull * wave + lane] = x;
}
#endif

// A lane's result; when `sector` is set, the frame's patched 64-byte check
// sector sits in the lane's LDS slot at `lds_sec`, to be written to `gsec` by
// the wave's cooperative store (store_sectors).
struct LaneOut {
  int32_t res;
  bool sector;
  uint32_t lds_sec;
  uint8_t *gsec;
};

// One 16-byte piece of an in-line check sector: non-temporal, or (wt) sc1 nt,
// written through the XCD's L2 at once.  Frames 2 KiB apart (the aligned
// UMEM) share no line, and there the write-through store leaves no dirty line
// for the end of the launch to write back: 64 B 58.0-58.3 vs 60.1-60.5 us; for
// frames packed back to back (-u) it costs 38.2 -> 42.2 us, sectors there
// sharing their 128-byte lines (profiles/r05/ab/ab_lane_sc*.jsonl; sc1 alone
// and sc0 sc1: no gain).
__device__ __forceinline__ void store_sector16(uint8_t *p, uint4 v, bool wt XSKNF_SITE) {
  if (!wt) {
    store_nt16(p, v);
    return;
  }
#ifdef XSKNF_GUARD
  if (!guard_ok(p, 16, site)) return;
#endif
  const u32x4 x = {v.x, v.y, v.z, v.w};
  // (s_nop 1: the store reads its data registers after issue, and the next
  // instruction hipcc places after the statement may overwrite them)
  asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
}

// The wave's patched sectors, 16 per instruction: lanes 4i..4i+3 write the 4
// pieces of lane (16p + i)'s sector -- one coalesced 64-byte request each,
// instead of 4 separate 16-byte stores per lane.
__device__ __forceinline__ void store_sectors(const LaneOut &o, int lane, bool plain, bool wt = false) {
  const uint64_t any = __builtin_amdgcn_ballot_w64(o.sector);
  if (!any) return;
  compiler_barrier();
  const uint32_t glo = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(o.gsec));
  const uint32_t ghi = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(o.gsec) >> 32);
#pragma unroll
  for (int p = 0; p < kWave / 16; ++p) {
    if (!((any >> (16 * p)) & 0xffffull)) continue;
    const int src = 16 * p + (lane >> 2);
    const int sa = src << 2;
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sa, static_cast<int>(glo)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sa, static_cast<int>(ghi)));
    const uint32_t ls = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sa, static_cast<int>(o.lds_sec)));
    if ((any >> src) & 1) {
      uint8_t *g = reinterpret_cast<uint8_t *>((static_cast<uintptr_t>(hi) << 32) | lo);
      const uint4 w = lds_u128(ls + 16 * (lane & 3));
      if (plain) {
        XSKNF_GST(g + 16 * (lane & 3), 16) *reinterpret_cast<uint4 *>(g + 16 * (lane & 3)) = w;
      } else {
        store_sector16(g + 16 * (lane & 3), w, wt);
      }
    }
  }
  compiler_barrier();
}

__device__ __forceinline__ FrameRef lane_ref(const KernelArgs &a, const uint4 d, uint32_t f) {
  return make_ref(a, (static_cast<uint64_t>(d.y) << 32) | d.x, d.z, f < a.n);
}

constexpr uint32_t kNoTile = 0xffffffffu;   // no tile / unit

// entry flags; kPatchInWin + window offset / 16 << 25 say where the sector lies
// in the frame's header window (round 4 took such sectors from the slots
// instead of reading them again: no gain, removed in round 5)
constexpr uint32_t kPatchValid = 1u << 23, kPatchWhole = 1u << 22, kPatchInWin = 1u << 24;
constexpr uint64_t kPatchMaxUmem = 1ull << 37;   // sector index: 32 bits (with margin)

// A deferred check as an entry of the split kernel's patch list (kernel_split.h).
__device__ __forceinline__ uint2 patch_entry(const KernelArgs &a, const FrameRef &r, int u, uint16_t c, int wbytes) {
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(r.fp);
  const uintptr_t ck = f0 + static_cast<uintptr_t>(u) + 6;
  const uintptr_t sec = ck & ~static_cast<uintptr_t>(63);
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.umem) & ~static_cast<uintptr_t>(63);
  const bool whole = sec >= f0 && sec + 64 <= f0 + static_cast<uintptr_t>(r.len) && (ck & 63) != 63;
  const uintptr_t c0 = reinterpret_cast<uintptr_t>(r.cp);
  const bool in_win = whole && sec >= c0 && sec + 64 <= c0 + static_cast<uintptr_t>(wbytes);
  return make_uint2(static_cast<uint32_t>((sec - base) >> 6),
                    kPatchValid | (whole ? kPatchWhole : 0u) | static_cast<uint32_t>((ck & 63) << 16) | c |
                        (in_win ? kPatchInWin | static_cast<uint32_t>((sec - c0) >> 4) << 25 : 0u));
}

// In-line check c of a lane-owned frame (lane kernel, split phases A and C):
// the whole 64-byte sector when it lies inside the frame and the wbytes of
// window in the lane's LDS slot -- the two bytes are patched there and `out`
// says where the sector is, for the wave's store_sectors -- else the 2 bytes.
__device__ __forceinline__ void store_check_inline(const KernelArgs &a, const FrameRef &r, int u, uint16_t c,
                                                   int wbytes, uint32_t slot, LaneOut &out) {
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(r.fp);
  const uintptr_t ck = f0 + u + 6;
  const uintptr_t sec = ck & ~static_cast<uintptr_t>(63);
  const uintptr_t c0 = reinterpret_cast<uintptr_t>(r.cp);
  if (a.sector_stores && sec >= f0 && sec + 64 <= f0 + r.len && (ck & 63) != 63 && sec >= c0 &&
      sec + 64 <= c0 + wbytes) {
    const uint32_t at = slot + static_cast<uint32_t>(ck - c0);
    lds_store_u8(at, static_cast<uint8_t>(c));
    lds_store_u8(at + 1, static_cast<uint8_t>(c >> 8));
    out.sector = true;
    out.lds_sec = slot + static_cast<uint32_t>(sec - c0);
    out.gsec = r.fp + static_cast<intptr_t>(sec - f0);   // global addressing from fp
  } else {
    XSKNF_GST(r.fp + u + 6, 2) *reinterpret_cast<uint16_t *>(r.fp + u + 6) = c;   // :108
  }
}

}  // namespace xsknf_gpu
