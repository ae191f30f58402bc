// kernel_plan.h -- the kernels of the device-side shard planner (plan_device.hip):
// what shard_plan.cpp computes on one CPU thread, over descriptors that already
// lie in the root's device memory.
//
// One u64 block scan (block_incl_scan) serves both prefix sums: over `len` for
// the byte-balanced cuts and over the packed slot length for the packed layout.
// The scan over the whole batch is three stream-ordered passes, so that NO block
// ever waits on another block (no look-back, no grid barrier, no flag):
//   1. plan_block_totals: every block sums its tile of kTile frames;
//   2. plan_scan_totals:  ONE block turns the block totals into exclusive
//      prefixes and, for each cut, finds the block that holds it;
//   3. plan_cuts (one block per cut, rescanning only the tile that holds it) and
//      plan_pack (every block scans its tile with its carry-in).
// The price is a second read of the descriptors.
//
// A tile is kPerThread rounds of one descriptor per lane, each a 16-byte load
// (frame base + round * 256 + thread: consecutive lanes, consecutive records).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"
#include "block_scan.h"
#include "desc_rules.h"

namespace xsknf_gpu {
namespace plan {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr uint32_t kTile = kThreads * kPerThread;   // frames per block
constexpr uint32_t kMaxShards = 64;
constexpr unsigned long long kNone = ~0ull;

// The workspace, in u64 words.  The first kResultWords are what the host reads
// back in one copy; the block prefixes follow the header: lenpre[nb + 1], then
// slotpre[nb + 1] (nb = tiles of the batch; entry nb holds the total).
enum : uint32_t {
  kBounds = 0,                          // nshards + 1 cuts
  kBytes = kBounds + kMaxShards + 1,    // per-shard frame bytes
  kAux = kBytes + kMaxShards,           // spans[2 * nshards] or sizes[nshards]
  kResultWords = kAux + 2 * kMaxShards,
  kCum = kResultWords,                  // running bytes before each cut (nshards + 1)
  kSlotCum = kCum + kMaxShards + 1,     // running slot bytes before each cut
  kTarget = kSlotCum + kMaxShards + 1,  // the cuts' targets (doubles)
  kCutBlock = kTarget + kMaxShards,     // the tile that holds each cut
  kRawSpan = kCutBlock + kMaxShards,    // min / max pairs the blocks reduce into
  kHeaderWords = kRawSpan + 2 * kMaxShards,
};

struct Desc {
  uint64_t addr;
  uint32_t len, options;
};

__device__ inline Desc load_desc(const uint4 *descs, uint64_t f) {
  const uint4 v = descs[f];
  return {static_cast<uint64_t>(v.x) | static_cast<uint64_t>(v.y) << 32, v.z, v.w};
}

__device__ inline void store_desc(uint4 *out, uint64_t f, uint64_t addr, uint32_t len, uint32_t options) {
  out[f] = make_uint4(static_cast<uint32_t>(addr), static_cast<uint32_t>(addr >> 32), len, options);
}

// Bytes of a frame's slot in its shard's packed buffer (shard_plan.cpp
// xsknf_gpu_shard_pack_plan): whole 16-byte chunks at the frame's address mod 16.
__device__ inline uint64_t slot_len(uint64_t umem_addr, uint64_t off, uint32_t len, uint64_t umem_size) {
  if (len == 0 || !in_umem(off, len, umem_size)) return 0;
  return slot_bytes(umem_addr + off, len);
}

// The u64 block scan (block_scan.h), shared with the router's kernels.
static_assert(scan::kThreads == kThreads, "block_incl_scan scans a block of kThreads");
using scan::block_incl_scan;

// The shard of frame f: the last k < nshards with sb[k] <= f (empty shards
// share a bound with their successor; f < sb[nshards]).
__device__ inline int find_shard(const uint64_t *sb, int nshards, uint64_t f) {
  int lo = 0, hi = nshards - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sb[mid] <= f) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Pass 1: lenpre[b] = the bytes of tile b's frames (every descriptor counts, in
// the UMEM or not), slotpre[b] = its slot bytes (packed mode).
__global__ void __launch_bounds__(kThreads) plan_block_totals(const uint4 *descs, uint64_t n, uint64_t umem_addr,
                                                              uint64_t umem_size, int packed, uint64_t *lenpre,
                                                              uint64_t *slotpre) {
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile;
  uint64_t sl = 0, ss = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * kThreads + threadIdx.x;
    if (f < n) {
      const Desc d = load_desc(descs, f);
      sl += d.len;
      if (packed) ss += slot_len(umem_addr, desc_offset(d.addr), d.len, umem_size);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    sl += __shfl_xor(sl, o);
    ss += __shfl_xor(ss, o);
  }
  __shared__ uint64_t red[2][kThreads / 64];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = sl;
    red[1][threadIdx.x >> 6] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lenpre[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    if (packed) slotpre[blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// Pass 2, one block: the block totals become exclusive prefixes in place (entry
// nb: the total); each cut r gets its target -- the host's double(total * r) /
// nshards, IEEE division, so this file is never built with fast-math -- and
// the first tile whose running bytes reach it; the header's fixed entries.
__global__ void __launch_bounds__(kThreads) plan_scan_totals(uint64_t *ws, uint64_t nb, uint64_t n, int nshards,
                                                             int packed) {
  __shared__ uint64_t wtot[kThreads / 64];
  uint64_t *lenpre = ws + kHeaderWords, *slotpre = lenpre + nb + 1;
  for (int a = 0; a < (packed ? 2 : 1); ++a) {
    uint64_t *arr = a ? slotpre : lenpre;
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < nb; i0 += kThreads) {
      const uint64_t i = i0 + threadIdx.x;
      const uint64_t v = i < nb ? arr[i] : 0;
      uint64_t tot;
      const uint64_t incl = block_incl_scan(v, wtot, &tot);
      if (i < nb) arr[i] = carry + incl - v;
      carry += tot;
    }
    if (threadIdx.x == 0) arr[nb] = carry;
  }
  __syncthreads();   // the prefixes, written by this block, are read below
  const uint64_t total = lenpre[nb];
  const int r = threadIdx.x;
  if (r >= 1 && r < nshards) {
    const double target = static_cast<double>(total * static_cast<uint64_t>(r)) / nshards;
    // the first tile b whose inclusive running bytes lenpre[b + 1] are not below the target
    uint64_t lo = 0, hi = nb - 1;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (static_cast<double>(lenpre[mid + 1]) < target) lo = mid + 1; else hi = mid;
    }
    ws[kTarget + r] = static_cast<uint64_t>(__double_as_longlong(target));
    ws[kCutBlock + r] = lo;
  }
  if (threadIdx.x == 0) {
    ws[kBounds] = 0;
    ws[kBounds + nshards] = n;
    ws[kCum] = 0;
    ws[kCum + nshards] = total;
    ws[kSlotCum] = 0;
    ws[kSlotCum + nshards] = packed ? slotpre[nb] : 0;
  }
  if (threadIdx.x < 2 * nshards) ws[kRawSpan + threadIdx.x] = (threadIdx.x & 1) ? 0 : kNone;
}

// Pass 3a, block r - 1 for cut r: rescan the tile that holds the cut; the first
// frame whose inclusive running bytes are not below the target ends shard r - 1
// (shard_plan.cpp:43-50: cut = that frame + 1; the cuts come out non-decreasing
// and <= n by themselves, the targets being non-decreasing and <= total).  The
// running bytes and slot bytes at the cut are kept: shard sums are differences.
__global__ void __launch_bounds__(kThreads) plan_cuts(const uint4 *descs, uint64_t n, uint64_t umem_addr,
                                                      uint64_t umem_size, uint64_t nb, int packed, uint64_t *ws) {
  __shared__ uint64_t wtot[kThreads / 64];
  __shared__ unsigned long long best;
  const int r = blockIdx.x + 1;
  const uint64_t *lenpre = ws + kHeaderWords, *slotpre = lenpre + nb + 1;
  const uint64_t b = ws[kCutBlock + r];
  const double target = __longlong_as_double(static_cast<long long>(ws[kTarget + r]));
  uint64_t carry_l = lenpre[b], carry_s = packed ? slotpre[b] : 0;
  if (threadIdx.x == 0) best = kNone;
  const uint64_t base = b * kTile;
  bool found = false;
  uint64_t my_f = 0, my_cum = 0, my_slot = 0;
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * kThreads + threadIdx.x;
    uint64_t len = 0, slot = 0;
    if (f < n) {
      const Desc d = load_desc(descs, f);
      len = d.len;
      if (packed) slot = slot_len(umem_addr, desc_offset(d.addr), d.len, umem_size);
    }
    uint64_t tl, ts = 0, si = 0;
    const uint64_t li = block_incl_scan(len, wtot, &tl) + carry_l;
    carry_l += tl;
    if (packed) {
      si = block_incl_scan(slot, wtot, &ts) + carry_s;
      carry_s += ts;
    }
    if (!found && f < n && !(static_cast<double>(li) < target)) {
      found = true;
      my_f = f;
      my_cum = li;
      my_slot = si;
    }
  }
  // (the scans' barriers order the store to `best` before these)
  if (found) atomicMin(&best, static_cast<unsigned long long>(my_f));
  __syncthreads();
  if (found && best == my_f) {
    ws[kBounds + r] = my_f + 1;
    ws[kCum + r] = my_cum;
    ws[kSlotCum + r] = my_slot;
  }
  if (best == kNone && threadIdx.x == 0) {   // no frame reaches the target: the host's clamp to n
    ws[kBounds + r] = n;
    ws[kCum + r] = ws[kCum + gridDim.x + 1];
    ws[kSlotCum + r] = ws[kSlotCum + gridDim.x + 1];
  }
}

// Block 0 of the per-frame passes: the shard sums, as differences.
__device__ inline void write_sums(uint64_t *ws, int nshards, bool sizes) {
  if (threadIdx.x < nshards) {
    ws[kBytes + threadIdx.x] = ws[kCum + threadIdx.x + 1] - ws[kCum + threadIdx.x];
    if (sizes) ws[kAux + threadIdx.x] = ws[kSlotCum + threadIdx.x + 1] - ws[kSlotCum + threadIdx.x];
  }
}

// Span mode, pass 3b: each shard's min offset / max end over its frames inside
// the UMEM.  A thread folds its frames while they stay in one shard, a wave
// whose lanes all hold the same shard folds by shuffles, the block folds in LDS
// and one vector atomic pair per shard and block goes to device memory.
__global__ void __launch_bounds__(kThreads) plan_spans(const uint4 *descs, uint64_t n, uint64_t umem_size,
                                                       int nshards, uint64_t *ws) {
  __shared__ uint64_t sb[kMaxShards + 1];
  __shared__ unsigned long long smin[kMaxShards], smax[kMaxShards];
  if (threadIdx.x <= nshards) sb[threadIdx.x] = ws[kBounds + threadIdx.x];
  if (threadIdx.x < nshards) {
    smin[threadIdx.x] = kNone;
    smax[threadIdx.x] = 0;
  }
  if (blockIdx.x == 0) write_sums(ws, nshards, false);
  __syncthreads();
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile;
  int cur = -1;
  unsigned long long lo = kNone, hi = 0;
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * kThreads + threadIdx.x;
    if (f >= n) break;
    const Desc d = load_desc(descs, f);
    const uint64_t off = desc_offset(d.addr);
    if (!in_umem(off, d.len, umem_size)) continue;
    const int k = find_shard(sb, nshards, f);
    if (k != cur) {
      if (cur >= 0) {
        atomicMin(&smin[cur], lo);
        atomicMax(&smax[cur], hi);
      }
      cur = k;
      lo = kNone;
      hi = 0;
    }
    if (off < lo) lo = off;
    if (off + d.len > hi) hi = off + d.len;
  }
  if (__all(cur == __shfl(cur, 0))) {
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
      if (l2 < lo) lo = l2;
      if (h2 > hi) hi = h2;
    }
    if ((threadIdx.x & 63) != 0) cur = -1;
  }
  if (cur >= 0) {
    atomicMin(&smin[cur], lo);
    atomicMax(&smax[cur], hi);
  }
  __syncthreads();
  if (threadIdx.x < nshards && smin[threadIdx.x] != kNone) {
    atomicMin(reinterpret_cast<unsigned long long *>(ws + kRawSpan + 2 * threadIdx.x), smin[threadIdx.x]);
    atomicMax(reinterpret_cast<unsigned long long *>(ws + kRawSpan + 2 * threadIdx.x + 1), smax[threadIdx.x]);
  }
}

// Span mode, pass 4: the descriptors each shard receives, relative to its
// span's first byte (xsknf_gpu_shard_rebase per shard); block 0 writes the
// spans the host reads ({0, 0} for a shard with no frame inside the UMEM).
__global__ void __launch_bounds__(kThreads) plan_rebase(const uint4 *descs, uint64_t n, uint64_t umem_size,
                                                        int nshards, uint64_t *ws, uint4 *out) {
  __shared__ uint64_t sb[kMaxShards + 1], b0[kMaxShards];
  if (threadIdx.x <= nshards) sb[threadIdx.x] = ws[kBounds + threadIdx.x];
  if (threadIdx.x < nshards) {
    const uint64_t lo = ws[kRawSpan + 2 * threadIdx.x], hi = ws[kRawSpan + 2 * threadIdx.x + 1];
    b0[threadIdx.x] = lo == kNone ? 0 : lo;
    if (blockIdx.x == 0) {
      ws[kAux + 2 * threadIdx.x] = lo == kNone ? 0 : lo;
      ws[kAux + 2 * threadIdx.x + 1] = lo == kNone ? 0 : hi;
    }
  }
  __syncthreads();
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile;
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * kThreads + threadIdx.x;
    if (f >= n) break;
    const Desc d = load_desc(descs, f);
    const uint64_t off = desc_offset(d.addr);
    const uint64_t addr = in_umem(off, d.len, umem_size) ? off - b0[find_shard(sb, nshards, f)] : kOutOfRange;
    store_desc(out, f, addr, d.len, d.options);
  }
}

// Packed mode, pass 3b: every block scans its tile's slot bytes with its
// carry-in; a frame's slot starts at its global exclusive prefix minus the
// prefix at its shard's first frame (the scan restarts at every bound), and its
// address there keeps the frame's address mod 16.
__global__ void __launch_bounds__(kThreads) plan_pack(const uint4 *descs, uint64_t n, uint64_t umem_addr,
                                                      uint64_t umem_size, uint64_t nb, int nshards, uint64_t *ws,
                                                      uint4 *out) {
  __shared__ uint64_t wtot[kThreads / 64];
  __shared__ uint64_t sb[kMaxShards + 1], sc[kMaxShards];
  if (threadIdx.x <= nshards) sb[threadIdx.x] = ws[kBounds + threadIdx.x];
  if (threadIdx.x < nshards) sc[threadIdx.x] = ws[kSlotCum + threadIdx.x];
  if (blockIdx.x == 0) write_sums(ws, nshards, true);
  __syncthreads();
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile;
  uint64_t carry = ws[kHeaderWords + nb + 1 + blockIdx.x];
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * kThreads + threadIdx.x;
    Desc d = {0, 0, 0};
    uint64_t off = 0, slot = 0;
    if (f < n) {
      d = load_desc(descs, f);
      off = desc_offset(d.addr);
      slot = slot_len(umem_addr, off, d.len, umem_size);
    }
    uint64_t tot;
    const uint64_t incl = block_incl_scan(slot, wtot, &tot) + carry;
    carry += tot;
    if (f < n) {
      const uint64_t addr = in_umem(off, d.len, umem_size)
                                ? incl - slot - sc[find_shard(sb, nshards, f)] + ((umem_addr + off) & 15)
                                : kOutOfRange;
      store_desc(out, f, addr, d.len, d.options);
    }
  }
}

}  // namespace plan
}  // namespace xsknf_gpu
