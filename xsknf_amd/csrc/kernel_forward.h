// kernel_forward.h -- the kernel of the device-side frame forward
// (forward_device.hip): the copy of src/xsknf.c:563-571 for a routed batch whose
// tx lists lie in device memory -- every frame of an interface with a UMEM of
// its own is copied from the rx UMEM into that UMEM at the same offset, what
// forward_host.cpp does on one CPU thread.
//
// One launch of a persistent grid; no block waits on another.  Every block
// reads the <= 33 counts the router left and builds the interface bases in LDS.
// The work is dealt as kernel_pack.h pack_frames deals it: a wave takes 64
// consecutive entries (a tile), prefix-sums their 16-byte chunk counts and its
// lanes take the tile's chunks round robin, kUnroll rounds at a time, so a
// 9000-byte frame and the 1-byte frames beside it keep all 64 lanes busy.
//
// Source and destination share the offset and both bases are 16-byte aligned, so
// a frame's chunks are aligned in both.  A chunk that lies wholly inside its
// frame moves as one 16-byte load and store.  The first and last chunk of a
// frame that is not aligned are partial: their bytes INSIDE the frame move as
// aligned 8-, 4-, 2- and 1-byte pieces (copy_edge); the bytes around the frame
// in the destination are another frame's, or nobody's, and are neither read nor
// written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"
#include "desc_rules.h"
#include "forward_args.h"

// Destination stores non-temporal (the product: DESIGN 4.2's A/B) or plain (0)
#ifndef XSKNF_FORWARD_NT
#define XSKNF_FORWARD_NT 1
#endif

namespace xsknf_gpu {
namespace forward {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;            // rounds of 64 chunks in flight per wave
constexpr uint32_t kMaxBlocks = 2048; // 256 CUs x 8 blocks

// The destination UMEMs, by value in the kernel's arguments.  base[i] == NULL:
// interface i shares the rx UMEM (the host side has folded "equals rx_umem" into
// NULL) and its entries are not looked at.
struct TxUmems {
  uint8_t *base[kMaxInterfaces];
  uint64_t size[kMaxInterfaces];
};

__device__ inline void store16(uint4 *p, uint4 v) {
#if XSKNF_FORWARD_NT
  typedef uint32_t v4u __attribute__((ext_vector_type(4)));   // one 16-byte store, not four
  __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u *>(p));
#else
  *p = v;
#endif
}

// Bytes [b0, b1) of one aligned 16-byte chunk (0 <= b0 < b1 <= 16; s and d are
// the chunk's first byte in the source and the destination): the largest
// aligned piece that fits, then the next.  Nothing outside [b0, b1) is touched.
__device__ inline void copy_edge(uint8_t *d, const uint8_t *s, uint32_t b0, uint32_t b1) {
  uint32_t p = b0;
  while (p < b1) {
    const uint32_t left = b1 - p;
    if (!(p & 7) && left >= 8) {
      *reinterpret_cast<uint64_t *>(d + p) = *reinterpret_cast<const uint64_t *>(s + p);
      p += 8;
    } else if (!(p & 3) && left >= 4) {
      *reinterpret_cast<uint32_t *>(d + p) = *reinterpret_cast<const uint32_t *>(s + p);
      p += 4;
    } else if (!(p & 1) && left >= 2) {
      *reinterpret_cast<uint16_t *>(d + p) = *reinterpret_cast<const uint16_t *>(s + p);
      p += 2;
    } else {
      d[p] = s[p];
      p += 1;
    }
  }
}

// stats: [0] frames copied, [1] bytes copied, [2] frames skipped (zeroed on the
// stream before the launch).  `n` bounds the entries read whatever the counts say.
__global__ void __launch_bounds__(kThreads) forward_frames(const uint8_t *rx, uint64_t rx_size, TxUmems tx,
                                                           uint32_t nif, const xsknf_gpu_desc *tx_descs,
                                                           const uint64_t *counts, uint32_t n,
                                                           unsigned long long *stats) {
  __shared__ uint64_t s_base[kMaxInterfaces + 1];     // interface i's list is [s_base[i], s_base[i + 1])
  __shared__ uint64_t s_dst[kMaxInterfaces], s_dsize[kMaxInterfaces];
  __shared__ uint64_t pre[kWaves][65];                // a tile's chunks before each frame (u64: 64 lengths of 2^32)
  __shared__ uint64_t off_of[kWaves][64];             // a frame's offset in both UMEMs ...
  __shared__ uint64_t dst_of[kWaves][64];             // ... its destination UMEM ...
  __shared__ uint32_t len_of[kWaves][64];             // ... and its length (read by any lane)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

  if (wv == 0) {
    // inclusive scan of the counts over the wave's first nif lanes
    uint64_t x = lane < static_cast<int>(nif) ? counts[lane] : 0;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane < static_cast<int>(nif)) s_base[lane + 1] = x;
    if (lane == 0) s_base[0] = 0;
    // (constant indices: the arguments stay in scalar registers, no private copy)
#pragma unroll
    for (int i = 0; i < static_cast<int>(kMaxInterfaces); ++i) {
      if (lane == i) {
        s_dst[i] = reinterpret_cast<uintptr_t>(tx.base[i]);
        s_dsize[i] = tx.size[i];
      }
    }
  }
  __syncthreads();
  const uint64_t all = s_base[nif];
  const uint64_t total = all < n ? all : n;   // never an entry at or past the capacity
  const uint64_t tiles = (total + 63) / 64;

  unsigned long long c_frames = 0, c_bytes = 0, c_skipped = 0;
  for (uint64_t t = blockIdx.x * static_cast<uint64_t>(kWaves) + wv; t < tiles;
       t += gridDim.x * static_cast<uint64_t>(kWaves)) {
    const uint64_t e = t * 64 + lane;
    uint64_t off = 0, dst = 0;
    uint32_t len = 0;
    uint64_t nch = 0;
    if (e < total) {
      // the entry's interface: the last i < nif with s_base[i] <= e (an empty
      // list before it has the same base and a smaller i)
      int lo = 0, hi = static_cast<int>(nif) - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_base[mid] <= e) lo = mid; else hi = mid - 1;
      }
      dst = s_dst[lo];
      if (dst) {
        const xsknf_gpu_desc d = tx_descs[e];
        off = desc_offset(d.addr);
        len = d.len;
        if (in_umem(off, len, rx_size) && in_umem(off, len, s_dsize[lo])) {
          c_frames += 1;
          c_bytes += len;
          // desc_rules.h chunk_count(off, len), written out: the call reorders the kernel and measured slower
          if (len) nch = ((off & 15) + len + 15) >> 4;
        } else {
          c_skipped += 1;
        }
      }
    }
    uint64_t x = nch;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    pre[wv][lane + 1] = x;
    if (lane == 0) pre[wv][0] = 0;
    off_of[wv][lane] = off;
    dst_of[wv][lane] = dst;
    len_of[wv][lane] = len;
    __builtin_amdgcn_wave_barrier();   // (one wave's LDS accesses complete in order)
    const uint64_t chunks = __shfl(x, 63);

    // The lane's current frame j of the tile: chunks [f_lo, f_hi) of the tile are
    // its chunks, f_first its first chunk's offset, f_end the offset past its last
    // byte.  A lane's chunk numbers only grow, so j only grows.  (From LDS, not
    // by a lane shuffle: the loop's last round leaves lanes inactive, and a
    // shuffle reads nothing from an inactive lane.)
    int j = 0;
    uint64_t f_lo = 0, f_hi = 0, f_first = 0, f_off = 0, f_end = 0, f_dst = 0;
    for (uint64_t k0 = lane; k0 < chunks; k0 += 64ull * kUnroll) {
      uint64_t at[kUnroll];        // the chunk's offset in both UMEMs
      uint64_t to[kUnroll];        // its destination UMEM
      uint32_t b0[kUnroll], b1[kUnroll];   // its bytes inside the frame: [b0, b1) (b1 == 0: no chunk)
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t k = k0 + 64ull * u;
        at[u] = 0; to[u] = 0; b0[u] = 0; b1[u] = 0;
        if (k >= chunks) continue;
        if (k >= f_hi) {
          // the frame whose chunks hold chunk k: pre[j] <= k < pre[j + 1], j above the last one
          int hi = 63;
          while (j < hi) {
            const int mid = (j + hi + 1) >> 1;
            if (pre[wv][mid] <= k) j = mid; else hi = mid - 1;
          }
          f_lo = pre[wv][j];
          f_hi = pre[wv][j + 1];
          f_off = off_of[wv][j];
          f_first = f_off & ~15ull;
          f_end = f_off + len_of[wv][j];
          f_dst = dst_of[wv][j];
        }
        at[u] = f_first + 16 * (k - f_lo);
        to[u] = f_dst;
        b0[u] = at[u] < f_off ? static_cast<uint32_t>(f_off - at[u]) : 0;
        b1[u] = f_end - at[u] < 16 ? static_cast<uint32_t>(f_end - at[u]) : 16;
      }
      uint4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u)
        if (b1[u] - b0[u] == 16) v[u] = *reinterpret_cast<const uint4 *>(rx + at[u]);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (b1[u] - b0[u] == 16)
          store16(reinterpret_cast<uint4 *>(to[u] + at[u]), v[u]);
        else if (b1[u])
          copy_edge(reinterpret_cast<uint8_t *>(to[u] + at[u]), rx + at[u], b0[u], b1[u]);
      }
    }
    __builtin_amdgcn_wave_barrier();   // the tile's LDS rows are rewritten by the next tile
  }

  // one atomic per wave and counter (vector atomics to device memory)
  for (int o = 32; o > 0; o >>= 1) {
    c_frames += __shfl_xor(c_frames, o);
    c_bytes += __shfl_xor(c_bytes, o);
    c_skipped += __shfl_xor(c_skipped, o);
  }
  if (lane == 0) {
    if (c_frames) atomicAdd(&stats[0], c_frames);
    if (c_bytes) atomicAdd(&stats[1], c_bytes);
    if (c_skipped) atomicAdd(&stats[2], c_skipped);
  }
}

}  // namespace forward
}  // namespace xsknf_gpu
