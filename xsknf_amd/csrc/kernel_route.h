// kernel_route.h -- the kernels of the device-side router (route_device.hip):
// the second half of process_batch / process_batch_1if (src/xsknf.c:503-522,
// :654-672) for a batch whose verdicts lie in device memory -- a stable
// partition of the frames into one tx list per interface and the fill list of
// the dropped frames, what route_host.cpp computes on one CPU thread.
//
// A frame's bin is its interface (0 .. nif - 1) or the drop bin (nif): at most
// kMaxBins = 33.  Three stream-ordered passes, so that NO block ever waits on
// another block (no look-back, no grid barrier, no flag), and no order depends
// on an atomic (there is none): the lists come out the same every time.
//   1. route_tile_counts: every block counts its tile's frames per bin;
//   2. route_scan_counts: one block per bin turns that bin's tile counts into
//      exclusive prefixes and writes the bin's total into the header;
//   3. route_scatter: every block re-reads its tile's verdicts, reads its
//      descriptors, ranks its frames and writes the lists.
//
// A tile is kTile frames, a contiguous run of kWaveFrames per wave, taken in
// kPerThread rounds of one frame per lane: (wave, round, lane) order is frame
// order, so a frame's place in its bin is
//   the bin's base + its tile's prefix + the earlier waves' frames of the bin
//   + its rank in its wave,
// the last from a ballot per distinct bin of the round (wave_rank).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/xsknf_gpu.h"
#include "block_scan.h"

namespace xsknf_gpu {
namespace route {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kTile = kThreads * kPerThread;    // frames per block
constexpr uint32_t kWaveFrames = 64 * kPerThread;    // a wave's contiguous run of its tile
constexpr uint32_t kMaxBins = XSKNF_GPU_ROUTE_MAX_INTERFACES + 1;
constexpr uint32_t kNoBin = 63;                      // a lane past the batch's end: in no bin
constexpr uint32_t kBinBits = 6;                     // bin | rank << kBinBits (rank < kWaveFrames)
static_assert(scan::kThreads == kThreads, "block_incl_scan scans a block of kThreads");
static_assert(kMaxBins <= kNoBin && kNoBin < (1u << kBinBits) && kMaxBins <= 64, "a bin per lane, kNoBin is none");

// The workspace: kHeaderWords u64 (the counts: one per interface, then the
// drops; what the host reads back), then nbins x nb u32 tile counts, bin-major
// (bin b's nb tiles in a row: one block scans them in place).
constexpr uint32_t kHeaderWords = kMaxBins + 1;      // (even: the u32 counts start 16-byte aligned)

// The bin of a verdict.  One interface: process_batch_1if's rule (-1 drops,
// anything else is the one tx queue).  Several: dispose_multi's (a verdict that
// names no interface drops).
__device__ inline uint32_t bin_of(int32_t v, uint32_t nif) {
  if (nif == 1) return v == -1 ? 1u : 0u;
  return v < 0 || static_cast<uint32_t>(v) >= nif ? nif : static_cast<uint32_t>(v);
}

// One round of a wave: the number of lower lanes of the wave (this round) plus
// of earlier rounds that hold this lane's bin.  `run` is the wave's count of
// bin l so far, kept by lane l.  One ballot per DISTINCT bin of the round;
// `todo` is a ballot, the same in every lane, so every lane of the wave stays in
// the loop to its last round and each ballot sees the whole wave (a lane past
// the batch's end carries kNoBin and matches nothing).
__device__ inline uint32_t wave_rank(uint32_t bin, int lane, uint32_t &run) {
  uint32_t rank = 0;
  uint64_t todo = __ballot(bin != kNoBin);
  while (todo) {
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll(static_cast<long long>(todo)) - 1);
    const uint32_t b = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bin), leader));
    const uint64_t m = __ballot(bin == b);
    const uint32_t before = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(run), static_cast<int>(b)));
    if (bin == b) rank = before + __popcll(m & ((1ull << lane) - 1));
    if (lane == static_cast<int>(b)) run += __popcll(m);
    todo &= ~m;
  }
  return rank;
}

// Pass 1: cnt[b * nb + tile] = the tile's frames in bin b.
__global__ void __launch_bounds__(kThreads) route_tile_counts(const int32_t *verdicts, uint32_t n, uint32_t nif,
                                                              uint64_t nb, uint32_t *cnt) {
  __shared__ uint32_t wtot[kWaves][kMaxBins];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile + wv * kWaveFrames + lane;
  int32_t v[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * 64;
    v[j] = f < n ? verdicts[f] : 0;
  }
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * 64;
    wave_rank(f < n ? bin_of(v[j], nif) : kNoBin, lane, run);
  }
  if (lane < static_cast<int>(kMaxBins)) wtot[wv][lane] = run;
  __syncthreads();
  if (threadIdx.x <= nif) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += wtot[w][threadIdx.x];
    cnt[threadIdx.x * nb + blockIdx.x] = t;
  }
}

// Pass 2, block b: bin b's tile counts become exclusive prefixes in place; its
// total is the header's count b.
__global__ void __launch_bounds__(kThreads) route_scan_counts(uint32_t *cnt, uint64_t nb, uint64_t *hdr) {
  __shared__ uint64_t wtot[kWaves];
  uint32_t *arr = cnt + blockIdx.x * nb;
  uint64_t carry = 0;
  for (uint64_t i0 = 0; i0 < nb; i0 += kThreads) {
    const uint64_t i = i0 + threadIdx.x;
    const uint64_t c = i < nb ? arr[i] : 0;
    uint64_t tot;
    const uint64_t incl = scan::block_incl_scan(c, wtot, &tot);
    if (i < nb) arr[i] = static_cast<uint32_t>(carry + incl - c);
    carry += tot;
  }
  if (threadIdx.x == 0) hdr[blockIdx.x] = carry;
}

// Pass 3: the lists.  A frame's place o counts in `order`'s space: the tx lists
// one after another (interface i from base_i = the counts before it), then the
// drops from ntx.  tx_descs[o] = {addr, len, 0} for a tx frame, fill_addrs[o -
// ntx] = addr for a drop, order[o] = the frame.  (o < n whenever the verdicts
// are the ones pass 1 counted; the test keeps a caller who rewrites them under
// the passes from writing outside the lists.)
__global__ void __launch_bounds__(kThreads) route_scatter(const uint4 *descs, const int32_t *verdicts, uint32_t n,
                                                          uint32_t nif, uint64_t nb, const uint64_t *hdr,
                                                          const uint32_t *cnt, uint4 *tx_descs, uint64_t *fill_addrs,
                                                          uint32_t *order) {
  __shared__ uint32_t wtot[kWaves][kMaxBins], woff[kWaves][kMaxBins];
  __shared__ uint32_t s_ntx;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kTile + wv * kWaveFrames + lane;
  int32_t v[kPerThread];
  uint4 d[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * 64;
    v[j] = f < n ? verdicts[f] : 0;
    d[j] = f < n ? descs[f] : make_uint4(0, 0, 0, 0);
  }
  uint32_t run = 0, place[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint64_t f = base + j * 64;
    const uint32_t bin = f < n ? bin_of(v[j], nif) : kNoBin;
    place[j] = bin | wave_rank(bin, lane, run) << kBinBits;
  }
  if (lane < static_cast<int>(kMaxBins)) wtot[wv][lane] = run;
  __syncthreads();
  if (threadIdx.x <= nif) {
    const uint32_t b = threadIdx.x;
    uint32_t at = 0;                       // the frames of the bins before b: base_b, or ntx for the drops
    for (uint32_t i = 0; i < b; ++i) at += static_cast<uint32_t>(hdr[i]);
    if (b == nif) s_ntx = at;
    at += cnt[b * nb + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      woff[w][b] = at;
      at += wtot[w][b];
    }
  }
  __syncthreads();
  const uint32_t ntx = s_ntx;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const uint32_t bin = place[j] & ((1u << kBinBits) - 1);
    if (bin == kNoBin) continue;
    const uint32_t o = woff[wv][bin] + (place[j] >> kBinBits);
    if (o >= n) continue;
    if (bin < nif) {
      tx_descs[o] = make_uint4(d[j].x, d[j].y, d[j].z, 0);
    } else {
      if (o < ntx) continue;
      fill_addrs[o - ntx] = static_cast<uint64_t>(d[j].x) | static_cast<uint64_t>(d[j].y) << 32;
    }
    if (order) order[o] = static_cast<uint32_t>(base + j * 64);
  }
}

}  // namespace route
}  // namespace xsknf_gpu
