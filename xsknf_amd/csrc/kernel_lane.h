// kernel_lane.h -- the lane-per-frame kernel (small frames).  Part of
// checksummer.hip's one translation unit.
#pragma once
#include "csum_device.h"

namespace xsknf_gpu {


// One lane owns a whole frame: it loads the frame's first NCH 16-byte chunks
// itself, parses the header from its own LDS slot, sums with no cross-lane
// reduction and writes its check from its own registers.  For 64 B frames the
// group kernels spend most of their time on per-frame overhead (descriptor,
// header, reduction for 8 frames per wave step); here a wave step covers 64
// frames.  A wave works through tiles of SPT steps (64 * SPT consecutive frames)
// with the two-buffer unrolled pipeline of the register kernel; the tile's
// descriptors ride in registers, loaded one tile ahead.  Chunks past NCH (frames
// longer than the window) are loaded and summed in a per-lane tail loop.


// Transposed window load (the lane kernel's TL shapes): the NCH chunks of the
// step's 64 frames as NCH instructions whose lanes walk the frames' windows in
// order -- lanes NCH*i .. NCH*i+NCH-1 read frame i's window, one coalesced
// request per frame -- instead of NCH instructions that each send a 16-byte
// request to every frame.  x[p] holds chunk (64 p + lane) % NCH of frame
// (64 p + lane) / NCH; store_lane_tl drops it into that frame's LDS slot.
template <int NCH>
__device__ __forceinline__ void load_lane_tl(const FrameRef &r, uint4 (&x)[NCH]) {
  const int lane = lane_id();
  const uintptr_t cpv = reinterpret_cast<uintptr_t>(r.cp);
#pragma unroll
  for (int p = 0; p < NCH; ++p) {
    const int j = kWave * p + lane;
    const int f = j / NCH, c = j % NCH;
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(f << 2, static_cast<int>(cpv)));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(f << 2, static_cast<int>(cpv >> 32)));
    const int nc = __builtin_amdgcn_ds_bpermute(f << 2, r.nch);
    const uint4 *cp = reinterpret_cast<const uint4 *>((static_cast<uintptr_t>(hi) << 32) | lo);
    x[p] = *XSKNF_GLD(cp + min(c, nc - 1), 16);
  }
}

template <int NCH>
__device__ __forceinline__ void store_lane_tl(uint32_t area, const uint4 (&x)[NCH]) {
  const int lane = lane_id();
#pragma unroll
  for (int p = 0; p < NCH; ++p) {
    const int j = kWave * p + lane;
    lds_store_u128(area + kLaneSlot * (j / NCH) + 16 * (j % NCH), x[p]);
  }
}

// kInSlot: the window is already in the lane's slot (transposed load), v holds a copy
template <int NCH, bool kInSlot = false>
__device__ __forceinline__ LaneOut process_lane(const KernelArgs &args, const FrameRef &r, const uint4 (&v)[NCH],
                                                uint32_t slot) {
  static_assert(NCH >= 4 && NCH <= kHdrChunks, "lane window");
  LaneOut out = {0, false, slot, r.fp};
  if constexpr (!kInSlot) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) lds_store_u128(slot + 16 * k, v[k]);
  }
  const int need = min(kHdrChunks, r.nch);   // header bytes past the window (large ihl)
  for (int k = NCH; k < need; ++k) lds_store_u128(slot + 16 * k, *XSKNF_GLD(r.cp + k, 16));
  compiler_barrier();
  const Header h = parse_header(slot + r.rs);
  compiler_barrier();
  bool do_sum;
  const int32_t verdict = verdict_of(r, h, args.fwd_verdict, do_sum);
  if (!r.exists) return out;
  out.res = verdict;
  if (!do_sum) return out;
  const int lo = r.rs + h.u, hi = r.rs + r.len;
  const uint32_t wl = (lo & 1) ? 0x01000100u : 0x00010001u;
  const uint32_t wh = wl << 8 | wl >> 24;
  uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
  for (int k = 0; k < NCH; ++k) chunk_sum(v[k], 16 * k, lo, hi, wl, wh, acc_lo, acc_hi);
  for (int k = NCH; k < r.nch; ++k) chunk_sum(*XSKNF_GLD(r.cp + k, 16), 16 * k, lo, hi, wl, wh, acc_lo, acc_hi);
  const uint16_t c = check_of(h, acc_lo + (acc_hi << 8), args.payload_mult);
  if (!check_changes(args, h, c)) return out;
  if (static_cast<uint32_t>(r.len) >= args.defer_min_len) {
    out.res = static_cast<int32_t>(make_record(static_cast<uint32_t>(h.u), c));
    return out;
  }
  store_check_inline(args, r, h.u, c, 16 * NCH, slot, out);
  return out;
}

// SW > 4 (one 16-wave block per CU): the block's tiles, every nb-th from the
// block index, are a pool its waves claim from through an LDS counter, one
// tile ahead, as the split kernel's pool (a CU's waves do not stream equally
// fast; from a shared pool the faster ones take more tiles).
// TLM: 0 = every lane loads its own frame's window (load_lane), 1 = transposed
// window loads (load_lane_tl), 2 = per tile: transposed when the tile's frames
// lie apart (a 2 KiB-chunk UMEM, or frames in fill-ring order: one coalesced
// request per frame instead of NCH), per lane when they are packed back to
// back (the -u layout: the lanes' own loads already stream, and the transposed
// path's LDS round trip costs more than it saves).
template <int NCH, int SPT, int SW = kWavesPerBlock, int WPE = 1, int TLM = 0>
__global__ __launch_bounds__(SW * kWave) __attribute__((amdgpu_waves_per_eu(WPE)))
void checksum_kernel_lane(const KernelArgs args) {
  constexpr uint32_t T = SPT * kWave;        // frames per tile
  constexpr bool kPool = SW > kWavesPerBlock;
  __shared__ __attribute__((aligned(16))) uint8_t hdr[SW][kWave][kLaneSlot];
  __shared__ uint32_t pool_next;
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint32_t slot = lds_addr(&hdr[wv][lane][0]);
  const uint32_t waves = gridDim.x * SW;
  const uint32_t last = args.n - 1;
  const uint32_t ntiles = (args.n + T - 1) / T, nb = gridDim.x;
  const uint32_t bt = ntiles > blockIdx.x ? (ntiles - blockIdx.x + nb - 1) / nb : 0u;   // the block's tiles

  uint32_t tile;
  if constexpr (kPool) {
    tile = static_cast<uint32_t>(wv) < bt ? blockIdx.x + wv * nb : kNoTile;
    if (threadIdx.x == 0) pool_next = SW;
    __syncthreads();
  } else {
    tile = blockIdx.x * SW + wv < ntiles ? blockIdx.x * SW + wv : kNoTile;
  }
  const auto desc_at = [&](uint32_t t, int st) {
    return *XSKNF_GLD(reinterpret_cast<const uint4 *>(args.descs + (t == kNoTile ? last : min(t * T + st * kWave + lane, last))), 16);
  };
  uint32_t nrec = 0;
#ifdef XSKNF_TIMELINE
  const unsigned long long tl0 = wall_clock64();
  int tl_tiles = 0;
#endif
  uint4 dn[SPT];
#pragma unroll
  for (int st = 0; st < SPT; ++st) dn[st] = desc_at(tile, st);
  while (tile != kNoTile) {
    const uint32_t tf0 = tile * T;
#ifdef XSKNF_TIMELINE
    ++tl_tiles;
#endif
    uint32_t next;
    if constexpr (kPool) {
      uint32_t dq = 0;
      if (lane == 0) dq = __hip_atomic_fetch_add(&pool_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const uint32_t p = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(dq), 0));
      next = p < bt ? blockIdx.x + p * nb : kNoTile;
    } else {
      next = tile + waves < ntiles ? tile + waves : kNoTile;
    }
    uint4 d[SPT];
#pragma unroll
    for (int st = 0; st < SPT; ++st) {
      d[st] = dn[st];
      dn[st] = desc_at(next, st);
    }
    uint4 v[2][NCH];
    FrameRef r[2];
    r[0] = lane_ref(args, d[0], tf0 + lane);
    bool tl = TLM == 1;
    bool wt = false;   // in-line sectors written through (store_sector16)
    {
      // the tile's first and last frames' offsets: 64 frames packed back to back
      // span a few KiB, 64 chunks of a 2 KiB-chunk UMEM 126 KiB
      const uint64_t off = reinterpret_cast<uintptr_t>(r[0].fp) - reinterpret_cast<uintptr_t>(args.umem);
      const uint64_t o0 = static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<int>(off), 0)) |
                          static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<int>(off >> 32), 0)) << 32;
      const uint64_t o1 = static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<int>(off), kWave - 1)) |
                          static_cast<uint64_t>(__builtin_amdgcn_readlane(static_cast<int>(off >> 32), kWave - 1)) << 32;
      const bool apart = (o1 > o0 ? o1 - o0 : o0 - o1) >= static_cast<uint64_t>(kWave - 1) * 256;
      if constexpr (TLM == 2) tl = apart;
      wt = apart;
    }
    if (tl) load_lane_tl<NCH>(r[0], v[0]); else load_lane<NCH>(r[0], v[0]);
#pragma unroll
    for (int st = 0; st < SPT; ++st) {
      // step st: process buffer st & 1, prefetch step st + 1 into the other
      if (st + 1 < SPT) {
        r[(st + 1) & 1] = lane_ref(args, d[st + 1], tf0 + (st + 1) * kWave + lane);
        if (tl) load_lane_tl<NCH>(r[(st + 1) & 1], v[(st + 1) & 1]);
        else load_lane<NCH>(r[(st + 1) & 1], v[(st + 1) & 1]);
      }
      LaneOut o;
      if (tl) {
        // the step's windows into their frames' slots (the previous step's
        // reads of the slots are done: a wave's LDS operations stay in order),
        // then each lane reads its own frame's back
        compiler_barrier();
        store_lane_tl<NCH>(lds_addr(&hdr[wv][0][0]), v[st & 1]);
        compiler_barrier();
        uint4 own[NCH];
#pragma unroll
        for (int k = 0; k < NCH; ++k) own[k] = lds_u128(slot + 16 * k);
        o = process_lane<NCH, true>(args, r[st & 1], own, slot);
      } else {
        o = process_lane<NCH>(args, r[st & 1], v[st & 1], slot);
      }
      store_sectors(o, lane, args.plain_sector, wt);
      const uint32_t f = tf0 + st * kWave + lane;
      nrec += store_result(args, f, f < args.n, o.res);
      compiler_barrier();   // the next frame rewrites this lane's header window
    }
    tile = next;
  }
#ifdef XSKNF_TIMELINE
  // stream done (last store issued), then its stores acknowledged
  const unsigned long long tl1 = wall_clock64();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  timeline_put(blockIdx.x * SW + wv, lane, tl0, tl1, tl_tiles, 0, 0, 0);
#endif
  publish_records(args, nrec, lane);
}

}  // namespace xsknf_gpu
