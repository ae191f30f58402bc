// kernel_split.h -- the split kernel: headers by lane, payload by group (the
// default for frames > 128 B).  Part of checksummer.hip's one translation unit.
#pragma once
#include "csum_device.h"

namespace xsknf_gpu {


// The group kernels pay a frame's fixed work (descriptor, header parse, verdict,
// check store) once per GROUP: LPF lanes redo it, and a short frame leaves most
// of its group idle.  With a mix of lengths (IMIX) or medium frames (570 B)
// that overhead, not HBM, sets the time.  Here a wave takes a tile of 64
// consecutive frames in three phases:
//  A. lane l owns frame l: it loads the frame's first W chunks (the header
//     window), parses the header in its LDS slot, sums the window and, when the
//     frame fits the window, finishes it exactly as the lane kernel does;
//  B. the payload of the longer frames past the window is cut into ITEMS of one
//     group pass (LPF lanes x NCH chunks) and the items are dealt to the wave's
//     groups round robin, so the groups stay balanced whatever the mix; item
//     sums meet in a per-frame LDS accumulator (ds_add);
//  C. lane l folds its frame's total and stores the check (2 bytes in-line, or
//     a record for the scatter pass).
// The item list reuses the lane slots (dead after phase A).  Frames with more
// items than a slot share holds take a whole-wave loop (correctness path).

__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, int lane, uint32_t &total) {
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t y = static_cast<uint32_t>(__shfl_up(static_cast<int>(x), o, kWave));
    if (lane >= o) x += y;
  }
  total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(x), kWave - 1));
  return x - v;
}

__device__ __forceinline__ void lds_add_u32(uint32_t a, uint32_t v) {
  __hip_atomic_fetch_add(reinterpret_cast<__attribute__((address_space(3))) uint32_t *>(static_cast<uintptr_t>(a)),
                         v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void lds_store_u16(uint32_t a, uint16_t v) {
  *reinterpret_cast<__attribute__((address_space(3))) uint16_t *>(static_cast<uintptr_t>(a)) = v;
}

__device__ __forceinline__ uint32_t lds_u16(uint32_t a) {
  return *reinterpret_cast<const __attribute__((address_space(3))) uint16_t *>(static_cast<uintptr_t>(a));
}

__device__ __forceinline__ uint32_t lds_byte(uint32_t a) {
  return *reinterpret_cast<const lds_u8 *>(static_cast<uintptr_t>(a));
}

// Frame bytes rebuilt from integers (LDS) must be marked global, or hipcc
// emits FLAT loads, which count in lgkmcnt too and serialize every LDS read
// behind the loads in flight.
typedef const __attribute__((address_space(1))) u32x4 *gchunk_ptr;

__device__ __forceinline__ uint4 load_nt(gchunk_ptr p XSKNF_SITE) {
#ifdef XSKNF_GUARD
  p = guard_ld(p, 16, site);
#endif
  const u32x4 x = __builtin_nontemporal_load(p);
  return make_uint4(x.x, x.y, x.z, x.w);
}

// A payload frame as phase B sees it: {fp lo, fp hi, len, u} in LDS.
struct Payload {
  gchunk_ptr cp;
  int nch, lo, hi;
  uint32_t wl, wh;
};

__device__ __forceinline__ Payload payload_of(uint4 m) {
  Payload p;
  const uintptr_t fp = (static_cast<uintptr_t>(m.y) << 32) | m.x;
  const int rs = static_cast<int>(fp & 15);
  p.cp = reinterpret_cast<gchunk_ptr>(fp - rs);
  p.nch = static_cast<int>((static_cast<uint64_t>(rs) + m.z + 15) >> 4);
  p.lo = rs + static_cast<int>(m.w);
  p.hi = rs + static_cast<int>(m.z);
  p.wl = (p.lo & 1) ? 0x01000100u : 0x00010001u;
  p.wh = p.wl << 8 | p.wl >> 24;
  return p;
}

// Phase B's loads are issued from inline asm with explicitly counted waits:
// hipcc drains vmcnt to 0 at the top of any loop whose loads are consumed in a
// later iteration, which would serialize the two-stage pipeline.  Each loaded
// register is bound to its wait (an empty asm with a "+v" operand after the
// s_waitcnt), so no use can move above the wait, and a stage that is never
// consumed is drained before its registers can be reused.
__device__ __forceinline__ u32x4 gload_nt_asm(gchunk_ptr p XSKNF_SITE) {
#ifdef XSKNF_GUARD
  p = guard_ld(p, 16, site);
#endif
  u32x4 x;   // nt: default-policy loads measured 1500 B 296 -> 344 us per step
  asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(x) : "v"(p) : "memory");
  return x;
}

// One stage of phase B: U items per group, NCH chunks per lane each.
template <int U, int NCH>
struct ItemStage {
  u32x4 t[U][NCH];
  Payload pl[U];
  uint32_t fi[U];
  int c0[U];
  bool ok[U];

  template <int W, int LPF, int SPAN>
  __device__ __forceinline__ void issue(uint32_t area, uint32_t mt, uint32_t it0, uint32_t total, int grp, int gl) {
    constexpr int G = kWave / LPF;
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const uint32_t it = it0 + q * G + grp;
      ok[q] = it < total;
      const uint32_t e = lds_u16(area + 2 * min(it, total - 1));
      fi[q] = e >> 8;
      pl[q] = payload_of(lds_u128(mt + 16 * fi[q]));
      c0[q] = W + static_cast<int>(e & 0xff) * SPAN;
      if (!ok[q]) pl[q].hi = pl[q].lo;   // masked: sums nothing
    }
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int k = 0; k < NCH; ++k) t[q][k] = gload_nt_asm(pl[q].cp + min(c0[q] + k * LPF + gl, pl[q].nch - 1));
  }

  // wait until at most N vector-memory operations younger than this stage's are outstanding
  template <int N>
  __device__ __forceinline__ void wait() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits on gfx950");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int k = 0; k < NCH; ++k) asm volatile("" : "+v"(t[q][k]));
  }

  template <int LPF>
  __device__ __forceinline__ void consume(uint32_t ab, int gl) {
    wait<U * NCH>();   // the other stage's loads stay in flight
#pragma unroll
    for (int q = 0; q < U; ++q) {
      uint32_t blo = 0, bhi = 0;
#pragma unroll
      for (int k = 0; k < NCH; ++k) {
        const uint4 v = make_uint4(t[q][k].x, t[q][k].y, t[q][k].z, t[q][k].w);
        chunk_sum_fast(v, (c0[q] + k * LPF + gl) * 16, pl[q].lo, pl[q].hi, pl[q].wl, pl[q].wh, blo, bhi);
      }
      const uint32_t P = group_sum_last<LPF>(blo + (bhi << 8));
      if (gl == LPF - 1 && ok[q]) lds_add_u32(ab + 4 * fi[q], P);
    }
  }
};


// The patch list: where the default shape (W = 8, two items in flight: 157
// VGPRs, 3 waves per SIMD, so 3 blocks per CU) has LDS to spare, a deferred
// check is not parked in `verdicts` but kept in the wave's LDS list, one
// 8-byte entry per frame for its first kPatchTiles tiles: the check's 64-byte
// sector as an index from the 64-byte-aligned UMEM base, and {valid, whole
// sector, byte of the check in the sector, the check}.  The frame's final
// verdict is stored in the tile's one verdict store, and the wave's patches
// read neither records nor descriptors back: one round trip (the sectors)
// instead of three.  launch_split sizes the grid so that no wave has more
// tiles than its list (the code for tiles past it -- checks in-line -- is kept
// as a fallback).  Past the list, checks were first parked as records in
// `verdicts` for the wave to patch after its list (three round trips), then
// written in-line; launches past their lists faulted with an illegal address
// three times in full GPU suites, twice with the records and once in-line,
// never alone or under the guard build.
constexpr int kPatchTiles = 6;   // 6 x 64 x 8 B x 4 waves = 12 KiB per block
constexpr int kPatchT = 2;       // tiles whose sectors are in flight together (3, 4: no gain, r02 ab_tail2, r04)
// (the entry's flags and patch_entry, which makes one: csum_device.h)

// Tiles in a wave's patch list: 16 x 2 items fit 3 waves per SIMD (6 tiles per
// wave at 1M frames; 7 with the pool, whose faster waves take more units), 16 x
// 3 fit 2 (8 tiles per wave); the other shapes keep no list.  A block of more
// than 4 waves holds a whole CU's waves and shares the CU's tiles as a pool.
// (Round 4's compact shape -- 4 waves per SIMD, phase-B scratch in the dead
// window slots, 4-tile lists -- and its 16-wave static twin tied the default
// and were removed in round 5: DESIGN 7.)
constexpr bool pooled_split(int sw) { return sw > kWavesPerBlock; }
// The parts each of a pool block's last tiles runs as: halves up to 4 KiB,
// quarters for jumbo (W = 4; halves 1469.5-1470.7, eighths 1471.1-1471.5 vs
// 1459.2-1461.0 us, NIC +10..14 us -- profiles/r05/ab/ab_jumbo_parts_r05jp.jsonl),
// and how many: the last SW tiles, the last 3 SW for jumbo (2 SW with 16-unit
// lists: 1445.2-1445.7 vs 1447.9-1448.8 us and 1455.4-1456.3 vs 1456.4-1459.2
// on a second box, NIC -1..-2, ab_jumbo_split_tiles_r05jk.jsonl; 3 SW with
// 20-unit lists: NIC -3.5..-4 us on two boxes, worst case -0.5..-1.7,
// ab_jumbo_units20_r05j20.jsonl; as many as the lists hold, leaving the waves
// no slack to balance: +50 us).
constexpr uint32_t pool_parts(int w) { return w == 4 ? 4u : 2u; }
// Tiles split at the end of a pool block of SW waves (the last 8 or 16 tiles
// halved instead of 12 at 1500 B: 276.5-277.5 and 277.5-278.5 vs 277.3-278.3
// us, NIC +0.5..1 -- profiles/r05/ab/ab_halves_tiles_*).
constexpr uint32_t pool_split_tiles(int w, int sw) { return w == 4 ? 3u * sw : static_cast<uint32_t>(sw); }
// The most tiles one pool block may hold so that its units fit its waves'
// patch lists (SW x PT entries): bt tiles, the last pool_split_tiles of them in
// pool_parts units each, are bt + (parts - 1) x split units.  launch_split sizes
// the grid by it and the kernel asserts the same count, so the two cannot drift.
constexpr uint32_t pool_block_tiles_max(int w, int sw, int pt) {
  return static_cast<uint32_t>(sw * pt) - (pool_parts(w) - 1) * pool_split_tiles(w, sw);
}

// Pool guard: a pooled wave whose patch list is full claims no more units, so
// a grid too small for the batch would leave units unclaimed (their frames
// unsummed).  launch_split's bound makes that unreachable; should it ever be
// reached, each block with more units than its waves' lists hold counts here
// at its start, and each wave that waits in vain for a unit's mark in the
// patch queue counts too (xsknf_gpu_pool_guard_trips reads it).
__device__ unsigned int g_pool_guard_trips;

// The pooled jumbo shape (W = 4, 16 x 3 items, one 8-wave block per CU) keeps
// a 20-unit list (80 KiB of its block's 151 KiB; 16 units until the late
// round-5 A/B above): with every check deferred
// (fused_stores 2 + 16) the block's queue patches them in the launch instead of
// a scatter_checks pass (round 5: 9000 B 1448.4-1449.3 vs 1455.9-1457.9 us and
// 1457.2-1458.1 vs 1461.6-1462.9 on a second box, NIC checks -4 us;
// profiles/r05/ab/).
constexpr int kJumboPatchUnits = 20;
template <int W, int NCH, int U, bool kPool>
constexpr int patch_list_tiles() {
  if constexpr (W == 4 && NCH == 3 && U >= 2 && kPool) return kJumboPatchUnits;
  return (W == 8 && U >= 2) ? (NCH == 2 ? (kPool ? 7 : kPatchTiles) : 8) : 0;
}


typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void lds_store_u64(uint32_t a, uint2 v) {
  const u32x2 x = {v.x, v.y};
  *reinterpret_cast<__attribute__((address_space(3))) u32x2 *>(static_cast<uintptr_t>(a)) = x;
}

__device__ __forceinline__ uint2 lds_u64(uint32_t a) {
  const u32x2 x = *reinterpret_cast<const __attribute__((address_space(3))) u32x2 *>(static_cast<uintptr_t>(a));
  return make_uint2(x.x, x.y);
}

// The wave's patch list (ntiles tiles of 64 entries at LDS `pl`): 16 frames per
// round, 4 lanes per frame, each frame's sector read and rewritten whole (one
// non-temporal 64-byte store of 4 lanes), or its 2 check bytes where the sector
// leaves the frame.  kPatchT tiles' sectors are in flight together.
__device__ __forceinline__ void tail_patch_list(const KernelArgs &args, uint32_t pl, int ntiles, int lane) {
  const int piece = lane & 3;
  uint8_t *const base = args.umem - (reinterpret_cast<uintptr_t>(args.umem) & 63);   // keeps global addressing
  constexpr int T = kPatchT;
  for (int t0 = 0; t0 < ntiles; t0 += T) {
    uint4 v[T][4];
    uint8_t *mine[T][4];
    uint32_t info[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint2 e = t0 + t < ntiles ? lds_u64(pl + 8 * ((t0 + t) * kWave + 16 * k + (lane >> 2))) : make_uint2(0, 0);
        info[t][k] = e.y;
        uint8_t *sec = base + (static_cast<uint64_t>(e.x) << 6);
        const bool whole = (e.y & (kPatchValid | kPatchWhole)) == (kPatchValid | kPatchWhole);
        mine[t][k] = whole ? sec + 16 * piece : sec + ((e.y >> 16) & 63);
        if (whole)
          v[t][k] = load_nt(reinterpret_cast<const uint4 *>(mine[t][k]));
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t c = info[t][k] & 0xffffu;
        if ((info[t][k] & (kPatchValid | kPatchWhole)) == (kPatchValid | kPatchWhole)) {
          const int o = static_cast<int>((info[t][k] >> 16) & 63) - 16 * piece;
          uint4 w = put_byte(v[t][k], o, c);
          w = put_byte(w, o + 1, c >> 8);
          store_nt16(mine[t][k], w);   // plain (write-back) stores: 1500 B +20 us, IMIX +8 (r02 ab_tail2)
        } else if ((info[t][k] & kPatchValid) && piece == 0) {
          XSKNF_GST(mine[t][k], 2) {
            mine[t][k][0] = static_cast<uint8_t>(c);
            mine[t][k][1] = static_cast<uint8_t>(c >> 8);
          }
        }
      }
    }
  }
}


// One item per group in flight (U = 1) fits 4 waves per SIMD (<= 128 VGPRs),
// which the LDS footprint also allows (4 blocks per CU): measured IMIX / 570 B
// +8-11 % from 2 -> 3 waves per SIMD, so the register budget is pinned.
template <int W, int LPF, int NCH, int U, bool TL, int SW>
__global__ __launch_bounds__(SW * kWave) __attribute__((amdgpu_waves_per_eu(U == 1 ? 4 : 1)))
void checksum_kernel_split(const KernelArgs args) {
  static_assert(W >= 4 && (W <= kHdrChunks || W == 8), "header window");
  static_assert(!TL || W == 4 || W == 8, "transposed window load: W lanes x 16 B per frame");
  static_assert(kWave % LPF == 0 && LPF >= 4, "group shape");
  constexpr int G = kWave / LPF;
  constexpr int SPAN = LPF * NCH;                          // chunks per item
  constexpr int kSlot = 16 * W > kLaneSlot ? 16 * W : kLaneSlot;   // per-lane header window
  constexpr int kSlotArea = kWave * kSlot;                 // bytes per wave
  constexpr int kItemCap = 256;                            // items per round of phase B
  constexpr uint32_t kItemsPerFrame = 255;                 // u8 pass index; more: whole-wave loop
  constexpr bool kPool = pooled_split(SW);   // one block per CU: its waves share the CU's tiles
  __shared__ __attribute__((aligned(16))) uint8_t slots[SW][kSlotArea];
  __shared__ __attribute__((aligned(16))) uint16_t itemq[SW][kItemCap];
  __shared__ __attribute__((aligned(16))) uint4 meta[SW][kWave];
  __shared__ __attribute__((aligned(16))) uint32_t accb[SW][kWave];
  // (jumbo's list: each wave patching its own list after its last unit tied the scatter
  // pass, 1463 vs 1461 us -- profiles/r02/ab_jumbo_tail.jsonl; from the block's queue it is ahead)
  constexpr int PT = patch_list_tiles<W, NCH, U, kPool>();
  __shared__ __attribute__((aligned(16))) uint2 plist[SW][PT > 0 ? PT * kWave : 1];

  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int grp = lane / LPF, gl = lane % LPF;
  const uint32_t area = lds_addr(&slots[wv][0]);
  const uint32_t slot = area + kSlot * lane;
  const uint32_t mt = lds_addr(&meta[wv][0]);
  const uint32_t ab = lds_addr(&accb[wv][0]);
  const uint32_t iq = lds_addr(&itemq[wv][0]);
  const uint32_t waves = gridDim.x * SW;
  const uint32_t last = args.n - 1;
// Streaming waves issue ahead of patching ones: priority 1 until the wave's
// last unit, 0 for its patches (with the patch queue below: 1500 B -0.9..-1.5
// us, its NIC traffic -3 us, other sizes level -- profiles/r04/ab/ab_patch_prio_*)
  __builtin_amdgcn_s_setprio(1);

  uint32_t nrec = 0;
#ifdef XSKNF_TIMELINE
  const unsigned long long tl0 = wall_clock64();
  unsigned long long tl_a = 0, tl_p = 0, tl_b = 0, tl_t = 0;
#define XSKNF_TL_MARK(acc) do { const unsigned long long n_ = wall_clock64(); acc += n_ - tl_t; tl_t = n_; } while (0)
#define XSKNF_TL_START() do { tl_t = wall_clock64(); } while (0)
#else
#define XSKNF_TL_START() do { } while (0)
#define XSKNF_TL_MARK(acc) do { } while (0)
#endif
  const uint32_t pl = lds_addr(&plist[wv][0]);
  const bool list_ok = PT > 0 && args.tail_scatter && args.umem_size < kPatchMaxUmem;
  int it = 0;              // tiles done by this wave
  bool any_entry = false;  // wave-uniform: the patch list holds an entry
  // The wave's tiles: `tile`, then `tn`, `tnn` (kNoTile: none).
  // * SW = 4 (several blocks per CU): every waves-th tile from the wave's index,
  //   descriptors two tiles ahead.
  // * kPool (one block holds every wave of its CU: SW = 12, or 8 for jumbo):
  //   the block's tiles, every nb-th from the block index, are a pool of units
  //   its waves draw from -- the first by wave index, each later one claimed
  //   through an LDS counter when the wave starts a unit, its descriptors
  //   loaded while that unit streams.  A CU's waves do not stream equally fast
  //   (three 4-wave blocks per CU: the third block's waves ended their streams
  //   ~40 us after the first two's at 1500 B, tools/timeline.py), and from a
  //   shared pool the faster ones take more units.  A unit past the wave's
  //   patch list writes its checks in-line.  (Per-XCD global counters were
  //   tried: a device-scope atomic retires in vmcnt order, and each round trip
  //   held up the next load wait -- 1500 B 347 vs 291 us.)
  const uint32_t ntiles = (args.n + kWave - 1) / kWave;
  __shared__ uint32_t pool_next;
  const uint32_t nb = gridDim.x;
  const uint32_t bt = ntiles > blockIdx.x ? (ntiles - blockIdx.x + nb - 1) / nb : 0u;   // the block's tiles
  const auto tile_of = [&](uint32_t k) { return blockIdx.x + k * nb; };
  // The pool's units: the block's tiles, except that its last SW tiles (2 SW
  // for jumbo) run as kParts parts each, so the waves' streams end closer together: halves up to
  // 4 KiB (quarters there: 570 B 165 vs 151 us, 1024 B 213 vs 205 --
  // profiles/r02/ab_pool.jsonl), quarters for jumbo tiles (W = 4), which
  // stream for ~160 us each.  (Whole tiles only: IMIX level, 1500 B +6-7 us;
  // profiles/r04/ab/ab_pool_no_halves*.)
  constexpr uint32_t kParts = pool_parts(W);
  const uint32_t nsplit = kPool ? min(bt, pool_split_tiles(W, SW)) : 0u;
  const uint32_t nfull = bt - nsplit;
  const uint32_t units = nfull + kParts * nsplit;
  const auto pool_unit = [&](uint32_t p) { return p < units ? p : kNoTile; };
  // first frame and frame count of unit / static tile u
  const auto unit_f0 = [&](uint32_t u) -> uint32_t {
    if constexpr (kPool) {
      if (u < nfull) return tile_of(u) * kWave;
      const uint32_t h = u - nfull;
      return tile_of(nfull + h / kParts) * kWave + (h % kParts) * (kWave / kParts);
    } else {
      return u * kWave;
    }
  };
  const auto unit_cnt = [&](uint32_t u) -> uint32_t { return kPool && u >= nfull ? kWave / kParts : kWave; };
  bool pool_live = kPool;   // wave-uniform: no failed dequeue yet
  uint32_t tile, tn, tnn;   // pool units (kPool) or tiles
  if constexpr (kPool) {
    // a wave holds at most the unit it sums and the next (claimed three ahead,
    // the waves of a block ended 43 us apart at 1500 B: 284.5 vs 279.2 us;
    // claimed when the unit's payload starts rather than at its start: 1500 B a
    // tie, 570 B 149.1 vs 146.7, IMIX 118.5 vs 115.9 -- profiles/r02/ab_pool.jsonl)
    tile = pool_unit(wv);
    tn = tnn = kNoTile;
    if (threadIdx.x == 0) pool_next = SW;
    __syncthreads();
  } else {
    const uint32_t t0 = blockIdx.x * SW + wv;
    tile = t0 < ntiles ? t0 : kNoTile;
    tn = t0 + waves < ntiles ? t0 + waves : kNoTile;
    tnn = t0 + 2 * waves < ntiles ? t0 + 2 * waves : kNoTile;
  }
  // One patch queue per block (the pooled shapes) instead of each wave patching its own list
  // after its last unit: a wave publishes each finished unit's list (its index,
  // or a null mark for a unit with nothing to patch), and a wave whose stream
  // is done takes the next published unit of ANY wave of the block, so the
  // block's last stream is followed by one unit's patches, not by its wave's
  // whole list.  Every wave publishes one mark per unit; the block's count of
  // units is known, so the consumers' loop ends; the wait for a mark is bounded
  // by the clock.  Measured alone: 1500 B -0.8..-1.5 us, the launch still ends
  // ~7 us after its last stream (profiles/r04/ab/ab_patch_queue_*); with the
  // streaming waves' priority the product's since round 4.  The static 4-wave
  // blocks (IMIX) keep each wave patching its own list (a queue there: IMIX +1
  // us, profiles/r04/ab/ab_patch_queue_static_bench.jsonl).
  constexpr bool kShared = PT > 0 && kPool;
  constexpr uint32_t kPQ = kShared ? SW * PT : 1;   // marks: the grid is sized so a block has <= SW * PT units
  constexpr uint32_t kPQNull = 0xffffu;
  static_assert(!kShared || pool_block_tiles_max(W, SW, PT) + (pool_parts(W) - 1) * pool_split_tiles(W, SW) == kPQ,
                "a pool block at launch_split's tile bound has exactly as many units as its lists hold");
  __shared__ uint32_t pq_tail, pq_head;
  __shared__ uint32_t pq[kPQ];
  const bool shared_on = kShared && list_ok;   // block-uniform
  bool pq_full = false;                        // wave-uniform: a mark found no room
  uint32_t block_units = 0;
  if constexpr (kShared) {
    block_units = units;
    // more units than the waves' lists hold: the waves stop claiming once their
    // lists are full, so units are left unclaimed (never, by launch_split's bound;
    // the same count the marks below would wait for in vain)
    if (threadIdx.x == 0 && shared_on && units > kPQ)
      __hip_atomic_fetch_add(&g_pool_guard_trips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) pq_tail = pq_head = 0;
    for (uint32_t i = threadIdx.x; i < kPQ; i += SW * kWave) pq[i] = 0;
    __syncthreads();
  }
  const auto desc_of = [&](uint32_t t) {
    return *XSKNF_GLD(reinterpret_cast<const uint4 *>(args.descs + (t == kNoTile ? last : min(unit_f0(t) + lane, last))), 16);
  };
  // descriptors travel two tiles ahead (static), one unit ahead (kPool)
  uint4 d = desc_of(tile);
  uint4 dn = kPool ? d : desc_of(tn);
  while (tile != kNoTile) {
    XSKNF_TL_START();
    if constexpr (kPool) {   // claim the next unit, and load its descriptors while this one streams
      uint32_t dq = 0;
      // a wave whose patch list is full claims no more: launch_split sizes the
      // grid so that the lists of a block's waves hold all of its units
      if (list_ok && it + 1 >= PT) pool_live = false;
      if (pool_live && lane == 0) dq = __hip_atomic_fetch_add(&pool_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      tn = pool_live ? pool_unit(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(dq), 0))) : kNoTile;
      pool_live = tn != kNoTile;
      dn = desc_of(tn);
    }

    const uint32_t f0 = unit_f0(tile), cnt = unit_cnt(tile);
    const uint32_t f = lane < cnt ? f0 + lane : args.n;   // lanes past a half unit hold no frame
    const FrameRef r = lane_ref(args, d, f);
    uint4 v[W];
    if constexpr (TL) {
      // transposed: lanes W*i .. W*i+W-1 load the window of frame (64/W)*p + i
      // (p = 0..W-1), one coalesced 16*W-byte request per frame instead of W
      // 16-byte ones, and drop it in that frame's slot
      constexpr int FPI = kWave / W;   // frames per load instruction
      const uintptr_t cpv = reinterpret_cast<uintptr_t>(r.cp);
      u32x4 x[W];
#pragma unroll
      for (int p = 0; p < W; ++p) {
        const int g = FPI * p + lane / W;
        const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(g << 2, static_cast<int>(cpv)));
        const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(g << 2, static_cast<int>(cpv >> 32)));
        const int nc = __builtin_amdgcn_ds_bpermute(g << 2, r.nch);
        const gchunk_ptr cp = reinterpret_cast<gchunk_ptr>((static_cast<uintptr_t>(hi) << 32) | lo);
        x[p] = *XSKNF_GLD(cp + min(lane % W, nc - 1), 16);   // default policy: nt measured 64 B 39 -> 55 us, 1500 B 292 -> 308
      }
      compiler_barrier();
#pragma unroll
      for (int p = 0; p < W; ++p)
        lds_store_u128(area + kSlot * (FPI * p + lane / W) + 16 * (lane % W), make_uint4(x[p].x, x[p].y, x[p].z, x[p].w));
      compiler_barrier();
#pragma unroll
      for (int k = 0; k < W; ++k) v[k] = lds_u128(slot + 16 * k);
    } else {
      load_lane<W>(r, v);
    }
    XSKNF_TL_MARK(tl_a);
    const uint4 dnn = kPool ? d : desc_of(tnn);
    const bool to_list = list_ok && it < PT;   // wave-uniform
    // per-tile store policy, as the register kernel: long frames defer their
    // checks only where they are at least half of the tile
    // (a wave's tiles past its patch list: in-line)
    uint32_t defer_min = args.tail_scatter && !to_list ? kNoDefer : args.defer_min_len;
    if (defer_min != kNoDefer && defer_min != 0 && !args.no_scatter) {
      const uint32_t nlong = static_cast<uint32_t>(__builtin_popcountll(
          __builtin_amdgcn_ballot_w64(f < args.n && d.z >= defer_min)));
      const uint32_t nlive = f0 < args.n ? min(cnt, args.n - f0) : 0u;
      if (kDeferTileK * nlong < nlive) defer_min = kNoDefer;
    }

    // ---- phase A: header, window sum, short frames finished ----
    compiler_barrier();
    if constexpr (!TL) {
#pragma unroll
      for (int k = 0; k < W; ++k) lds_store_u128(slot + 16 * k, v[k]);
    }
    compiler_barrier();
    {  // header bytes past the window (large ihl, or a frame start late in its chunk)
      const int u0 = 14 + 4 * static_cast<int>(lds_byte(slot + r.rs + 14) & 0x0f);
      const int need = min((r.rs + u0 + 8 + 15) >> 4, r.nch);
      for (int k = W; k < need; ++k) lds_store_u128(slot + 16 * k, *XSKNF_GLD(r.cp + k, 16));
    }
    compiler_barrier();
    const Header h = parse_header(slot + r.rs);
    compiler_barrier();
    bool do_sum;
    const int32_t verdict = verdict_of(r, h, args.fwd_verdict, do_sum);
    const int lo = r.rs + h.u, hi = r.rs + r.len;
    const uint32_t wl = (lo & 1) ? 0x01000100u : 0x00010001u;
    const uint32_t wh = wl << 8 | wl >> 24;
    uint32_t acc_lo = 0, acc_hi = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) chunk_sum(v[k], 16 * k, lo, hi, wl, wh, acc_lo, acc_hi);
    const uint32_t PA = acc_lo + (acc_hi << 8);
    const bool more = do_sum && r.nch > W && args.payload_mult != 0;   // payload past the window
    const uint32_t items = more ? static_cast<uint32_t>((r.nch - W + SPAN - 1) / SPAN) : 0u;
    const bool huge = items > kItemsPerFrame;
    int32_t res = r.exists ? verdict : 0;
    LaneOut o = {res, false, slot, r.fp};
    uint2 ent = make_uint2(0, 0);
    if (do_sum && !more && check_changes(args, h, check_of(h, PA, args.payload_mult))) {
      const uint16_t c = check_of(h, PA, args.payload_mult);
      if (static_cast<uint32_t>(r.len) >= defer_min) {
        if (to_list) ent = patch_entry(args, r, h.u, c, 16 * W);
        else res = static_cast<int32_t>(make_record(static_cast<uint32_t>(h.u), c));
      } else {
        store_check_inline(args, r, h.u, c, 16 * W, slot, o);
      }
    }
    store_sectors(o, lane, args.plain_sector);
    const uint32_t part = h.pseudo + args.payload_mult * (PA - h.old_check);

    // ---- phase B: payload items of the longer frames ----
    XSKNF_TL_MARK(tl_p);
    if (__builtin_amdgcn_ballot_w64(more)) {
      const uintptr_t fpv = reinterpret_cast<uintptr_t>(r.fp);
      lds_store_u128(mt + 16 * lane, make_uint4(static_cast<uint32_t>(fpv), static_cast<uint32_t>(fpv >> 32),
                                                static_cast<uint32_t>(r.len), static_cast<uint32_t>(h.u)));
      lds_store_u32(ab + 4 * lane, 0u);
      uint32_t total;
      const uint32_t mine = huge ? 0u : items;
      const uint32_t start = wave_excl_scan(mine, lane, total);
      // the wave's item list, in rounds of kItemCap: two stages of U items per
      // group, ping-pong, so the loads of stage s+1 are in flight while stage s
      // is summed (a stage past the list reloads the last item, masked:
      // straight-line code keeps vmcnt counted, not drained)
      for (uint32_t r0 = 0; r0 < total; r0 += kItemCap) {
        const uint32_t nr = min(total - r0, static_cast<uint32_t>(kItemCap));
        const uint32_t k0 = r0 > start ? r0 - start : 0u;
        const uint32_t k1 = r0 + nr > start ? min(mine, r0 + nr - start) : 0u;
        compiler_barrier();   // the previous round's list has been consumed
        for (uint32_t k = k0; __builtin_amdgcn_ballot_w64(k < k1); ++k)
          if (k < k1) lds_store_u16(iq + 2 * (start + k - r0), static_cast<uint16_t>((lane << 8) | k));
        compiler_barrier();
        ItemStage<U, NCH> sa, sb;
        sa.template issue<W, LPF, SPAN>(iq, mt, 0, nr, grp, gl);
        for (uint32_t it0 = 0;;) {
          sb.template issue<W, LPF, SPAN>(iq, mt, it0 + G * U, nr, grp, gl);
          sa.template consume<LPF>(ab, gl);
          if ((it0 += G * U) >= nr) { sb.template wait<0>(); break; }
          sa.template issue<W, LPF, SPAN>(iq, mt, it0 + G * U, nr, grp, gl);
          sb.template consume<LPF>(ab, gl);
          if ((it0 += G * U) >= nr) { sa.template wait<0>(); break; }
        }
      }
      // frames past the item budget: the whole wave sums each one
      for (uint64_t hm = __builtin_amdgcn_ballot_w64(huge); hm; hm &= hm - 1) {
        const int fl = __builtin_ctzll(hm);
        const Payload pl = payload_of(lds_u128(mt + 16 * fl));
        uint32_t blo = 0, bhi = 0;
        for (int c = W + lane; __builtin_amdgcn_ballot_w64(c < pl.nch); c += kWave)
          chunk_sum_fast(load_nt(pl.cp + min(c, pl.nch - 1)), c * 16, pl.lo, pl.hi, pl.wl, pl.wh, blo, bhi);
        const uint32_t P = group_sum_last<kWave>(blo + (bhi << 8));
        if (lane == kWave - 1) lds_add_u32(ab + 4 * fl, P);
      }
      compiler_barrier();
      XSKNF_TL_MARK(tl_b);
      // ---- phase C: fold, check, store ----
      // an in-line check whose 64-byte sector lies in the frame and the window
      // is written as that whole sector: patched in the lane's slot (the window
      // is still there) and stored by the wave, as in phase A
      LaneOut oc = {0, false, slot, r.fp};
      const uint16_t c = fold_check(part + args.payload_mult * lds_i32(ab + 4 * lane));   // :92-106
      // (its own copy of store_check_inline, the address arithmetic ahead of the
      // defer test: through the helper the list-keeping shapes gain 4 instructions)
      if (more && check_changes(args, h, c)) {
        const uintptr_t f0 = reinterpret_cast<uintptr_t>(r.fp);
        const uintptr_t ck = f0 + h.u + 6;
        const uintptr_t sec = ck & ~static_cast<uintptr_t>(63);
        const uintptr_t c0 = reinterpret_cast<uintptr_t>(r.cp);
        if (static_cast<uint32_t>(r.len) >= defer_min) {
          if (to_list) ent = patch_entry(args, r, h.u, c, 16 * W);
          else res = static_cast<int32_t>(make_record(static_cast<uint32_t>(h.u), c));
        } else if (args.sector_stores && sec >= f0 && sec + 64 <= f0 + r.len && (ck & 63) != 63 &&
                   sec >= c0 && sec + 64 <= c0 + 16 * W) {
          const uint32_t at = slot + static_cast<uint32_t>(ck - c0);
          lds_store_u8(at, static_cast<uint8_t>(c));
          lds_store_u8(at + 1, static_cast<uint8_t>(c >> 8));
          oc.sector = true;
          oc.lds_sec = slot + static_cast<uint32_t>(sec - c0);
          oc.gsec = r.fp + static_cast<intptr_t>(sec - f0);
        } else {
          XSKNF_GST(r.fp + h.u + 6, 2) *reinterpret_cast<uint16_t *>(r.fp + h.u + 6) = c;   // :108
        }
      }
      store_sectors(oc, lane, args.plain_sector);
      compiler_barrier();
    }
    nrec += store_result(args, f, f < args.n, res);
    if (to_list) {
      lds_store_u64(pl + 8 * (it * kWave + lane), ent);
      any_entry |= __builtin_amdgcn_ballot_w64(ent.y != 0) != 0;
    }
    if constexpr (kShared) {
      if (shared_on) {   // publish this unit's list (the entries are in LDS before the mark)
        const bool tany = to_list && __builtin_amdgcn_ballot_w64(ent.y != 0) != 0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        uint32_t slot = 0;
        if (lane == 0) slot = __hip_atomic_fetch_add(&pq_tail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        slot = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(slot), 0));
        if (slot < kPQ) {
          if (lane == 0)
            __hip_atomic_store(&pq[slot], tany ? (static_cast<uint32_t>(wv) << 8 | static_cast<uint32_t>(it)) + 1u : kPQNull,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
          pq_full = true;   // (never: the grid is sized) the wave patches its whole list itself at the end
        }
      }
    }
    ++it;
    compiler_barrier();   // the next tile rewrites the slots
    if constexpr (kPool) {
      tile = tn;
      d = dn;
    } else {
      const uint32_t t3 = tnn != kNoTile && tnn + waves < ntiles ? tnn + waves : kNoTile;
      tile = tn;
      tn = tnn;
      tnn = t3;
      d = dn;
      dn = dnn;
    }
  }
#ifdef XSKNF_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned long long tl1 = wall_clock64();
#endif
  __builtin_amdgcn_s_setprio(0);
  if (args.tail_scatter) {
    if constexpr (kShared) {
      if (shared_on) {
        const uint64_t tw0 = wall_clock64();
        for (;;) {
          uint32_t h = 0;
          if (lane == 0) h = __hip_atomic_fetch_add(&pq_head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          h = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(h), 0));
          if (h >= block_units || h >= kPQ) break;
          uint32_t m = 0;
          for (;;) {
            m = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(
                __hip_atomic_load(&pq[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))));
            if (m != 0 || wall_clock64() - tw0 > 2000000ull) break;   // 20 ms: never, unless units went unclaimed
            __builtin_amdgcn_s_sleep(2);
          }
          if (m == 0) {   // a unit no wave claimed: its frames are unsummed (never, by the grid bound)
            if (lane == 0) __hip_atomic_fetch_add(&g_pool_guard_trips, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          if (m != kPQNull) {
            const uint32_t w2 = (m - 1) >> 8, t2 = (m - 1) & 0xffu;
            tail_patch_list(args, lds_addr(&plist[w2][0]) + 8 * t2 * kWave, 1, lane);
          }
        }
      }
    }
    if (any_entry && (!shared_on || pq_full)) tail_patch_list(args, pl, min(it, PT), lane);
  } else {
    publish_records(args, nrec, lane);
  }
#ifdef XSKNF_TIMELINE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  timeline_put(blockIdx.x * SW + wv, lane, tl0, tl1, it, tl_a, tl_p, tl_b);
#endif
}

}  // namespace xsknf_gpu
