// kernel_group.h -- the register kernel: a group of LPF lanes per frame, the
// frames' chunks in VGPRs (checksum_kernel; its tiles also serve the resident
// worker).  Part of checksummer.hip's one translation unit.
#pragma once
#include "csum_device.h"

namespace xsknf_gpu {

// The word this frame leaves in verdicts[f] after the summing pass; the check
// bytes are written here only in single-pass (fused) mode.
__device__ __forceinline__ int32_t frame_result(const KernelArgs &a, const FrameRef &r, const Header &h,
                                                int32_t verdict, bool do_sum, uint32_t P,
                                                bool sector_done = false) {
  if (!do_sum) return verdict;
  const uint16_t c = check_of(h, P, a.payload_mult);
  if (!check_changes(a, h, c)) return verdict;
  if (static_cast<uint32_t>(r.len) >= a.defer_min_len)
    return static_cast<int32_t>(make_record(static_cast<uint32_t>(h.u), c));
  if (!sector_done) *reinterpret_cast<uint16_t *>(r.fp + h.u + 6) = c;   // :108
  return verdict;
}

// In-line check as a whole-sector rewrite (register kernel, pass-0 frames):
// when the check's 64-byte sector lies inside the frame, the (up to 4) lanes
// whose 16-byte chunks make up that sector patch the check bytes into the
// chunk they loaded and store it back non-temporally -- one full-sector write
// instead of a 2-byte partial write, which HBM turns into read-modify-write.
// Returns true (on every lane of the group) when the sector was written.
// (The chunks are in registers, not an LDS slot, and the sector need not lie in
// a window: its own copy of store_check_inline's in-frame rule -- sharing the
// predicate changed checksum_kernel<64, 2, 4>'s register assignment.)
template <int LPF, int NCH>
__device__ __forceinline__ bool store_check_sector(const FrameRef &r, const Header &h, uint16_t c,
                                                   const uint4 (&v)[NCH], int gl) {
  const uintptr_t f0 = reinterpret_cast<uintptr_t>(r.fp);
  const uintptr_t ck = f0 + h.u + 6;
  const uintptr_t sec = ck & ~static_cast<uintptr_t>(63);
  if (sec < f0 || sec + 64 > f0 + r.len || (ck & 63) == 63) return false;
  const uintptr_t c0 = reinterpret_cast<uintptr_t>(r.cp);
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const uintptr_t piece = c0 + 16u * static_cast<uint32_t>(k * LPF + gl);
    if (piece >= sec && piece < sec + 64) {
      const int o = static_cast<int>(static_cast<intptr_t>(ck - piece));
      uint4 w = put_byte(v[k], o, c);
      w = put_byte(w, o + 1, c >> 8);
      store_nt16(r.fp + static_cast<intptr_t>(piece - f0), w);   // global addressing from fp
    }
  }
  return true;
}

// Frames longer than one pass.  The pipelined step only sums pass 0 and parks
// the frame as PENDING (make_pending(u) as its result word, checksummer_internal.h,
// the partial sum pseudo + mult*(P0 - old_check) in part[i]); the remaining passes
// run at the end of the tile, when no prefetch buffer is live (keeping them in
// the step would cost ~60 VGPRs of occupancy for a rare case).

// Result word of a frame after its pass-0 sum P0 (group-reduced, last lane).
__device__ __forceinline__ int32_t step_result(const KernelArgs &a, const FrameRef &r, const Header &h,
                                               int32_t verdict, bool do_sum, uint32_t P0, int span,
                                               uint32_t part_addr, bool sector_done = false) {
  if (do_sum && r.nch > span) {
    lds_store_u32(part_addr, h.pseudo + a.payload_mult * (P0 - h.old_check));
    return static_cast<int32_t>(make_pending(static_cast<uint32_t>(h.u)));
  }
  return frame_result(a, r, h, verdict, do_sum, P0, sector_done);
}

// Finish the PENDING frames of a tile: passes 1.. of each, then their result.
// dsc: the tile's descriptors in LDS; rec / part: the tile's result words and
// partial sums in LDS (index step * G + group).
template <int LPF, int NCH>
__device__ __forceinline__ void finish_long_frames(const KernelArgs &a, uint32_t dsc, uint32_t tf0, uint32_t rec,
                                                uint32_t part, int steps, int grp, int gl) {
  constexpr int G = kWave / LPF;
  constexpr int SPAN = LPF * NCH;
  for (int st = 0; st < steps; ++st) {
    const uint32_t i = st * G + grp;
    const uint32_t rv = static_cast<uint32_t>(lds_i32(rec + 4 * i));
    const bool pend = is_pending(rv) && tf0 + i < a.n;
    if (!__builtin_amdgcn_ballot_w64(pend)) continue;
    const FrameRef r = ref_from_lds(a, dsc + 16 * i, tf0 + i);
    const int u = static_cast<int>(pending_u(rv));
    const int lo = r.rs + u, hi = pend ? r.rs + r.len : lo;   // idle groups sum nothing
    const uint32_t wl = (lo & 1) ? 0x01000100u : 0x00010001u;
    const uint32_t wh = wl << 8 | wl >> 24;
    uint32_t acc_lo = 0, acc_hi = 0;
    for (int p = SPAN; __builtin_amdgcn_ballot_w64(pend && p < r.nch); p += SPAN) {
      uint4 t[NCH];
#pragma unroll
      for (int k = 0; k < NCH; ++k) t[k] = load_nt(r.cp + min(p + k * LPF + gl, r.nch - 1));
#pragma unroll
      for (int k = 0; k < NCH; ++k) chunk_sum_fast(t[k], (p + k * LPF + gl) * 16, lo, hi, wl, wh, acc_lo, acc_hi);
    }
    const uint32_t Prest = group_sum_last<LPF>(acc_lo + (acc_hi << 8));
    if (gl == LPF - 1 && pend) {
      const uint16_t c = fold_check(lds_i32(part + 4 * i) + a.payload_mult * Prest);   // :92-106
      int32_t res = a.fwd_verdict;
      // the old check, for check_changes (pass 0's window is gone: 2 bytes from the frame)
      const uint16_t old = static_cast<uint16_t>(r.fp[u + 6] | (r.fp[u + 7] << 8));
      if (c == old && !a.store_unchanged) {
        // the frame already holds c: nothing to write
      } else if (static_cast<uint32_t>(r.len) >= a.defer_min_len)
        res = static_cast<int32_t>(make_record(static_cast<uint32_t>(u), c));
      else *reinterpret_cast<uint16_t *>(r.fp + u + 6) = c;   // :108
      lds_store_i32(rec + 4 * i, res);
    }
  }
}

// ---- register kernel ----------------------------------------------------------
//
// A wave works through tiles of SPT steps x G frames (consecutive frames; the
// grid strides over tiles).  Inside a tile the step loop is fully unrolled over
// two register buffers: the loads of step s+1 are issued before step s is
// parsed / summed / reduced, and because the code is straight-line the compiler
// counts vmcnt exactly (a loop-carried load would make it drain to 0).

template <int LPF, int NCH>
__device__ __forceinline__ void load_frame(const FrameRef &r, int gl, uint4 (&v)[NCH]) {
#pragma unroll
  for (int k = 0; k < NCH; ++k) v[k] = load_nt(r.cp + min(k * LPF + gl, r.nch - 1));
}

template <int LPF, int NCH>
__device__ __forceinline__ int32_t process_regs(const KernelArgs &args, const FrameRef &r, const uint4 (&v)[NCH],
                                                uint32_t slot, int gl, uint32_t part_addr) {
  // header window (chunks 0..6) to LDS; one wave's LDS accesses execute in issue
  // order, only the compiler must not move the reads above the writes
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int c = k * LPF + gl;
    if (k * LPF < kHdrChunks && c < kHdrChunks) lds_store_u128(slot + 16 * c, v[k]);
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
  for (int k = 0; k < NCH; ++k) chunk_sum_fast(v[k], (k * LPF + gl) * 16, lo, hi, wl, wh, acc_lo, acc_hi);
  const uint32_t P0 = group_sum_last<LPF>(acc_lo + (acc_hi << 8));
  bool sector_done = false;
  if (args.sector_stores && __builtin_amdgcn_ballot_w64(do_sum && r.nch <= LPF * NCH &&
                                                        static_cast<uint32_t>(r.len) < args.defer_min_len)) {
    const uint32_t P = group_bcast_last<LPF>(P0, lane_id());
    const uint16_t c = check_of(h, P, args.payload_mult);
    if (do_sum && r.nch <= LPF * NCH && static_cast<uint32_t>(r.len) < args.defer_min_len &&
        check_changes(args, h, c))
      sector_done = store_check_sector<LPF, NCH>(r, h, c, v, gl);
  }
  return (gl == LPF - 1 && r.exists)
             ? step_result(args, r, h, verdict, do_sum, P0, LPF * NCH, part_addr, sector_done) : 0;
}

// The register kernel's tiles of block `blk` of `nblk` (a launch's blockIdx /
// gridDim, or the resident worker's blocks over one ring batch).
template <int LPF, int NCH, int SPT>
__device__ __forceinline__ void group_tiles(const KernelArgs &args, uint32_t blk, uint32_t nblk) {
  static_assert(kWave % LPF == 0 && LPF >= 4, "LPF must divide the wave");
  static_assert(LPF * NCH >= kHdrChunks, "pass 0 must cover the header window");
  constexpr int G = kWave / LPF;
  constexpr int T = SPT * G;                 // frames per tile
  static_assert(T <= kWave, "one descriptor / result per lane");

  __shared__ __attribute__((aligned(16))) uint8_t hdr[kWavesPerBlock][G][kSlotBytes];
  __shared__ __attribute__((aligned(16))) int32_t recs[kWavesPerBlock][kWave];
  __shared__ __attribute__((aligned(16))) uint32_t parts[kWavesPerBlock][kWave];
  __shared__ __attribute__((aligned(16))) xsknf_gpu_desc dtile[kWavesPerBlock][kWave];

  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int grp = lane / LPF;
  const int gl = lane % LPF;
  const uint32_t slot = lds_addr(&hdr[wv][grp][0]);
  const uint32_t rec = lds_addr(&recs[wv][0]);
  const uint32_t part = lds_addr(&parts[wv][0]);
  const uint32_t dsc = lds_addr(&dtile[wv][0]);
  const uint32_t waves = nblk * kWavesPerBlock;
  const uint32_t last = args.n - 1;

  // the next tile's descriptors ride in VGPRs (lane l: frame l of the tile)
  uint32_t tile = blk * kWavesPerBlock + wv;
  uint32_t nrec = 0;                         // records this wave parked (wave-uniform)
  uint4 dnext = *reinterpret_cast<const uint4 *>(args.descs + min(tile * T + min(lane, T - 1), last));
  for (; tile * T < args.n; tile += waves) {
    const uint32_t tf0 = tile * T;
    compiler_barrier();
    if (lane < T) lds_store_u128(dsc + 16 * lane, dnext);
    compiler_barrier();
    // per-tile store policy: long frames defer their checks only where they are
    // at least half of the tile (a 1500 B batch); in a mix (IMIX: 1 in 12) they
    // write in-line, which is cheaper than a scatter pass for a few frames
    KernelArgs ta = args;
    if (args.defer_min_len != kNoDefer && args.defer_min_len != 0 && !args.no_scatter) {
      const uint32_t nlong = static_cast<uint32_t>(__builtin_popcountll(
          __builtin_amdgcn_ballot_w64(lane < T && tf0 + lane < args.n && dnext.z >= args.defer_min_len)));
      const uint32_t nlive = min(static_cast<uint32_t>(T), args.n - tf0);
      if (kDeferTileK * nlong < nlive) ta.defer_min_len = kNoDefer;
    }
    dnext = *reinterpret_cast<const uint4 *>(args.descs + min((tile + waves) * T + min(lane, T - 1), last));

    uint4 va[NCH], vb[NCH];
    FrameRef ra = ref_from_lds(args, dsc + 16 * grp, tf0 + grp), rb;
    load_frame<LPF, NCH>(ra, gl, va);
#pragma unroll
    for (int st = 0; st < SPT; ++st) {
      // even steps: process (ra, va), prefetch into (rb, vb); odd steps: swapped
      FrameRef &rc = (st & 1) ? rb : ra;
      FrameRef &rn = (st & 1) ? ra : rb;
      uint4 (&vc)[NCH] = (st & 1) ? vb : va;
      uint4 (&vn)[NCH] = (st & 1) ? va : vb;
      if (st + 1 < SPT) {
        const uint32_t i = (st + 1) * G + grp;
        rn = ref_from_lds(args, dsc + 16 * i, tf0 + i);
        load_frame<LPF, NCH>(rn, gl, vn);
      }
      const int32_t res = process_regs<LPF, NCH>(ta, rc, vc, slot, gl, part + 4 * (st * G + grp));
      if (gl == LPF - 1 && rc.exists) lds_store_i32(rec + 4 * (st * G + grp), res);
      compiler_barrier();   // the next frame rewrites this group's header window
    }
    compiler_barrier();
    finish_long_frames<LPF, NCH>(ta, dsc, tf0, rec, part, SPT, grp, gl);
    compiler_barrier();
    nrec += store_result(args, tf0 + lane, lane < T && tf0 + lane < args.n, lds_i32(rec + 4 * min(lane, T - 1)));
    compiler_barrier();
  }
  publish_records(args, nrec, lane);
}

template <int LPF, int NCH, int SPT>
__global__ __launch_bounds__(kBlock) void checksum_kernel(const KernelArgs args) {
  group_tiles<LPF, NCH, SPT>(args, blockIdx.x, gridDim.x);
}

}  // namespace xsknf_gpu
