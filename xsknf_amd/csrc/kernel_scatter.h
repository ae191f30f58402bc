// kernel_scatter.h -- the write-only pass of the parked checks (scatter_checks).
// Part of checksummer.hip's one translation unit.
#pragma once
#include "csum_device.h"

namespace xsknf_gpu {

// ---- phase 2: write-only pass of the parked checks (:108) and verdicts -------
//
// Measured on MI355X (tools/hbm_probe): a scattered 2-byte write costs as much
// as a read-modify-write of its 64-byte memory sector, and writes left dirty in
// the caches are written back during the NEXT batch's read pass, where they
// cost far more.  So this pass uses non-temporal stores (written back now) and,
// where the aligned 64-byte sector holding the check lies entirely inside the
// frame, rewrites the whole sector -- its 64 bytes re-read and patched -- as ONE
// store instruction of 4 adjacent lanes (a full-sector write, no RMW): 4 lanes
// per frame.  Otherwise (sector crosses the frame edge, or the check straddles
// two sectors) it writes the 2 check bytes alone.  Only this frame's own bytes
// are ever rewritten (with their own values), so frames never race.
//
// Two shapes, picked per launch from the record count the summing kernel
// leaves in g_rec_count: dense (4 lanes per frame over the grid) and sparse
// (per-wave scan + compaction).

// Rewrite one parked check: lane `piece` (0..3) of the record's 4 lanes.
__device__ __forceinline__ void rewrite_check(const KernelArgs &args, uint32_t f, uint32_t r,
                                              const xsknf_gpu_desc &d, int piece) {
  uint8_t *fp = args.umem + desc_offset(d.addr);
  uint8_t *chk = fp + record_check_offset(r);
  const uint16_t c = record_check(r);
  uint8_t *sec = chk - (reinterpret_cast<uintptr_t>(chk) & 63);   // keeps global addressing
  const bool whole = sec >= fp && sec + 64 <= fp + d.len && (reinterpret_cast<uintptr_t>(chk) & 63) != 63;
  if (whole) {
    uint8_t *mine = sec + 16 * piece;
    const int o = static_cast<int>(chk - mine);          // check offset in my 16-B piece (-1..63)
    uint4 v = load_nt(reinterpret_cast<const uint4 *>(mine));
    v = put_byte(v, o, c);
    v = put_byte(v, o + 1, c >> 8);
    store_nt16(mine, v);
  } else if (piece == 0) {
    XSKNF_GST(chk, 2) {
      chk[0] = static_cast<uint8_t>(c);
      chk[1] = static_cast<uint8_t>(c >> 8);
    }
  }
  if (piece == 0) {
    XSKNF_GST(args.verdicts + f, 4) args.verdicts[f] = args.fwd_verdict;
  }
}

// Dense records (>= 1/4 of the frames): 4 lanes per frame over the whole grid;
// each lane's record and descriptor loads are independent of any scan.  A lane
// takes kScatterU frames per round, so each round costs two dependent memory
// round trips (record + descriptor, then the sector) for kScatterU frames
// rather than per frame: the pass is latency-bound, not bandwidth-bound.
constexpr int kScatterU = 4;

__device__ __forceinline__ void scatter_dense(const KernelArgs &args) {
  const uint32_t nthreads = gridDim.x * kBlock;
  const uint32_t total = 4 * args.n;
  for (uint32_t t0 = blockIdx.x * kBlock + threadIdx.x; t0 < total; t0 += kScatterU * nthreads) {
    uint32_t r[kScatterU];
    xsknf_gpu_desc d[kScatterU];
#pragma unroll
    for (int k = 0; k < kScatterU; ++k) {
      const uint32_t f = min(t0 + k * nthreads, total - 1) >> 2;
      r[k] = static_cast<uint32_t>(*XSKNF_GLD(args.verdicts + f, 4));
      d[k] = *XSKNF_GLD(args.descs + f, 16);
    }
    uint4 v[kScatterU];
    uint8_t *mine[kScatterU];
    int o[kScatterU];
    bool whole[kScatterU], rec[kScatterU];
#pragma unroll
    for (int k = 0; k < kScatterU; ++k) {
      const uint32_t t = t0 + k * nthreads;
      rec[k] = t < total && is_record(r[k]);
      uint8_t *fp = args.umem + desc_offset(d[k].addr);
      uint8_t *chk = fp + record_check_offset(r[k]);
      uint8_t *sec = chk - (reinterpret_cast<uintptr_t>(chk) & 63);   // keeps global addressing
      whole[k] = rec[k] && sec >= fp && sec + 64 <= fp + d[k].len && (reinterpret_cast<uintptr_t>(chk) & 63) != 63;
      mine[k] = whole[k] ? sec + 16 * (t & 3) : chk;
      o[k] = static_cast<int>(chk - mine[k]);
      if (whole[k]) v[k] = load_nt(reinterpret_cast<const uint4 *>(mine[k]));   // plain: 296 -> 311 us
    }
#pragma unroll
    for (int k = 0; k < kScatterU; ++k) {
      const uint32_t t = t0 + k * nthreads;
      const uint16_t c = record_check(r[k]);
      if (whole[k]) {
        uint4 w = put_byte(v[k], o[k], c);
        w = put_byte(w, o[k] + 1, c >> 8);
        store_nt16(mine[k], w);
      } else if (rec[k] && (t & 3) == 0) {
        XSKNF_GST(mine[k], 2) {
          mine[k][0] = static_cast<uint8_t>(c);
          mine[k][1] = static_cast<uint8_t>(c >> 8);
        }
      }
      if (rec[k] && (t & 3) == 0) {
        XSKNF_GST(args.verdicts + (t >> 2), 4) args.verdicts[t >> 2] = args.fwd_verdict;
      }
    }
  }
}

// Sparse records: one lane per frame scans; each wave ballots its 64 frames and
// rewrites only its records, 16 per round (4 lanes each), so the pass costs in
// proportion to the records (IMIX: 1 frame in 12), not to n.
__device__ __forceinline__ void scatter_sparse(const KernelArgs &args, uint8_t *which) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint32_t waves = gridDim.x * kWavesPerBlock;
  for (uint32_t base = (blockIdx.x * kWavesPerBlock + wv) * kWave; base < args.n; base += waves * kWave) {
    const uint32_t f = base + lane;
    const uint32_t r = f < args.n ? static_cast<uint32_t>(*XSKNF_GLD(args.verdicts + f, 4)) : 0u;
    const bool rec = is_record(r);
    const uint64_t m = __builtin_amdgcn_ballot_w64(rec);
    if (!m) continue;
    const int nrec = __builtin_popcountll(m);
    if (rec) {
      const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                 __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
      which[rank] = static_cast<uint8_t>(lane);
    }
    __builtin_amdgcn_wave_barrier();
    for (int k0 = 0; k0 < nrec; k0 += kWave / 4) {
      const int k = k0 + (lane >> 2);
      const int src = which[min(k, nrec - 1)];
      const uint32_t rs = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src << 2, static_cast<int>(r)));
      if (k < nrec) rewrite_check(args, base + src, rs, *XSKNF_GLD(args.descs + base + src, 16), lane & 3);
    }
    __builtin_amdgcn_wave_barrier();   // `which` is rewritten by the next chunk
  }
}

__global__ __launch_bounds__(kBlock) void scatter_checks(const KernelArgs args) {
  __shared__ uint8_t which[kWavesPerBlock][kWave];     // record rank -> lane (sparse shape)
  // nothing parked: done (exact, see g_rec_count); an unknown count (the
  // counter set was reused by a later launch in flight) takes the sparse scan,
  // which finds any record
  const uint32_t cnt = __builtin_amdgcn_readfirstlane(launch_records(args));
  if (cnt == 0) return;
  if (cnt != kCountUnknown && 4ull * cnt >= args.n)
    scatter_dense(args);
  else
    scatter_sparse(args, which[threadIdx.x / kWave]);
}

}  // namespace xsknf_gpu
