// kernel_resident.h -- the resident worker's kernel (resident_kernel).  Part of
// checksummer.hip's one translation unit.
#pragma once
#include "kernel_group.h"

namespace xsknf_gpu {

// ---- the resident worker (checksummer_internal.h) ------------------------------
//
// ONE kernel per device serves every RESIDENT context's ring (ResLaunch::ring).
// ResLaunch::block maps each block to its ring, its place g in an entry's group
// and its first entry; a block serves entries b, b + kResSlots / E, ... of that
// ring (E = ResArgs::entries_per_block, 1 unless the rings would need more
// blocks than the grid may have).  Its first lane polls those entries' headers
// (in host memory, or in device memory the host writes through the BAR) for
// the next sequence number that maps to each, which carries the batch's frame
// count in the same word: system-scope RELAXED loads (vector loads that bypass
// the caches without the invalidation an acquire adds per poll), all E of them
// issued before any is compared; the acquire is one fence once a batch with
// frames for this block is there.  The blocks of a group deal the batch in
// 64-frame rounds (the register kernel's tiles, 8 lanes x 12 chunks per frame:
// a frame of up to 1536 B in one pass, longer ones in further passes), so a
// 256-frame batch is one round of PCIe reads on each of four CUs and a 64-frame
// batch one round on one; each block with frames stores its `done` to host
// memory (system-scope release).  A ring whose batches are at most 64 frames
// runs one block per entry (ResRing::group = 1): idle blocks' polls cost those
// batches ~1 us.  A block without frames reads nothing but the word and moves
// on; it may find the entry already past it (the host waits only for the
// blocks with frames), and then takes the newer number.
// A block leaves when the host sets the stop word (a ring joins or leaves), when
// NO block has finished a batch for idle_ticks (ResLaunch::act, the clock of
// the latest batch, kept by an atomic max at most every idle_ticks / 8 per
// block), or after life_ticks in all; it
// tells the others by setting act to kResQuit, and the last block to leave
// reports the launch's epoch in ctl->exited.  A batch published to a kernel
// that has left waits for the host to relaunch it (every block then starts at
// its entries' first batch not done).  Every wave reaches an exit: the poll
// loops are bounded by the clock, and a batch is a bounded loop.
constexpr int kResLpf = 8, kResNch = 12, kResSpt = 2;

// A wave-uniform value read from LDS, moved to scalar registers: addresses
// built from it then use the SGPR-base forms, as with kernel arguments.
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  return static_cast<uint64_t>(uniform_u32(static_cast<uint32_t>(v >> 32))) << 32 | uniform_u32(static_cast<uint32_t>(v));
}
// ... and known to address global memory: a pointer read from LDS is generic,
// and every access through it would be a FLAT instruction (both counters, no
// scalar base); made from the integer as a global pointer, then cast to
// generic, its uses get the GLOBAL forms from the compiler's address-space
// inference, as kernel arguments do.
template <typename T>
__device__ __forceinline__ T *uniform_ptr(T *p) {
  typedef __attribute__((address_space(1))) T gT;
  gT *const q = (gT *)uniform_u64(reinterpret_cast<uint64_t>(p));   // an integer made a global pointer ...
  return (T *)q;                                                     // ... then generic: inferable
}

__global__ __launch_bounds__(kBlock) void resident_kernel(const ResArgs ra) {
  static_assert(kResBlockFrames == kWavesPerBlock * kResSpt * (kWave / kResLpf), "one round per block");
  __shared__ uint64_t cmd;
  __shared__ uint32_t hdr[5];
  // the block's ring, read once into scalar registers: the system-scope
  // acquire of every batch invalidates the caches, and the ring's pointers
  // would be re-read from memory behind it on each batch's critical path
  // (read through ra.rings, a read-only view: the compiler then knows them to
  // be global pointers and uses the GLOBAL forms, not FLAT)
  ResLaunch *const L = ra.L;
  const uint32_t m = L->block[blockIdx.x];
  const uint32_t r = m >> 16, g = (m >> 8) & 0xff, b0 = m & 0xff;
  const ResRing &Rg = ra.rings[r];
  uint8_t *const r_umem = uniform_ptr(Rg.umem);
  const uint64_t r_umem_size = uniform_u64(Rg.umem_size);
  ResIn *const in = uniform_ptr(Rg.in);
  xsknf_gpu_desc *const r_descs = uniform_ptr(Rg.descs);
  ResOut *const r_out = uniform_ptr(Rg.out);
  int32_t *const r_verdicts = uniform_ptr(Rg.verdicts);
  const uint32_t G = uniform_u32(Rg.group);
  const uint32_t E = ra.entries_per_block, stride = kResSlots / E;
  // lane 0's state: the next sequence number of each entry it serves (in LDS:
  // registers live across group_tiles would cost the kernel its second wave per SIMD)
  __shared__ uint64_t next[kResSlots];
  if (threadIdx.x < kResSlots)
    next[threadIdx.x] = threadIdx.x < E ? L->start[r][(b0 + threadIdx.x * stride) * kResGroup + g] : kResQuit;
  __syncthreads();
  const uint64_t t0 = wall_clock64();
  uint64_t last = t0, told = t0;   // this block's latest batch; when it last told L->act
  for (;;) {
    if (threadIdx.x == 0) {
      uint64_t c = kResQuit;
      uint32_t n = 0, b = b0;
      for (bool got = false; !got;) {
        // every word of the poll issued before any is looked at: one round
        // trip per poll, not one per word
        uint64_t w[kResSlots];
#pragma unroll
        for (uint32_t j = 0; j < kResSlots; ++j)
          w[j] = j < E ? __hip_atomic_load(&in[b0 + j * stride].seqn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                       : 0;
        const uint64_t act = __hip_atomic_load(&L->act, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t stop = __hip_atomic_load(ra.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint64_t now = wall_clock64();
#pragma unroll
        for (uint32_t j = 0; j < kResSlots; ++j) {
          // a number past next[j]: the entry moved on while this block had no
          // frames in its batches (the host waits for the blocks that do)
          if (!got && j < E && (w[j] >> 16) >= next[j]) {
            got = true;
            c = w[j] >> 16;
            n = static_cast<uint32_t>(w[j] & 0xFFFF);
            b = b0 + j * stride;
            next[j] = c + kResSlots;
          }
        }
        if (got) break;
        // (a signed difference: another block's latest batch may have ended
        // after this block read the clock)
        const int64_t idle = static_cast<int64_t>(now - (act > last ? act : last));
        if ((act == kResQuit) | (stop != 0) | (idle > static_cast<int64_t>(ra.idle_ticks)) |
            (now - t0 > ra.life_ticks)) {
          __hip_atomic_fetch_max(&L->act, kResQuit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      if (c != kResQuit) {
        // (the header is read only by a block with frames: the host cannot
        // rewrite it before that block's done; a block without frames skips
        // the fence, whose cache invalidation would cost the XCD's busy blocks)
        hdr[3] = g < res_used_blocks(n, G);
        hdr[0] = hdr[3] ? n : 0;
        hdr[4] = b;
        if (hdr[3]) {
          // the host's writes of this batch (header, descriptors, frames), seen from this CU
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // system scope
          // fwd and payload_mult in one 8-byte load (one round trip)
          const uint64_t fm = __hip_atomic_load(reinterpret_cast<uint64_t *>(&in[b].fwd), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_SYSTEM);
          hdr[1] = static_cast<uint32_t>(fm);
          hdr[2] = static_cast<uint32_t>(fm >> 32);
        }
      }
      cmd = c;
    }
    __syncthreads();
    const uint64_t c = cmd;
    if (c == kResQuit) break;
    {
      const uint32_t b = uniform_u32(hdr[4]);
      // the ring's UMEM is host memory mapped over PCIe: every check in-line as
      // a 2-byte store (byte enables, no read-modify-write); the store modes are
      // constants here, so only the ring's pointers take (scalar) registers
      KernelArgs a;
      a.umem = r_umem;
      a.umem_size = r_umem_size;
      a.descs = r_descs + static_cast<size_t>(b) * kResFrames;
      a.verdicts = r_verdicts + static_cast<size_t>(b) * kResFrames;
      a.dummy = reinterpret_cast<const uint4 *>(r_descs);
      a.n = min(uniform_u32(hdr[0]), kResFrames);
      a.fwd_verdict = static_cast<int32_t>(uniform_u32(hdr[1]));
      a.payload_mult = uniform_u32(hdr[2]);
      a.defer_min_len = kNoDefer;
      a.no_scatter = 0;
      a.seq = 0;
      a.count_records = 0;
      a.sector_stores = 0;
      a.plain_sector = 0;
      a.tail_scatter = 0;
      a.store_unchanged = 0;
      // the group's blocks deal the batch in 64-frame rounds: block g takes
      // frames [64 g, 64 g + 64) of a batch of up to 256
      if (a.n) group_tiles<kResLpf, kResNch, kResSpt>(a, g, G);
      __syncthreads();   // the block's stores are done (workgroup release / acquire)
      if (threadIdx.x == 0) {
        if (hdr[3]) {
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: the checks and verdicts
          __hip_atomic_store(&r_out[b * kResGroup + g].done, c, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        last = wall_clock64();
        // the device-wide activity only needs the idle exit's precision: an
        // atomic per batch (on one word, from every block) would sit in front
        // of the next poll's wait
        if (last - told > ra.idle_ticks / 8) {
          __hip_atomic_fetch_max(&L->act, last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          told = last;
        }
      }
    }
  }
  if (threadIdx.x == 0 &&
      __hip_atomic_fetch_add(&L->exits, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == ra.blocks - 1)
    __hip_atomic_store(&ra.ctl->exited, ra.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace xsknf_gpu
