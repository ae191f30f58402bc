// checksummer.hip -- gfx950 kernels for the xsknf checksummer per-packet path:
// one translation unit.  The device code is in csum_device.h (shared helpers)
// and one header per kernel family -- kernel_group.h (register), kernel_lane.h,
// kernel_split.h, kernel_scatter.h, kernel_resident.h; this file keeps the host
// side: error text, grid sizing, the launchers, the Variant table, default_cfg,
// prepare, run and the C API.
//
// Reference semantics: examples/checksummer/checksummer_user.c:30-112
// (xsknf_packet_processor), applied to every descriptor of an rx batch as the
// per-frame loop of src/xsknf.c:654-672 does.
//
// Arithmetic.  The reference sums 16-bit words serially from the UDP header to
// the end of the frame into a wrapping u32, so the sum can be taken in any
// order and in closed form:
//     s = pseudo + max(iters,0) * P                         (mod 2^32)
//     P = sum_{k even} f[u+k] + 256 * sum_{k odd} f[u+k],   k in [0, len-u)
// with f[u+6], f[u+7] (the old check) counted as zero.  "k even" are the bytes
// whose ABSOLUTE address parity equals that of the UDP header start, so frames
// are read as 16-byte aligned chunks wherever they start (unaligned-chunk UMEM
// puts frames at odd addresses) and every dword is split into its low- and
// high-weight byte pairs by v_dot4_u32_u8, whose u8 weight operand also carries
// the [udp, end) byte mask.  One fold with the carry dropped, as :105-106.
//
// Mapping (MI355X: 64-lane waves, HBM-bound integer reduction, no MFMA).
// * A group of LPF lanes owns one frame; a wave holds G = 64/LPF groups; each
//   lane covers NCH 16-byte chunks per pass, so one pass reads LPF*NCH*16
//   contiguous bytes of a frame with dwordx4 loads contiguous across the group.
// * Waves own TILES of 64 consecutive frames (persistent grid striding over
//   tiles), so per-frame results collect in LDS and leave as one 256-B store.
// * Loads are non-temporal (streamed once; +8-10 % read bandwidth measured).
// * Kernel families, same results:
//     - split (the default): lane l of a wave parses / finishes frame l of a
//       64-frame tile from its header window, and the payload past the window
//       is summed in one-pass items dealt to lane groups (any mix of lengths);
//     - register: each step loads U frames per group into VGPRs, then parses /
//       sums / reduces them one by one (frame u+1 in flight behind frame u);
//     - lane: one lane per frame, whole frame (small frames).
// * Group partial sums reduce with DPP (row_shr / row_bcast) into the group's
//   last lane.
// * Stores (default_cfg): frames <= 128 B write each check in-line as its
//   whole 64-byte sector (written through L2 where the frames lie apart).
//   Longer frames defer every check -- writes mixed into the read stream cost
//   several times their bytes (tools/hbm_probe) -- into the wave's LDS patch
//   list (sector index + check); once the stream is done each listed sector is
//   rewritten whole (tail_patch_list), with no second launch: by the wave
//   itself after its last tile (4-wave blocks), or by any wave of the block
//   done streaming, from the block's queue (pooled blocks, jumbo included).
//   Only the modes that ask for it (fused_stores 0) park check records in
//   `verdicts` for a write-only scatter_checks pass.
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <stdint.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dirent.h>
#include <stdarg.h>
#include <fcntl.h>
#include <unistd.h>

#include "../../include/xsknf_gpu.h"
#include "checksummer_internal.h"

#include "csum_device.h"
#include "kernel_group.h"
#include "kernel_lane.h"
#include "kernel_split.h"
#include "kernel_scatter.h"
#include "kernel_resident.h"

// ---- host side ----------------------------------------------------------------

// A/B builds (make ab) add launch shapes and knobs; the product sees no-ops
#ifdef XSKNF_AB
#include "checksummer_ab.h"
#else
namespace xsknf_gpu {
inline void ab_note_occupancy(const void *, int, int) {}
inline int ab_scatter_bpc(int dflt) { return dflt; }
inline bool ab_no_grid_bound() { return false; }
}  // namespace xsknf_gpu
#define XSKNF_AB_VARIANTS
#endif

namespace xsknf_gpu {

// The last error of ANY thread: a worker thread's failure (hook context
// creation, UMEM registration, a launch) must be readable by the application's
// main thread (checksummer_app.c prints it).  Each reader gets a private copy,
// so the returned text cannot change under it.
std::mutex g_err_mu;
char g_last_error[1024] = "";
thread_local char g_err_copy[1024] = "";

void set_error_text(const char *text) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  snprintf(g_last_error, sizeof(g_last_error), "%s", text);
}

void set_error(hipError_t e, const char *where) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", where, hipGetErrorString(e));
}

const char *last_error_copy() {
  std::lock_guard<std::mutex> lk(g_err_mu);
  memcpy(g_err_copy, g_last_error, sizeof(g_err_copy));
  return g_err_copy;
}

// A process that finds no usable device says why (src/xsknf.c:108-119: a start
// failure is fatal and loud): HIP's error and count, whether this process can
// open the KFD and the first render node, which *_VISIBLE_DEVICES are set, how
// many processes hold a KFD context (/sys/class/kfd/kfd/proc, by pid) and this
// process's open descriptors.  Used where hipGetDeviceCount fails or sees none.
struct ErrText {
  char buf[sizeof(g_last_error)] = "";
  size_t o = 0;
  __attribute__((format(printf, 2, 3))) void put(const char *fmt, ...) {
    if (o >= sizeof(buf)) return;
    va_list ap;
    va_start(ap, fmt);
    const int w = vsnprintf(buf + o, sizeof(buf) - o, fmt, ap);
    va_end(ap);
    if (w > 0) o += static_cast<size_t>(w);
  }
};

int set_device_error(hipError_t e, int count, const char *where) {
  ErrText t;
  t.put("%s: %s (hipError %d), %d devices", where, hipGetErrorString(e), static_cast<int>(e), count);
  const int kfd = open("/dev/kfd", O_RDWR | O_CLOEXEC);
  if (kfd >= 0) {
    t.put("; /dev/kfd opens");
    close(kfd);
  } else {
    t.put("; /dev/kfd: errno %d (%s)", errno, strerror(errno));
  }
  int render = 0;
  char first[64] = "";
  if (DIR *d = opendir("/dev/dri")) {
    while (const dirent *ent = readdir(d))
      if (!strncmp(ent->d_name, "renderD", 7) && render++ == 0) snprintf(first, sizeof(first), "%s", ent->d_name);
    closedir(d);
  }
  if (render) {
    char path[96];
    snprintf(path, sizeof(path), "/dev/dri/%s", first);
    const int fd = open(path, O_RDWR | O_CLOEXEC);
    t.put("; %d render nodes, %s %s", render, path, fd >= 0 ? "opens" : strerror(errno));
    if (fd >= 0) close(fd);
  } else {
    t.put("; no render node in /dev/dri");
  }
  for (const char *v : {"HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"})
    if (const char *s = getenv(v)) t.put("; %s=%s", v, s);
  int procs = 0;
  if (DIR *d = opendir("/sys/class/kfd/kfd/proc")) {
    t.put("; KFD processes:");
    while (const dirent *ent = readdir(d))
      if (ent->d_name[0] != '.') {
        if (procs++ < 16) t.put(" %s", ent->d_name);
      }
    closedir(d);
    t.put(" (%d; this pid %d)", procs, static_cast<int>(getpid()));
  } else {
    t.put("; /sys/class/kfd/kfd/proc: %s", strerror(errno));
  }
  int fds = 0;
  if (DIR *d = opendir("/proc/self/fd")) {
    while (const dirent *ent = readdir(d)) fds += ent->d_name[0] != '.';
    closedir(d);
  }
  t.put("; %d open fds", fds);
  set_error_text(t.buf);
  return -ENODEV;
}

int device_cus() {
  static int cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cache[dev]) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return 256;
    // XSKNF_GPU_CU_LIMIT (test hook): size the grids as on a device with that
    // many CUs (a compute partition has 32), so the grid-sizing bounds for
    // smaller devices are exercised on this one (tests/test_gpu_parity.py)
    if (const char *lim = getenv("XSKNF_GPU_CU_LIMIT")) {
      const int l = atoi(lim);
      if (l > 0 && l < cus) {
        // a stray value would quietly slow every launch: say so, once per device
        fprintf(stderr, "libxsknf_gpu: XSKNF_GPU_CU_LIMIT=%d (test only): grids sized for %d of device %d's %d CUs\n",
                l, l, dev, cus);
        cus = l;
      }
    }
    cache[dev] = cus;
  }
  return cache[dev];
}

// Persistent grid: enough blocks for every tile, but never more than are
// resident at once (occupancy by VGPR / LDS of the instantiation), capped by
// blocks_per_cu.  A grid larger than residency would run in rounds with an
// idle tail, since tiles are dealt to waves statically.
int resident_blocks(const void *kernel, int threads) {
  struct Entry { const void *k; int dev; int blocks; };
  static thread_local Entry cache[64];
  static thread_local int used = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  for (int i = 0; i < used; ++i)
    if (cache[i].k == kernel && cache[i].dev == dev) return cache[i].blocks;
  int b = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kernel, threads, 0) != hipSuccess || b <= 0) b = 1;
  ab_note_occupancy(kernel, threads, b);
  if (used < 64) cache[used++] = Entry{kernel, dev, b};
  return b;
}

template <typename K>
uint32_t grid_blocks(K kernel, uint32_t n, int blocks_per_cu, uint32_t tile_frames, int waves_per_block = kWavesPerBlock) {
  const int resident = resident_blocks(reinterpret_cast<const void *>(kernel), waves_per_block * kWave);
  const int per_cu = blocks_per_cu < resident ? blocks_per_cu : resident;
  const uint32_t tiles = (n + tile_frames - 1) / tile_frames;
  const uint32_t need = (tiles + waves_per_block - 1) / waves_per_block;
  const uint32_t cap = static_cast<uint32_t>(device_cus() * per_cu);
  return need < cap ? need : cap;
}

int resident_blocks_per_cu() { return resident_blocks(reinterpret_cast<const void *>(resident_kernel), kBlock); }
int device_cu_count() { return device_cus(); }

int launch_resident(const ResArgs &ra, hipStream_t stream) {
  if (ra.blocks == 0 || ra.blocks > kResMaxBlocks) { set_error_text("resident_kernel: bad grid"); return -EINVAL; }
  hipLaunchKernelGGL(resident_kernel, dim3(ra.blocks), dim3(kBlock), 0, stream, ra);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(e, "resident_kernel launch"); return -EIO; }
  return 0;
}

int finish_launch(const KernelArgs &a, hipStream_t stream, const char *what) {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && a.defer_min_len != kNoDefer && !a.no_scatter && !a.tail_scatter) {
    const uint32_t need = (4 * a.n + kBlock - 1) / kBlock;   // dense shape: 4 lanes per frame
    const int bpc = ab_scatter_bpc(8);   // scatter blocks per CU
    const uint32_t cap = static_cast<uint32_t>(device_cus() * bpc);
    hipLaunchKernelGGL(scatter_checks, dim3(need < cap ? need : cap), dim3(kBlock), 0, stream, a);
    e = hipGetLastError();
    what = "scatter_checks launch";
  }
  if (e != hipSuccess) { set_error(e, what); return -EIO; }
  return 0;
}

template <int LPF, int NCH, int SPT>
int launch_reg(const KernelArgs &a, hipStream_t stream, int blocks_per_cu) {
  auto k = checksum_kernel<LPF, NCH, SPT>;
  hipLaunchKernelGGL(k, dim3(grid_blocks(k, a.n, blocks_per_cu, SPT * (kWave / LPF))), dim3(kBlock), 0, stream, a);
  return finish_launch(a, stream, "checksum_kernel launch");
}

// Whether the device can make one block of `threads` threads of `kernel`
// resident (a block holding a whole CU's waves and ~160 KiB of LDS may not
// fit): asked once per thread and kernel.
bool block_fits(const void *kernel, int threads) {
  struct Entry { const void *k; bool fits; };
  static thread_local Entry cache[16];
  static thread_local int used = 0;
  for (int i = 0; i < used; ++i)
    if (cache[i].k == kernel) return cache[i].fits;
  int b = 0;
  const bool fits = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kernel, threads, 0) == hipSuccess && b > 0;
  (void)hipGetLastError();
  if (used < 16) cache[used++] = Entry{kernel, fits};
  return fits;
}

template <int NCH, int SPT, int SW = kWavesPerBlock, int WPE = 1, int TLM = 0>
int launch_lane(const KernelArgs &a, hipStream_t stream, int blocks_per_cu) {
  auto k = checksum_kernel_lane<NCH, SPT, SW, WPE, TLM>;
  if constexpr (SW > kWavesPerBlock) {   // as launch_split: a CU-sized block the device cannot hold
    if (!block_fits(reinterpret_cast<const void *>(k), SW * kWave))
      return launch_lane<NCH, SPT, kWavesPerBlock>(a, stream, blocks_per_cu);
  }
  hipLaunchKernelGGL(k, dim3(grid_blocks(k, a.n, blocks_per_cu, SPT * kWave, SW)), dim3(SW * kWave), 0, stream, a);
  return finish_launch(a, stream, "checksum_kernel_lane launch");
}

template <int W, int LPF, int NCH, int U, bool TL, int SW = kWavesPerBlock>
int launch_split(const KernelArgs &a, hipStream_t stream, int blocks_per_cu) {
  auto k = checksum_kernel_split<W, LPF, NCH, U, TL, SW>;
  if constexpr (SW > kWavesPerBlock) {
    // a block holding a whole CU's waves (and ~160 KiB of LDS) that the device
    // cannot make resident runs as the 4-wave shape with the static schedule
    if (!block_fits(reinterpret_cast<const void *>(k), SW * kWave))
      return launch_split<W, LPF, NCH, U, TL, kWavesPerBlock>(a, stream, blocks_per_cu);
  }
  uint32_t grid = grid_blocks(k, a.n, blocks_per_cu, kWave, SW);
  constexpr uint32_t PT = patch_list_tiles<W, NCH, U, pooled_split(SW)>();
  if constexpr (PT > 0) {
    // Enough blocks that every tile's check goes to a patch list, whatever
    // blocks_per_cu asks or the device's CU count (blocks past residency start
    // as others end): the static schedule deals each wave every waves-th tile,
    // at most PT of them; a pool block's units (its tiles, the last SW of them
    // halved) are at most SW x PT, and a wave with a full list claims no more.
    // (Kept from the investigation of the GPU suites' illegal-address faults,
    // whose cause was HIP's locked-pageable-memory copy in the test process,
    // not these kernels -- DESIGN 3; tested by test_no_wave_passes_its_patch_list.)
    if (a.tail_scatter && !ab_no_grid_bound()) {   // (A/B builds can leave it out to exercise the guard)
      const uint32_t tiles = (a.n + kWave - 1) / kWave;
      // (a pool block of bt >= k * SW tiles has bt + (parts - 1) * k * SW units,
      // k * SW of them split, and its waves' lists hold SW * PT: so at most
      // SW * (PT - (parts - 1) * k) tiles -- the jumbo shape's 20-unit lists with
      // the last 3 SW tiles in quarters hold 88 tiles (64 at 1M frames on 256
      // CUs); until round 5 the bound was SW * (PT - 1), 120)
      constexpr uint32_t per_block = pooled_split(SW) ? pool_block_tiles_max(W, SW, PT) : SW * PT;
      const uint32_t fit = (tiles + per_block - 1) / per_block;
      if (grid < fit) grid = fit;
    }
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(SW * kWave), 0, stream, a);
  return finish_launch(a, stream, "checksum_kernel_split launch");
}




// Instantiated launch shapes: {lanes per frame, 16-B chunks per lane and pass,
// frames per group and step (register) / items per group in flight (split),
// kernel family, window field (header window chunks + the kWin flags)}.
struct Variant {
  int lpf, nch, u;
  int (*fn)(const KernelArgs &, hipStream_t, int);
  int kernel = XSKNF_GPU_KERNEL_AUTO, window = 0;
};

#define XSKNF_V(L, N, S) {L, N, S, &launch_reg<L, N, S>}
#define XSKNF_L(N, S) {1, N, S, &launch_lane<N, S>}
// ... transposed per tile where the tile's frames lie apart
#define XSKNF_LA(N, S) {1, N, S, &launch_lane<N, S, kWavesPerBlock, 4, 2>, XSKNF_GPU_KERNEL_AUTO, kWinLanePerTile}
// split: window field = W, + kWinTransposed for the transposed (coalesced) window load
#define XSKNF_S(W, L, N, U, TL) \
  {L, N, U, &launch_split<W, L, N, U, TL>, XSKNF_GPU_KERNEL_SPLIT, W + kWinTransposed * TL}
// one 12-wave block per CU, its waves drawing the CU's tiles from a shared pool (+ kWinPool)
#define XSKNF_SC(L, N, U) \
  {L, N, U, &launch_split<8, L, N, U, true, 12>, XSKNF_GPU_KERNEL_SPLIT, 8 + kWinTransposed + kWinPool}
// jumbo: one 8-wave block per CU (174 VGPRs: 2 waves per SIMD), W = 4
#define XSKNF_SC4(L, N, U) \
  {L, N, U, &launch_split<4, L, N, U, true, 8>, XSKNF_GPU_KERNEL_SPLIT, 4 + kWinTransposed + kWinPool}
const Variant kVariants[] = {
    // the product's shapes: default_cfg()'s split kernels, one per size class ...
    XSKNF_S(4, 16, 2, 2, 1), XSKNF_S(8, 16, 2, 2, 1), XSKNF_SC(16, 2, 2), XSKNF_S(8, 16, 3, 1, 1),
    XSKNF_S(4, 16, 3, 2, 1), XSKNF_SC4(16, 3, 2),
    // ... the lane kernel for short frames: windows loaded transposed where a
    // tile's frames lie apart (the default since round 5), and per lane ...
    XSKNF_LA(5, 2), XSKNF_L(5, 2),
    // ... and the zero-copy host path's small-batch group shapes (host_path.hip)
    XSKNF_V(32, 3, 2), XSKNF_V(64, 2, 4),
    XSKNF_AB_VARIANTS   // (A/B builds only: checksummer_ab.h)
};
#undef XSKNF_V
#undef XSKNF_L
#undef XSKNF_LA
#undef XSKNF_S
#undef XSKNF_SC
#undef XSKNF_SC4

const Variant *find_variant(const xsknf_gpu_launch_cfg &c) {
  for (const Variant &v : kVariants) {
    if (v.kernel != c.kernel) continue;
    if (v.kernel == XSKNF_GPU_KERNEL_SPLIT) {
      if (v.lpf == c.lanes_per_frame && v.nch == c.chunks_per_lane && v.u == c.frames_per_group &&
          v.window == c.window_chunks)
        return &v;
    } else if (v.lpf == c.lanes_per_frame && v.nch == c.chunks_per_lane &&
               v.u == c.frames_per_group && v.window == (c.window_chunks & ~(kWinPool - 1))) {
      return &v;
    }
  }
  return nullptr;
}

// Mean frame length under which a batch of <= 4 KiB frames keeps 4-wave blocks
// and the static schedule (0 = unknown: the CU-wide pool).  16 x 3 items (two
// in flight, 188 VGPRs: 2 waves per SIMD) for batches of mean >= 1280 B
// measured 1500 B 283.0 vs 287.7 us against 4-wave 16 x 2 (profiles/r02/
// ab_nch3.jsonl), but one launch of it over a batch larger than its patch
// lists faulted once in the full GPU suite and could not be reproduced alone,
// so it stays an A/B shape.
constexpr uint32_t kPoolMinMean = 512;

// Default shape for a batch whose longest frame is `hint` bytes and whose
// mean length is `mean` (0 = unknown: the shape that suits any mix).
void default_cfg(uint32_t hint, xsknf_gpu_launch_cfg &c, uint32_t mean) {
  c.frames_per_group = 4;
  c.blocks_per_cu = 8;
  c.lds_ring = 0;
  // measured best per size class on MI355X (tools/tune.py, 1M-frame batches,
  // launches rotating over enough batches that none is still in the 256 MiB
  // Infinity Cache from its previous pass -- bench.py's rotation):
  //  * hint <= 128: the lane kernel (one lane per frame, 5-chunk window), every
  //    check in-line as its whole 64-byte sector, non-temporal: 64 B 57.6 us
  //    [split kernel 60.3-61.3]; round 5: written through where a tile's frames
  //    lie apart, and there the windows loaded transposed (one request per
  //    frame): 56.7-57.1 vs 58.2-58.8 (profiles/r05/ab/ab_matrix_r05l.jsonl);
  //  * <= 4 KiB: the split kernel, 8-chunk window (the frame's whole first
  //    128-byte line, so phase B never refetches it), 16 x 2 items, two in
  //    flight, every check deferred and patched once the stream is done
  //    (no second launch; round 4: the pooled blocks from one queue): 570 B 148.8 us
  //    [in-line 170.2], IMIX 117.8 [per-tile policy + scatter pass 125-136,
  //    all in-line 127], 1500 B 291.6-292.5 [16 x 3 items + scatter pass
  //    294.4-297.4]; one 12-wave block per CU whose waves share the CU's
  //    tiles (window + 32), same process, interleaved: 1500 B 283.4 vs 292.6,
  //    1024 B 201.5 vs 206.8, 570 B 148.7 vs 150.1, IMIX 115.8 vs 114.8
  //    (profiles/r02/ab_pool.jsonl);
  //  * jumbo: 4-chunk window, 16 x 3 items, two per group in flight, the
  //    per-tile policy + scatter pass: 9000 B 1467 us [tail patches 1491];
  //    one 8-wave block per CU with the tile pool (+ 32): 1456 vs 1466 [12-wave
  //    blocks 1520; tail patches 1598] (profiles/r02/ab_pool_jumbo.jsonl);
  //    round 5: every check deferred and patched from the block's queue
  //    (2 + 16, no scatter launch): 1448-1449 vs 1456-1458 (profiles/r05/ab/).
  c.kernel = XSKNF_GPU_KERNEL_SPLIT;
  c.lanes_per_frame = 16;
  if (hint <= 128) {
    c.kernel = XSKNF_GPU_KERNEL_AUTO;
    // (+ kWinLanePerTile: windows loaded transposed where a tile's frames lie apart; 3
    // blocks per CU of the 4 that fit: 64 B 56.7-57.1 vs 56.8-57.2 us, packed
    // 64 B NIC 20.2-20.3 vs 22.5-22.8, nothing slower -- ab_lane_bpc_r05z.jsonl)
    c.lanes_per_frame = 1; c.window_chunks = kWinLanePerTile; c.chunks_per_lane = 5; c.frames_per_group = 2;
    c.fused_stores = kStoreInline;
    c.blocks_per_cu = 3;
  } else if (hint + 15 <= 4096) {
    // the CU-wide tile pool (+ 32) but for a known mix of mostly short frames
    // (IMIX: 115.9 vs 114.3 us with 4-wave blocks and the static schedule)
    c.window_chunks = 8 + kWinTransposed + (mean != 0 && mean < kPoolMinMean ? 0 : kWinPool);
    c.chunks_per_lane = 2; c.frames_per_group = 2; c.fused_stores = kStoreDeferred + kStoreTailPatch;
  } else {
    c.window_chunks = 4 + kWinTransposed + kWinPool; c.chunks_per_lane = 3; c.frames_per_group = 2;
    c.fused_stores = kStoreDeferred + kStoreTailPatch;
  }
}

int prepare(KernelArgs &a, uint8_t *umem, uint64_t umem_size, const xsknf_gpu_desc *descs, uint32_t n,
            uint32_t ingress_ifindex, const xsknf_csum_opts *opts, int32_t *verdicts) {
  if (!opts || opts->reserved != 0) return -EINVAL;
  if (opts->action != XSKNF_CSUM_ACTION_REDIRECT && opts->action != XSKNF_CSUM_ACTION_DROP) return -EINVAL;
  if (opts->action == XSKNF_CSUM_ACTION_REDIRECT && opts->num_interfaces == 0) return -EINVAL;
  if (n == 0) return 1;
  if (!umem || !descs || !verdicts) return -EINVAL;
  a.umem = umem;
  a.umem_size = umem_size;
  a.descs = descs;
  a.verdicts = verdicts;
  a.n = n;
  a.payload_mult = opts->csum_iterations > 0 ? static_cast<uint32_t>(opts->csum_iterations) : 0u;
  a.fwd_verdict = opts->action == XSKNF_CSUM_ACTION_REDIRECT
                      ? static_cast<int32_t>((ingress_ifindex + 1u) % opts->num_interfaces)
                      : -1;
  a.defer_min_len = kDeferMinLen;
  a.no_scatter = 0;
  a.sector_stores = 1;
  a.plain_sector = 0;
  a.tail_scatter = 0;
  a.store_unchanged = 0;
  a.seq = 0;
  a.count_records = 0;
  // aligned-down descriptor address: inside the descriptor array's own page
  a.dummy = reinterpret_cast<const uint4 *>(reinterpret_cast<uintptr_t>(descs) & ~static_cast<uintptr_t>(15));
  return 0;
}

constexpr uint32_t kLaunchFrames = 1u << 20;
constexpr uint32_t kLaneLaunchFrames = 1u << 24;
constexpr uint32_t kLaneTransposedMaxFrames = 2u << 20;

// cfg.fused_stores (the kStore constants) as the kernels' flags: which checks are
// deferred, and who writes the deferred ones -- the split kernel's own patches,
// the scatter pass (which then needs the records counted), or the caller.
void set_store_mode(KernelArgs &a, int fused_stores, bool split_kernel) {
  const int mode = fused_stores & kStoreModeMask;
  a.defer_min_len = mode == kStoreInline ? kNoDefer : (mode == kStorePerTile ? kDeferMinLen : 0u);
  if (mode == kStoreRecordsOnly) a.no_scatter = 1;
  if (fused_stores & kStoreTwoByte) a.sector_stores = 0;
  if (fused_stores & kStorePlainSector) a.plain_sector = 1;
  if (fused_stores & kStoreUnchanged) a.store_unchanged = 1;
  const bool deferred_here = a.defer_min_len != kNoDefer && !a.no_scatter;
  // (the patch list indexes 64-byte sectors in 32 bits: a larger UMEM parks its
  // checks for the scatter pass instead)
  a.tail_scatter = deferred_here && (fused_stores & kStoreTailPatch) && split_kernel && a.umem_size < kPatchMaxUmem;
  a.count_records = deferred_here && !a.tail_scatter;
}

int run(const KernelArgs &base, const xsknf_gpu_launch_cfg &cfg, void *stream, bool product_shape) {
  if (cfg.blocks_per_cu < 0 || cfg.blocks_per_cu > 64) return -EINVAL;
  if (cfg.fused_stores < 0 || cfg.fused_stores > kStoreAllBits) return -EINVAL;
  if (cfg.lds_ring != 0) return -EINVAL;   // (the LDS-DMA kernels it selected were removed in round 5)
  const Variant *v = find_variant(cfg);
  if (!v) return -EINVAL;
  KernelArgs a = base;
  set_store_mode(a, cfg.fused_stores, v->kernel == XSKNF_GPU_KERNEL_SPLIT);
  // A batch larger than kLaunchFrames runs as consecutive launches of that many
  // frames: one launch over the whole of an 8M-frame IMIX batch (config 4 on
  // one GPU, 16 GB of UMEM) takes 133 us per 1M frames against 113 for 1M-frame
  // launches -- the waves' tiles drift apart over a long static schedule, and
  // the pages in use with them.
  static std::atomic<uint32_t> seq{0};
  // The lane kernel (frames <= 128 B) goes the other way: one launch over a
  // larger batch pays one ramp and one drain for all of it -- 64 B, 13M frames
  // 50.2 us per 1M frames in one launch against 58.6 in 13 launches, 4M 55.4
  // against 57.9 (profiles/r05/ab/ab_lane_launch_frames.jsonl).
  const uint32_t lf = v->lpf == 1 && v->kernel != XSKNF_GPU_KERNEL_SPLIT ? kLaneLaunchFrames : kLaunchFrames;
  // The lane kernel's per-tile transposed windows (kWinLanePerTile) pay off
  // in a launch of up to a few M frames, per-lane loads in a longer one (64 B,
  // profiles/r05/ab/ab_lane_la_r05n.jsonl: 1M frames 57.5-57.7 vs 58.3-59.0 us,
  // 13M frames in one launch 701-710 vs 655-662 us): a longer launch runs as
  // the per-lane shape.
  // Only for the product's own shape (default_cfg, or an explicit cfg that leaves
  // blocks_per_cu to the library): an explicit shape runs as asked.
  const Variant *longer = v;
  if (product_shape && v->kernel == XSKNF_GPU_KERNEL_AUTO && v->lpf == 1 && v->window == kWinLanePerTile) {
    xsknf_gpu_launch_cfg c = cfg;
    c.window_chunks = 0;
    if (const Variant *w = find_variant(c)) longer = w;
  }
  for (uint32_t off = 0; off < base.n; off += lf) {
    KernelArgs p = a;
    p.descs = base.descs + off;
    p.verdicts = base.verdicts + off;
    p.n = base.n - off < lf ? base.n - off : lf;
    p.seq = seq.fetch_add(1, std::memory_order_relaxed);
    const Variant *lv = p.n > kLaneTransposedMaxFrames ? longer : v;
    // (and a longer launch as many blocks per CU as fit: 13M frames 660 us at
    // 4 per CU against 695-699 at the 3 of the default lane shape,
    // profiles/r05/ab/ab_lane_bpc_r05z*.jsonl)
    const int bpc = lv != v ? 8 : (cfg.blocks_per_cu ? cfg.blocks_per_cu : 8);
    const int rc = lv->fn(p, static_cast<hipStream_t>(stream), bpc);
    if (rc) return rc;
  }
  return 0;
}

}  // namespace xsknf_gpu

extern "C" {

uint32_t xsknf_gpu_version(void) { return (0u << 16) | 1u; }

int xsknf_gpu_device_count(int *count) {
  if (!count) return -EINVAL;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess || *count < 1) {
    const int seen = e == hipSuccess ? *count : 0;
    *count = 0;
    return xsknf_gpu::set_device_error(e, seen, "hipGetDeviceCount");
  }
  return 0;
}

const char *xsknf_gpu_last_error(void) { return xsknf_gpu::last_error_copy(); }

int xsknf_gpu_checksum_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
                             uint32_t n, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
                             int32_t *verdicts, uint32_t frame_len_hint, void *stream) {
  xsknf_gpu::KernelArgs a;
  const int rc = xsknf_gpu::prepare(a, umem, umem_size, descs, n, ingress_ifindex, opts, verdicts);
  if (rc != 0) return rc < 0 ? rc : 0;
  xsknf_gpu_launch_cfg cfg;
  xsknf_gpu::default_cfg(frame_len_hint ? frame_len_hint : 2048u, cfg);
  return xsknf_gpu::run(a, cfg, stream, true);
}

int xsknf_gpu_checksum_batch_cfg(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
                                 uint32_t n, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
                                 int32_t *verdicts, const struct xsknf_gpu_launch_cfg *cfg, void *stream) {
  if (!cfg) return -EINVAL;
  xsknf_gpu::KernelArgs a;
  const int rc = xsknf_gpu::prepare(a, umem, umem_size, descs, n, ingress_ifindex, opts, verdicts);
  if (rc != 0) return rc < 0 ? rc : 0;
  return xsknf_gpu::run(a, *cfg, stream, cfg->blocks_per_cu == 0);
}

int xsknf_gpu_default_launch_cfg(uint32_t frame_len_hint, struct xsknf_gpu_launch_cfg *cfg) {
  if (!cfg) return -EINVAL;
  xsknf_gpu::default_cfg(frame_len_hint ? frame_len_hint : 2048u, *cfg);
  return 0;
}

int xsknf_gpu_checksum_batch_lens(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
                                  uint32_t n, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
                                  int32_t *verdicts, uint32_t frame_len_max, uint32_t frame_len_mean,
                                  void *stream) {
  xsknf_gpu::KernelArgs a;
  const int rc = xsknf_gpu::prepare(a, umem, umem_size, descs, n, ingress_ifindex, opts, verdicts);
  if (rc != 0) return rc < 0 ? rc : 0;
  xsknf_gpu_launch_cfg cfg;
  xsknf_gpu::default_cfg(frame_len_max ? frame_len_max : 2048u, cfg, frame_len_mean);
  return xsknf_gpu::run(a, cfg, stream, true);
}

int xsknf_gpu_launch_cfg_for_lens(uint32_t frame_len_max, uint32_t frame_len_mean,
                                  struct xsknf_gpu_launch_cfg *cfg) {
  if (!cfg) return -EINVAL;
  xsknf_gpu::default_cfg(frame_len_max ? frame_len_max : 2048u, *cfg, frame_len_mean);
  return 0;
}

int xsknf_gpu_pool_guard_trips(uint32_t *trips, int reset) {
  if (!trips) return -EINVAL;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyFromSymbol(trips, HIP_SYMBOL(xsknf_gpu::g_pool_guard_trips), sizeof(*trips));
  if (e == hipSuccess && reset) {
    const uint32_t zero = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(xsknf_gpu::g_pool_guard_trips), &zero, sizeof(zero));
  }
  if (e != hipSuccess) {
    xsknf_gpu::set_error(e, "xsknf_gpu_pool_guard_trips");
    return -EIO;
  }
  return 0;
}

#ifdef XSKNF_GUARD
// Debug instrument: the guard buffer (u64: [0] count, [1..6] allowed ranges,
// records from [8]; NULL: off).  Not in the product library.
__attribute__((visibility("default"))) int xsknf_gpu_ab_set_guard(void *buf) {
  unsigned long long *p = static_cast<unsigned long long *>(buf);
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(xsknf_gpu::g_guard), &p, sizeof(p));
  return e == hipSuccess ? 0 : -EIO;
}
#endif

#ifdef XSKNF_TIMELINE
// A/B instrument: the split kernel's per-wave timeline goes to `buf` (4 u64
// per wave; NULL: off).  Not in the product library.
__attribute__((visibility("default"))) int xsknf_gpu_ab_set_timeline(void *buf) {
  unsigned long long *p = static_cast<unsigned long long *>(buf);
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(xsknf_gpu::g_timeline), &p, sizeof(p));
  return e == hipSuccess ? 0 : -EIO;
}
#endif

}  // extern "C"
