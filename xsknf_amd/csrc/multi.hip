// multi.hip -- one process over N devices: config 4's global batch, sharded.
//
// The reference scales one worker per NIC queue (src/xsknf.c:992, the worker
// loop started per queue at :1046-1100): frames never cross workers, so its
// parallelism is independent batches.  On a node of MI355X the same holds per
// device, and the per-worker hook (host_path.hip: worker w on device
// w % devices) is that model.  This file adds what a C host needs when a
// global batch starts on ONE device (BASELINE config 4):
//
//   * xsknf_gpu_shard_plan  -- contiguous descriptor ranges balanced by frame
//     bytes (the kernel is HBM-bound: bytes set each device's time), and the
//     UMEM byte span of each range; the same cuts as xsknf_amd/shard.py.
//   * xsknf_gpu_multi_create -- one RCCL communicator per device
//     (ncclCommInitAll: one process drives every device), a stream each.
//   * xsknf_gpu_multi_scatter -- each shard moved from the root device as ONE
//     span of UMEM bytes plus its rebased descriptors, by grouped ncclSend /
//     ncclRecv: every peer's transfer at once, each on its own xGMI link (the
//     root's own shard too, as a send to itself, so the path is the same at
//     N = 1).  A point-to-point pattern, not a ring collective.
//   * xsknf_gpu_multi_process -- the checksummer on every device's shard, each
//     on its own stream, all in flight together (no data-path collective).
//   * xsknf_gpu_multi_counters -- {frames, bytes, drops, forwards, sum of the
//     written checks, the same weighted by global UMEM offset} per device,
//     summed over devices by ncclAllReduce: the whole batch's result, as one
//     device's pass over all of it would give it.
//   * xsknf_gpu_multi_scatter_packed -- the same distribution moving only the
//     frames' bytes: a gather kernel on the root copies each shard's frames
//     into 16-byte slots (a frame keeps its address mod 16), so a UMEM of 2 KiB
//     chunks holding IMIX frames (mean 352 B) sends ~1/5 of its span bytes.
//   * xsknf_gpu_multi_return -- the results back to the root: each device runs
//     the summing pass in records-only mode over its shard (include/
//     xsknf_gpu.h fused_stores 3: the shard is only read), sends its 4-byte
//     records / verdicts to the root (grouped ncclSend / ncclRecv), and an apply
//     kernel on the root writes every changed check into the root's UMEM and
//     every final verdict: the root ends with the bytes and verdicts of one
//     device's pass over the whole batch, having moved frames out and 4 bytes
//     per frame back.
//   * xsknf_gpu_multi_scatter_dev -- either scatter for descriptors that lie on
//     the root device: planned there (plan_device.hip) instead of on the host,
//     then the same placement and moves (place_shards / send_shards below).
// Host code only: the kernels (shard_counters, pack_frames, apply_records) are kernel_pack.h's.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <time.h>
#include <new>
#include <vector>

#include "../../include/xsknf_gpu.h"
#include "checksummer_internal.h"
#include "kernel_pack.h"
#include "plan_device.h"

namespace {

using namespace xsknf_gpu::multi;

// Bytes per ncclSend / ncclRecv of a scatter.  One ncclSend of a whole span
// past 1 GiB delivered only part of it with this image's RCCL (a send to self
// of the 2 GiB and 16 GiB spans of 1M and 8M IMIX frames: the bytes from 1 GiB
// on -- from 2 GiB on in 4 GiB pieces -- never arrived, while the calls and the
// group returned success); 256 MiB pieces delivered every byte
// (profiles/r06/multi_p2p_pieces.jsonl; the probe, with the piece size as an
// environment knob, is in commit cca61bb's tools/diag_multi_p2p.py).
constexpr uint64_t kP2PPiece = 1ull << 28;

int nccl_fail(ncclResult_t r, const char *where) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", where, ncclGetErrorString(r));
  xsknf_gpu::set_error_text(buf);
  return -EIO;
}

int hip_fail(hipError_t e, const char *where) {
  xsknf_gpu::set_error(e, where);
  return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + ts.tv_nsec * 1e-9;
}

// Blocks of 256 threads for n items, one each, at most `cap` (the kernels stride).
unsigned grid_for(uint64_t n, uint64_t cap) {
  const uint64_t want = (n + 255) / 256;
  return static_cast<unsigned>(want < cap ? want : cap);
}

struct Shard {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint64_t lo = 0, hi = 0;       // frames [lo, hi) of the global batch
  uint64_t b0 = 0, b1 = 0;       // its UMEM byte span on the root (packed: 0 and its packed bytes)
  uint64_t bytes = 0;            // sum of the shard's frame lengths
  uint8_t *umem = nullptr;       // b1 - b0 bytes + 16 spare (the kernels' 16-byte chunk loads), inside umem_alloc
  uint8_t *umem_alloc = nullptr; // at the root's address mod kPlace (span scatter): the same placement as there
  uint64_t umem_cap = 0;
  xsknf_gpu_desc *descs = nullptr;
  int32_t *verdicts = nullptr;
  uint64_t frames_cap = 0;
  unsigned long long *counters = nullptr;   // device: XSKNF_GPU_MULTI_COUNTERS
};

}  // namespace

struct xsknf_gpu_multi {
  int ndev = 0;
  std::vector<int> devices;
  std::vector<ncclComm_t> comms;
  std::vector<Shard> sh;
  xsknf_gpu_desc *root_descs = nullptr;   // the rebased descriptors of every shard, on the root device
  uint64_t root_descs_cap = 0;
  int root_descs_dev = -1;                // the device root_descs lives on
  int root = -1;                          // index of the root of the last scatter
  uint64_t n = 0;                         // frames of the last scatter
  bool packed = false;                    // the last scatter moved packed frames
  bool processed = false;                 // _process wrote checks into the shards since the last scatter
  // on the root device (root_descs_dev): the last scatter's descriptors as the
  // caller gave them (for the results' return) and the packed staging buffer
  xsknf_gpu_desc *root_orig = nullptr;
  uint64_t root_orig_cap = 0;
  uint8_t *root_pack = nullptr;
  uint64_t root_pack_cap = 0;
  // the device planner's workspace (xsknf_gpu_multi_scatter_dev), on the root device too
  uint8_t *root_plan = nullptr;
  uint64_t root_plan_cap = 0;
};

namespace {

// (Re)allocate a root-device buffer to at least `bytes`.
template <typename T>
hipError_t root_buffer(T *&p, uint64_t &cap, uint64_t bytes) {
  if (p && bytes <= cap) return hipSuccess;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), bytes ? bytes : 1);
  if (e == hipSuccess) cap = bytes;
  return e;
}

// The root-side buffers of a scatter: the device the root buffers live on
// becomes devices[root] (buffers of an earlier root are freed), root_orig and
// root_descs hold n descriptors each.
hipError_t root_prepare(xsknf_gpu_multi *m, int root, uint64_t n) {
  hipError_t e = hipSuccess;
  if (m->root_descs_dev >= 0 && m->root_descs_dev != m->devices[root]) {
    e = hipSetDevice(m->root_descs_dev);
    for (void *p : {static_cast<void *>(m->root_descs), static_cast<void *>(m->root_orig),
                    static_cast<void *>(m->root_pack), static_cast<void *>(m->root_plan)})
      if (e == hipSuccess && p) e = hipFree(p);
    m->root_descs = m->root_orig = nullptr;
    m->root_pack = m->root_plan = nullptr;
    m->root_descs_cap = m->root_orig_cap = m->root_pack_cap = m->root_plan_cap = 0;
  }
  if (e == hipSuccess) e = hipSetDevice(m->devices[root]);
  m->root_descs_dev = m->devices[root];
  const uint64_t bytes = sizeof(xsknf_gpu_desc) * n;
  uint64_t cap_d = m->root_descs_cap * sizeof(xsknf_gpu_desc), cap_o = m->root_orig_cap * sizeof(xsknf_gpu_desc);
  if (e == hipSuccess) e = root_buffer(m->root_descs, cap_d, bytes);
  if (e == hipSuccess) e = root_buffer(m->root_orig, cap_o, bytes);
  m->root_descs_cap = cap_d / sizeof(xsknf_gpu_desc);
  m->root_orig_cap = cap_o / sizeof(xsknf_gpu_desc);
  return e;
}

// The root-side staging of a scatter from host descriptors: the caller's
// descriptors go to root_orig (for the results' return) and `sent` (the
// descriptors each shard receives, in global order) to root_descs.
hipError_t stage_root(xsknf_gpu_multi *m, int root, const xsknf_gpu_desc *descs, const xsknf_gpu_desc *sent,
                      uint64_t n) {
  hipError_t e = root_prepare(m, root, n);
  const uint64_t bytes = sizeof(xsknf_gpu_desc) * n;
  if (e == hipSuccess && n) e = hipMemcpy(m->root_descs, sent, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) e = hipMemcpy(m->root_orig, descs, bytes, hipMemcpyHostToDevice);
  return e;
}

// A shard's device buffers for `span` bytes (+ 16 spare: the kernels' 16-byte
// chunk loads) and `frames` descriptors / verdicts; the spare bytes zeroed.
// The span starts at address `place` mod kPlace, so that a shard of a UMEM's
// span keeps the placement its frames had on the root (the channels a frame's
// sectors fall on follow the address: config 4's 64-B frames at 2 KiB strides).
constexpr uint64_t kPlace = 4096;
hipError_t shard_buffers(Shard &s, uint64_t span, uint64_t frames, uint64_t place) {
  hipError_t e = hipSetDevice(s.device);
  const uint64_t need = span + 16 + kPlace;
  if (e == hipSuccess && need > s.umem_cap) {
    if (s.umem_alloc) (void)hipFree(s.umem_alloc);
    s.umem_alloc = s.umem = nullptr;
    s.umem_cap = 0;
    e = hipMalloc(&s.umem_alloc, need);
    if (e == hipSuccess) s.umem_cap = need;
  }
  if (e == hipSuccess) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(s.umem_alloc);
    s.umem = s.umem_alloc + ((place - a) & (kPlace - 1));
  }
  if (e == hipSuccess && frames > s.frames_cap) {
    if (s.descs) (void)hipFree(s.descs);
    if (s.verdicts) (void)hipFree(s.verdicts);
    s.descs = nullptr;
    s.verdicts = nullptr;
    s.frames_cap = 0;
    e = hipMalloc(&s.descs, sizeof(xsknf_gpu_desc) * (frames ? frames : 1));
    if (e == hipSuccess) e = hipMalloc(&s.verdicts, sizeof(int32_t) * (frames ? frames : 1));
    if (e == hipSuccess) s.frames_cap = frames;
  }
  if (e == hipSuccess) e = hipMemsetAsync(s.umem + span, 0, 16, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  return e;
}

// One grouped set of point-to-point moves, in kP2PPiece pieces: each
// (src on devices[from], dst on devices[to], bytes) as ncclSend on `from`'s
// communicator / stream and ncclRecv on `to`'s.
struct Move {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t bytes;
  int from, to;
};

int grouped_moves(xsknf_gpu_multi *m, const std::vector<Move> &moves, const char *what) {
  ncclResult_t r = ncclGroupStart();
  for (const Move &mv : moves)
    for (uint64_t o = 0; o < mv.bytes && r == ncclSuccess; o += kP2PPiece) {
      const size_t len = mv.bytes - o < kP2PPiece ? mv.bytes - o : kP2PPiece;
      r = ncclSend(mv.src + o, len, ncclUint8, mv.to, m->comms[mv.from], m->sh[mv.from].stream);
      if (r == ncclSuccess) r = ncclRecv(mv.dst + o, len, ncclUint8, mv.from, m->comms[mv.to], m->sh[mv.to].stream);
    }
  const ncclResult_t r2 = ncclGroupEnd();
  if (r != ncclSuccess) return nccl_fail(r, what);
  if (r2 != ncclSuccess) return nccl_fail(r2, what);
  for (Shard &s : m->sh) {
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) return hip_fail(e, what);
  }
  return 0;
}

// A scatter's plan as the host holds it, from shard_plan.cpp or the device
// planner: the cuts, each shard's span (2 per shard) or packed bytes (1 per
// shard), each shard's frame bytes.
struct Plan {
  bool packed;
  std::vector<uint64_t> bounds, ext, bytes;
  Plan(int N, bool pk) : packed(pk), bounds(N + 1), ext(pk ? N : 2 * N), bytes(N) {}
};

// The planned shards' fields and device buffers (packed: the root's staging
// buffer too; pk_lo[k] = shard k's place in it).  After the root's staging.
int place_shards(xsknf_gpu_multi *m, int root, const uint8_t *umem, const Plan &p, std::vector<uint64_t> &pk_lo) {
  const int N = m->ndev;
  if (p.packed) {
    // the root's own shard is packed straight into its shard buffer; the staging
    // buffer holds the others' (at N = 1 nothing is staged, nothing copied)
    uint64_t total = 0;
    pk_lo.assign(N, 0);
    for (int k = 0; k < N; ++k) {
      pk_lo[k] = k == root ? 0 : total;
      total += k == root ? 0 : p.ext[k];
    }
    hipError_t e = root_buffer(m->root_pack, m->root_pack_cap, total);
    if (e != hipSuccess) return hip_fail(e, "multi packed scatter: root buffers");
  }
  for (int k = 0; k < N; ++k) {
    Shard &s = m->sh[k];
    s.lo = p.bounds[k];
    s.hi = p.bounds[k + 1];
    s.b0 = p.packed ? 0 : p.ext[2 * k];
    s.b1 = p.packed ? p.ext[k] : p.ext[2 * k + 1];
    s.bytes = p.bytes[k];
    hipError_t e = shard_buffers(s, s.b1 - s.b0, s.hi - s.lo,
                                 p.packed ? 0 : reinterpret_cast<uintptr_t>(umem) + s.b0);
    if (e != hipSuccess)
      return hip_fail(e, p.packed ? "multi packed scatter: shard buffers" : "multi scatter: shard buffers");
  }
  return 0;
}

// The placed shards out of the root, root_descs and root_orig holding the
// batch: (packed) the gather of every shard's frames on the root, then every
// shard at once, one group.
int send_shards(xsknf_gpu_multi *m, int root, const uint8_t *umem, uint64_t umem_size, uint64_t n, const Plan &p,
                const std::vector<uint64_t> &pk_lo) {
  const int N = m->ndev;
  std::vector<Move> moves;
  if (p.packed) {
    // gather every shard's frames on the root, on the root's stream (its sends
    // follow on the same stream): the root's own into its shard buffer
    Shard &rs = m->sh[root];
    hipError_t e = hipSetDevice(rs.device);
    for (int k = 0; k < N && e == hipSuccess; ++k) {
      const uint64_t frames = p.bounds[k + 1] - p.bounds[k];
      if (!frames) continue;
      hipLaunchKernelGGL(pack_frames, dim3(grid_for(frames, 4096)), dim3(256), 0, rs.stream, umem, umem_size,
                         m->root_orig + p.bounds[k], m->root_descs + p.bounds[k], frames,
                         k == root ? rs.umem : m->root_pack + pk_lo[k]);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_fail(e, "multi packed scatter: pack_frames");
  }
  // the root sends each its span (packed: its packed frames) and descriptors,
  // every device receives its own; the root's own span and descriptors go as a
  // send to itself, so the path is the same at N = 1
  for (int k = 0; k < N; ++k) {
    Shard &s = m->sh[k];
    if (!p.packed)
      moves.push_back({umem + s.b0, s.umem, s.b1 - s.b0, root, k});
    else if (k != root)
      moves.push_back({m->root_pack + pk_lo[k], s.umem, p.ext[k], root, k});
    moves.push_back({reinterpret_cast<const uint8_t *>(m->root_descs + s.lo), reinterpret_cast<uint8_t *>(s.descs),
                     sizeof(xsknf_gpu_desc) * (s.hi - s.lo), root, k});
  }
  const int rc = grouped_moves(m, moves, p.packed ? "multi packed scatter: ncclSend / ncclRecv"
                                                  : "multi scatter: ncclSend / ncclRecv");
  if (rc) return rc;
  m->root = root;
  m->n = n;
  m->processed = false;
  m->packed = p.packed;
  return 0;
}

// xsknf_gpu_multi_scatter and _scatter_packed: the plan on the host, the
// descriptors every shard receives (rebased to its own span, or addressing its
// packed bytes) staged on the root in global order, the placement, the moves.
int scatter_host(xsknf_gpu_multi *m, int root, const uint8_t *umem, uint64_t umem_size, const xsknf_gpu_desc *descs,
                 uint64_t n, bool packed, double *seconds) {
  if (!m || root < 0 || root >= m->ndev || (n && (!umem || !descs))) return -EINVAL;
  const int N = m->ndev;
  Plan p(N, packed);
  int rc = xsknf_gpu_shard_plan(descs, n, umem_size, static_cast<uint32_t>(N), p.bounds.data(),
                                packed ? nullptr : p.ext.data());
  if (rc) return rc;
  std::vector<xsknf_gpu_desc> sent(n);
  if (packed) {
    rc = xsknf_gpu_shard_pack_plan(descs, n, reinterpret_cast<uintptr_t>(umem), umem_size, static_cast<uint32_t>(N),
                                   p.bounds.data(), sent.data(), p.ext.data());
    if (rc) return rc;
  } else {
    for (int k = 0; k < N; ++k)
      xsknf_gpu_shard_rebase(descs + p.bounds[k], p.bounds[k + 1] - p.bounds[k], p.ext[2 * k], umem_size,
                             sent.data() + p.bounds[k]);
  }
  hipError_t e = stage_root(m, root, descs, sent.data(), n);
  if (e != hipSuccess)
    return hip_fail(e, packed ? "multi packed scatter: root buffers" : "multi scatter: root descriptors");
  for (int k = 0; k < N; ++k)   // each shard's sum of frame lengths
    for (uint64_t f = p.bounds[k]; f < p.bounds[k + 1]; ++f) p.bytes[k] += descs[f].len;
  std::vector<uint64_t> pk_lo;
  rc = place_shards(m, root, umem, p, pk_lo);
  if (rc) return rc;
  const double t0 = now_s();
  rc = send_shards(m, root, umem, umem_size, n, p, pk_lo);
  if (rc) return rc;
  if (seconds) *seconds = now_s() - t0;
  return 0;
}

}  // namespace

extern "C" {

int xsknf_gpu_multi_create(struct xsknf_gpu_multi **out, const int *devices, int ndev) {
  if (!out || ndev < 1 || ndev > 64) return -EINVAL;
  *out = nullptr;
  int count = 0;
  const int rc = xsknf_gpu_device_count(&count);
  if (rc) return rc;
  std::vector<int> devs(ndev);
  for (int k = 0; k < ndev; ++k) {
    devs[k] = devices ? devices[k] : k;
    if (devs[k] < 0 || devs[k] >= count) return -EINVAL;
    for (int j = 0; j < k; ++j)
      if (devs[j] == devs[k]) return -EINVAL;   // one communicator rank per device
  }
  xsknf_gpu_multi *m = new (std::nothrow) xsknf_gpu_multi;
  if (!m) return -ENOMEM;
  m->ndev = ndev;
  m->devices = devs;
  m->comms.assign(ndev, nullptr);
  m->sh.resize(ndev);
  ncclResult_t r = ncclCommInitAll(m->comms.data(), ndev, devs.data());
  if (r != ncclSuccess) {
    delete m;
    return nccl_fail(r, "ncclCommInitAll");
  }
  for (int k = 0; k < ndev; ++k) {
    Shard &s = m->sh[k];
    s.device = devs[k];
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&s.e0);
    if (e == hipSuccess) e = hipEventCreate(&s.e1);
    if (e == hipSuccess) e = hipMalloc(&s.counters, sizeof(unsigned long long) * XSKNF_GPU_MULTI_COUNTERS);
    if (e != hipSuccess) {
      xsknf_gpu_multi_destroy(m);
      return hip_fail(e, "multi device setup");
    }
  }
  *out = m;
  return 0;
}

int xsknf_gpu_multi_scatter(struct xsknf_gpu_multi *m, int root, const uint8_t *umem, uint64_t umem_size,
                            const struct xsknf_gpu_desc *descs, uint64_t n, double *seconds) {
  return scatter_host(m, root, umem, umem_size, descs, n, false, seconds);
}

int xsknf_gpu_multi_scatter_packed(struct xsknf_gpu_multi *m, int root, const uint8_t *umem, uint64_t umem_size,
                                   const struct xsknf_gpu_desc *descs, uint64_t n, double *seconds) {
  return scatter_host(m, root, umem, umem_size, descs, n, true, seconds);
}

int xsknf_gpu_multi_scatter_dev(struct xsknf_gpu_multi *m, int root, const uint8_t *umem, uint64_t umem_size,
                                const struct xsknf_gpu_desc *descs_dev, uint64_t n, int mode, double *seconds,
                                double *plan_seconds) {
  if (!m || root < 0 || root >= m->ndev || (n && (!umem || !descs_dev))) return -EINVAL;
  if (mode != XSKNF_GPU_PLAN_SPAN && mode != XSKNF_GPU_PLAN_PACKED) return -EINVAL;
  if (reinterpret_cast<uintptr_t>(descs_dev) & 15) return -EINVAL;   // the planner's 16-byte loads
  const int N = m->ndev;
  const double t0 = now_s();
  Plan p(N, mode == XSKNF_GPU_PLAN_PACKED);
  const char *what = "multi device-planned scatter: root buffers";
  hipError_t e = root_prepare(m, root, n);
  if (e == hipSuccess) e = root_buffer(m->root_plan, m->root_plan_cap, xsknf_gpu::plan_dev_workspace_bytes(n));
  if (e != hipSuccess) return hip_fail(e, what);
  // the plan, straight into root_descs, on the root's stream
  Shard &rs = m->sh[root];
  const double tp = now_s();
  int rc = xsknf_gpu::plan_dev_run(descs_dev, n, reinterpret_cast<uintptr_t>(umem), umem_size,
                                   static_cast<uint32_t>(N), mode, m->root_descs, p.bounds.data(), p.ext.data(),
                                   p.bytes.data(), m->root_plan, rs.stream);
  if (rc) return rc;
  if (plan_seconds) *plan_seconds = now_s() - tp;
  // the caller's descriptors for the results' return (ahead of pack_frames on
  // the same stream; send_shards waits for the stream before it returns)
  if (n) e = hipMemcpyAsync(m->root_orig, descs_dev, sizeof(xsknf_gpu_desc) * n, hipMemcpyDeviceToDevice, rs.stream);
  if (e != hipSuccess) return hip_fail(e, "multi device-planned scatter: descriptor copy");
  std::vector<uint64_t> pk_lo;
  rc = place_shards(m, root, umem, p, pk_lo);
  if (rc) return rc;
  rc = send_shards(m, root, umem, umem_size, n, p, pk_lo);
  if (rc) return rc;
  if (seconds) *seconds = now_s() - t0;
  return 0;
}

int xsknf_gpu_multi_process(struct xsknf_gpu_multi *m, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
                            uint32_t frame_len_max, uint32_t frame_len_mean, float *ms) {
  if (!m || !opts || m->root < 0) return -EINVAL;
  // every device's launches first (all in flight together), then the waits
  for (Shard &s : m->sh) {
    const uint64_t frames = s.hi - s.lo;
    if (frames > UINT32_MAX) return -EINVAL;
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipEventRecord(s.e0, s.stream);
    if (e != hipSuccess) return hip_fail(e, "multi process: start");
    const int rc = xsknf_gpu_checksum_batch_lens(s.umem, s.b1 - s.b0, s.descs, static_cast<uint32_t>(frames),
                                                 ingress_ifindex, opts, s.verdicts, frame_len_max, frame_len_mean,
                                                 s.stream);
    if (rc) return rc;
    e = hipEventRecord(s.e1, s.stream);
    if (e != hipSuccess) return hip_fail(e, "multi process: end");
    m->processed = true;
  }
  for (int k = 0; k < m->ndev; ++k) {
    Shard &s = m->sh[k];
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipEventSynchronize(s.e1);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, s.e0, s.e1);
    if (e != hipSuccess) return hip_fail(e, "multi process: wait");
    if (ms) ms[k] = t;
  }
  return 0;
}

int xsknf_gpu_multi_counters(struct xsknf_gpu_multi *m, uint64_t *out) {
  if (!m || !out || m->root < 0) return -EINVAL;
  // the weighted check sum needs each frame's place in the root's UMEM, which
  // a packed shard no longer holds: after a packed scatter the results come
  // back whole (xsknf_gpu_multi_return) and are checked there
  if (m->packed) return -EOPNOTSUPP;
  for (Shard &s : m->sh) {
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess)
      e = hipMemsetAsync(s.counters, 0, sizeof(unsigned long long) * XSKNF_GPU_MULTI_COUNTERS, s.stream);
    const uint64_t frames = s.hi - s.lo;
    if (e == hipSuccess && frames) {
      hipLaunchKernelGGL(shard_counters, dim3(grid_for(frames, 2048)), dim3(256), 0, s.stream, s.umem, s.b1 - s.b0,
                         s.descs, s.verdicts, frames, s.b0, s.counters);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_fail(e, "multi counters: launch");
  }
  ncclResult_t r = ncclGroupStart();
  for (int k = 0; k < m->ndev && r == ncclSuccess; ++k)
    r = ncclAllReduce(m->sh[k].counters, m->sh[k].counters, XSKNF_GPU_MULTI_COUNTERS, ncclUint64, ncclSum,
                      m->comms[k], m->sh[k].stream);
  const ncclResult_t r2 = ncclGroupEnd();
  if (r != ncclSuccess) return nccl_fail(r, "multi counters: ncclAllReduce");
  if (r2 != ncclSuccess) return nccl_fail(r2, "multi counters: ncclGroupEnd");
  for (Shard &s : m->sh) {
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) return hip_fail(e, "multi counters: wait");
  }
  // every device holds the sum; the root's copy is the answer
  Shard &rs = m->sh[m->root];
  hipError_t e = hipSetDevice(rs.device);
  if (e == hipSuccess)
    e = hipMemcpy(out, rs.counters, sizeof(unsigned long long) * XSKNF_GPU_MULTI_COUNTERS, hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : hip_fail(e, "multi counters: copy");
}

int xsknf_gpu_multi_return(struct xsknf_gpu_multi *m, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
                           uint32_t frame_len_max, uint32_t frame_len_mean, uint8_t *umem, int32_t *verdicts, float *ms,
                           double *seconds) {
  if (!m || !opts || m->root < 0 || (m->n && (!umem || !verdicts))) return -EINVAL;
  // the records describe a pass over the frames as the scatter sent them: once
  // _process has rewritten checks in the shards, a second pass is not the same
  // (a frame whose UDP header overlaps its IP addresses, ihl 2 or 3, sums the
  // check it just wrote), so the caller scatters again
  if (m->processed) {
    xsknf_gpu::set_error_text("xsknf_gpu_multi_return: the shards were checksummed in place since the scatter");
    return -EBUSY;
  }
  xsknf_gpu_launch_cfg cfg;
  int rc = xsknf_gpu_launch_cfg_for_lens(frame_len_max, frame_len_mean, &cfg);
  if (rc) return rc;
  cfg.fused_stores = xsknf_gpu::kStoreRecordsOnly;   // the shard is read, each changed check comes back as a record
  const double t0 = now_s();
  for (Shard &s : m->sh) {
    const uint64_t frames = s.hi - s.lo;
    if (frames > UINT32_MAX) return -EINVAL;
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipEventRecord(s.e0, s.stream);
    if (e != hipSuccess) return hip_fail(e, "multi return: start");
    rc = xsknf_gpu_checksum_batch_cfg(s.umem, s.b1 - s.b0, s.descs, static_cast<uint32_t>(frames), ingress_ifindex,
                                      opts, s.verdicts, &cfg, s.stream);
    if (rc) return rc;
    e = hipEventRecord(s.e1, s.stream);
    if (e != hipSuccess) return hip_fail(e, "multi return: end");
  }
  // every device's records to the root, into the caller's verdict array, one group
  std::vector<Move> moves;
  for (int k = 0; k < m->ndev; ++k) {
    Shard &s = m->sh[k];
    moves.push_back({reinterpret_cast<const uint8_t *>(s.verdicts), reinterpret_cast<uint8_t *>(verdicts + s.lo),
                     sizeof(int32_t) * (s.hi - s.lo), k, m->root});
  }
  rc = grouped_moves(m, moves, "multi return: ncclSend / ncclRecv");
  if (rc) return rc;
  for (int k = 0; k < m->ndev && ms; ++k) {
    hipError_t e = hipSetDevice(m->sh[k].device);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], m->sh[k].e0, m->sh[k].e1);
    if (e != hipSuccess) return hip_fail(e, "multi return: events");
  }
  // the root applies them to its UMEM, with the descriptors the caller scattered
  Shard &rs = m->sh[m->root];
  hipError_t e = hipSetDevice(rs.device);
  if (e == hipSuccess && m->n) {
    const int32_t fwd = opts->action == XSKNF_CSUM_ACTION_REDIRECT
                            ? static_cast<int32_t>((ingress_ifindex + 1u) % opts->num_interfaces) : -1;
    hipLaunchKernelGGL(apply_records, dim3(grid_for(m->n, 4096)), dim3(256), 0, rs.stream, umem, m->root_orig,
                       verdicts, m->n, fwd);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(rs.stream);
  }
  if (e != hipSuccess) return hip_fail(e, "multi return: apply_records");
  if (seconds) *seconds = now_s() - t0;
  return 0;
}

int xsknf_gpu_multi_shard_info(const struct xsknf_gpu_multi *m, int k, struct xsknf_gpu_shard_info *info) {
  if (!m || !info || k < 0 || k >= m->ndev) return -EINVAL;
  const Shard &s = m->sh[k];
  info->device = s.device;
  info->flags = m->packed ? XSKNF_GPU_SHARD_PACKED : 0;
  info->frame_lo = s.lo;
  info->frame_hi = s.hi;
  info->span_lo = s.b0;   // (packed: 0 .. the shard's packed bytes)
  info->span_hi = s.b1;
  info->frame_bytes = s.bytes;
  info->umem = s.umem;
  info->descs = s.descs;
  info->verdicts = s.verdicts;
  return 0;
}

int xsknf_gpu_multi_fetch(const struct xsknf_gpu_multi *m, int k, uint8_t *umem_out, struct xsknf_gpu_desc *descs_out,
                          int32_t *verdicts_out) {
  if (!m || k < 0 || k >= m->ndev || m->root < 0) return -EINVAL;
  const Shard &s = m->sh[k];
  hipError_t e = hipSetDevice(s.device);
  if (e == hipSuccess && umem_out && s.b1 > s.b0)
    e = hipMemcpy(umem_out, s.umem, s.b1 - s.b0, hipMemcpyDeviceToHost);
  if (e == hipSuccess && descs_out && s.hi > s.lo)
    e = hipMemcpy(descs_out, s.descs, sizeof(xsknf_gpu_desc) * (s.hi - s.lo), hipMemcpyDeviceToHost);
  if (e == hipSuccess && verdicts_out && s.hi > s.lo)
    e = hipMemcpy(verdicts_out, s.verdicts, sizeof(int32_t) * (s.hi - s.lo), hipMemcpyDeviceToHost);
  return e == hipSuccess ? 0 : hip_fail(e, "multi fetch");
}

int xsknf_gpu_multi_destroy(struct xsknf_gpu_multi *m) {
  if (!m) return -EINVAL;
  for (Shard &s : m->sh) {
    if (hipSetDevice(s.device) != hipSuccess) continue;
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.umem_alloc) (void)hipFree(s.umem_alloc);
    if (s.descs) (void)hipFree(s.descs);
    if (s.verdicts) (void)hipFree(s.verdicts);
    if (s.counters) (void)hipFree(s.counters);
    if (s.e0) (void)hipEventDestroy(s.e0);
    if (s.e1) (void)hipEventDestroy(s.e1);
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  if (m->root_descs_dev >= 0 && hipSetDevice(m->root_descs_dev) == hipSuccess) {
    if (m->root_descs) (void)hipFree(m->root_descs);
    if (m->root_orig) (void)hipFree(m->root_orig);
    if (m->root_pack) (void)hipFree(m->root_pack);
    if (m->root_plan) (void)hipFree(m->root_plan);
  }
  for (ncclComm_t c : m->comms)
    if (c) (void)ncclCommDestroy(c);
  delete m;
  return 0;
}

}  // extern "C"
