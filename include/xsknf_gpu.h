/*
 * xsknf_gpu.h -- C ABI of the MI355X checksummer batch path.
 *
 * The reference calls one user function per received frame,
 *     int xsknf_packet_processor(void *pkt, unsigned len, unsigned ingress_ifindex);
 * (reference src/xsknf.h:19-23), once per rx descriptor from the per-frame loop of
 * process_batch_1if() (reference src/xsknf.c:654-672).  The checksummer's body is
 * reference examples/checksummer/checksummer_user.c:30-112.
 *
 * This library replaces that per-frame loop with ONE call per rx batch: the
 * whole batch of descriptors is handed over, every frame is checksummed on the
 * GPU, the 2-byte UDP check field is rewritten in place in the UMEM and one
 * verdict per frame is returned, with exactly the reference's meaning:
 *     -1           drop  (frame goes back to the fill ring, src/xsknf.c:663-666)
 *     0..n_if-1    transmit on that interface (tx ring, src/xsknf.c:667-671)
 *
 * Conventions (the reference's own): functions return 0 on success or a
 * negative errno; no torch or HIP types appear in any signature (streams are
 * passed as an opaque `void *` holding a hipStream_t; NULL = default stream).
 */
#ifndef XSKNF_GPU_H
#define XSKNF_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Everything else in the library is hidden (built with -fvisibility=hidden). */
#define XSKNF_GPU_API __attribute__((visibility("default")))

/* Same layout as struct xdp_desc (linux/if_xdp.h), i.e. exactly what the rx
 * ring holds and what xsk_ring_cons__rx_desc() returns (src/xsknf.c:655-656). */
struct xsknf_gpu_desc {
	uint64_t addr;      /* UMEM address; unaligned mode: base | (offset << 48) */
	uint32_t len;       /* frame length in bytes */
	uint32_t options;
};

/* xsk_umem__add_offset_to_addr() (libxdp, used at src/xsknf.c:659) */
#define XSKNF_GPU_UNALIGNED_BUF_OFFSET_SHIFT 48
#define XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK ((1ULL << XSKNF_GPU_UNALIGNED_BUF_OFFSET_SHIFT) - 1)

/* enum action, examples/checksummer/checksummer_user.c:15-18 */
#define XSKNF_CSUM_ACTION_REDIRECT 0
#define XSKNF_CSUM_ACTION_DROP 1

/* The three globals the reference callback reads (checksummer_user.c:24-25,28). */
struct xsknf_csum_opts {
	int32_t csum_iterations;   /* opt_csum_iterations (-i N), default 1; <= 0: no payload sum */
	int32_t action;            /* opt_action (-c REDIRECT|DROP), default REDIRECT */
	uint32_t num_interfaces;   /* config.num_interfaces (must be >= 1 for REDIRECT) */
	uint32_t reserved;         /* must be 0 */
};

/* Library version: (major << 16) | minor. */
XSKNF_GPU_API uint32_t xsknf_gpu_version(void);

/* Number of visible HIP devices in *count. */
XSKNF_GPU_API int xsknf_gpu_device_count(int *count);

/*
 * Checksum one rx batch, asynchronously on `stream`, on the current HIP device.
 * Replaces the loop `for i in batch: verdict[i] = xsknf_packet_processor(pkt_i,
 * len_i, ingress)` of src/xsknf.c:654-672 (pkt_i = umem + translated addr_i).
 *
 *   umem, umem_size   device-resident UMEM (hipMalloc'd, or a device mirror)
 *   descs, n          device-resident rx descriptors (n may be 0)
 *   ingress_ifindex   interface index of the rx socket (0 on the 1-iface path)
 *   opts              host pointer, read before return
 *   verdicts          device array of n int32, written by the kernel
 *   frame_len_hint    largest frame length expected in the batch (0 = 2048);
 *                     a performance hint only: every length is handled correctly
 *   stream            hipStream_t or NULL
 *
 * Descriptors whose [addr, addr+len) lies outside [0, umem_size) are not
 * touched and get verdict -1 (the kernel's own rx validation guarantees the
 * reference never sees one).  The frames of a batch are distinct UMEM chunks,
 * as an rx ring's are (the reference's serial loop would make two descriptors
 * of the same bytes order-dependent; here their frames are checksummed
 * concurrently).
 * A batch runs as one launch per 1M frames (per 16M for frames of at most
 * 128 bytes, where one launch over more frames measured faster; a lane-kernel
 * launch of more than 2M frames loads each lane's window itself and runs 8
 * blocks per CU, the faster shape for a long launch -- for the default shape
 * only: xsknf_gpu_checksum_batch_cfg() with blocks_per_cu != 0 runs exactly
 * the shape it is given).
 * Returns 0, -EINVAL on bad arguments, -EIO on a HIP launch error.
 *
 * Test hook: the environment variable XSKNF_GPU_CU_LIMIT=N sizes every grid as
 * on a device of N CUs (results are unchanged, launches slower; the library
 * says so on stderr once per device).  Not for production use.
 */
XSKNF_GPU_API int xsknf_gpu_checksum_batch(uint8_t *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n,
		uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
		int32_t *verdicts, uint32_t frame_len_hint, void *stream);

/*
 * Launch shape of the batch kernel (tuning / benchmarking).  A group of
 * `lanes_per_frame` lanes (4, 8, 16, 32 or 64) owns one frame at a time and loads
 * `chunks_per_lane` 16-byte chunks per pass; in the register kernel a wave
 * takes tiles of `frames_per_group` consecutive frames per group (the next
 * frame's loads in flight while the current one is reduced); the persistent
 * grid has `blocks_per_cu`
 * 256-thread blocks per CU (0 = 8).  `lds_ring` must be 0 (an LDS-DMA ring
 * kernel, measured slower, was A/B material until round 5; any other value is
 * -EINVAL); `kernel` = XSKNF_GPU_KERNEL_AUTO with lanes_per_frame > 1 selects
 * the register kernel.
 * `lanes_per_frame` = 1 selects the lane kernel for small frames: each lane
 * owns a frame, loads its first `chunks_per_lane` (5..7) chunks itself, and a
 * wave step covers 64 frames (`frames_per_group` = steps per tile); longer
 * frames are finished by a per-lane loop.
 * `fused_stores` = 1 writes every check from the summing kernel itself; 2 parks
 * every check for a second, write-only pass (non-temporal full 64-byte sector
 * rewrites); 0 (default) decides per frame: frames of 1024 bytes or more are
 * deferred (scattered writes mixed into the read stream cost ~25 % of its
 * bandwidth on MI355X), shorter ones write in-line (their check shares the line
 * just read).  3 = records only: the summing kernel runs alone, the UMEM is
 * only read, and every summed frame's verdicts[i] is left as the record
 *   XSKNF_GPU_RECORD_TAG | (u << 16) | check,   u = bits 22..16,
 * meaning "write the 16-bit `check` (as stored in memory, low byte first) at
 * frame offset u + 6, verdict = the forward verdict"; frames that are not
 * summed carry their final verdict.  The STAGED host path uses this mode (the
 * host applies the checks); benchmarks use it to time the summing kernel.
 * In-line checks whose 64-byte sector lies inside the frame are written as
 * that whole sector (group and lane kernels); adding 4 to `fused_stores` writes
 * the 2 check bytes alone instead, adding 8 makes the lane kernel's sector
 * stores plain (write-back) rather than non-temporal (A/B); where the 64 frames
 * of a lane-kernel step lie apart (a 2 KiB-chunk UMEM) its sector stores are
 * written through the L2 (sc1 nt).  Adding 16 (split kernel) patches the
 * deferred checks in the summing kernel itself, once the waves' streams are
 * done, instead of a second launch (the default with 2 for every frame length
 * past the lane kernel's: every check deferred, then patched in bursts at the
 * waves' ends; jumbo frames too since round 5).
 * A frame whose computed check equals the check it already holds (traffic whose
 * UDP checksums a NIC filled in, tests/gen-traffic.lua:120) ends with the bytes
 * it began with (:68 clears the check, :108 stores the same value), so the
 * product kernels write nothing for it and leave its verdict (no record in mode
 * 3).  Adding 32 to `fused_stores` writes such checks anyway (A/B only; the
 * UMEM and verdicts come out the same).
 * `kernel` = XSKNF_GPU_KERNEL_SPLIT selects the split kernel (the default for
 * every hint): lane l of a wave parses, sums and finishes frame l of a
 * 64-frame tile from its first `window_chunks` & 15 (4..7, or 8) chunks, and the
 * payload of longer frames is summed in items of one pass of `lanes_per_frame`
 * x `chunks_per_lane` chunks dealt to the wave's lane groups, `frames_per_group`
 * items per group in flight (any mix of lengths keeps every lane busy);
 * `window_chunks` + 16 loads the windows transposed (W lanes per frame, one
 * coalesced request); + 32 (with + 16, W = 8, 16 x 2 items, two in flight)
 * launches one 12-wave block per CU whose waves draw the CU's tiles from a
 * shared pool (the default up to 4 KiB frames; W = 4, 16 x 3: one 8-wave block
 * per CU, the jumbo default).  Only instantiated shapes are accepted (-EINVAL
 * otherwise); every shape gives identical results.
 */
#define XSKNF_GPU_RECORD_TAG 0x40000000u       /* bits 31..30 = 01 */
#define XSKNF_GPU_RECORD_TAG_MASK 0xC0000000u

#define XSKNF_GPU_KERNEL_AUTO 0    /* group register / lane kernel by the fields above */
#define XSKNF_GPU_KERNEL_SPLIT 1   /* headers by lane, payload by lane groups */

struct xsknf_gpu_launch_cfg {
	int32_t lanes_per_frame;
	int32_t chunks_per_lane;
	int32_t frames_per_group;
	int32_t blocks_per_cu;
	int32_t lds_ring;
	int32_t fused_stores;
	int32_t kernel;          /* XSKNF_GPU_KERNEL_* */
	int32_t window_chunks;   /* split kernel: header window per lane (16-byte chunks), +16 transposed load */
};

/* The shape xsknf_gpu_checksum_batch() uses for a given frame_len_hint. */
XSKNF_GPU_API int xsknf_gpu_default_launch_cfg(uint32_t frame_len_hint, struct xsknf_gpu_launch_cfg *cfg);

/*
 * xsknf_gpu_checksum_batch() for a caller that knows its batch's lengths: the
 * longest frame and the mean length (0 = unknown, as xsknf_gpu_checksum_batch()).
 * The mean picks the shape, which a largest-frame hint alone cannot: up to
 * 4 KiB, one 12-wave block per CU drawing the CU's tiles from a shared pool
 * (1500 B -4 %, 570 B -2 %), except for a mix of mostly short frames (mean
 * < 512 B, e.g. IMIX), which keeps 4-wave blocks and the static schedule
 * (+1.4 % with the pool).  Results are identical whatever the shape.
 */
XSKNF_GPU_API int xsknf_gpu_checksum_batch_lens(uint8_t *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n,
		uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
		int32_t *verdicts, uint32_t frame_len_max, uint32_t frame_len_mean, void *stream);
/* The shape xsknf_gpu_checksum_batch_lens() uses. */
XSKNF_GPU_API int xsknf_gpu_launch_cfg_for_lens(uint32_t frame_len_max, uint32_t frame_len_mean,
		struct xsknf_gpu_launch_cfg *cfg);

/* xsknf_gpu_checksum_batch() with an explicit launch shape instead of a hint. */
XSKNF_GPU_API int xsknf_gpu_checksum_batch_cfg(uint8_t *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n,
		uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts,
		int32_t *verdicts, const struct xsknf_gpu_launch_cfg *cfg, void *stream);

/*
 * Host-path context: the batch hook as the AF_XDP worker of src/xsknf.c would
 * call it, with the UMEM in host memory (the worker's mmap, src/xsknf.c:958,975)
 * and descriptors / verdicts in host arrays (the rx ring and to_drop / to_tx
 * routing of process_batch_1if, src/xsknf.c:654-672).
 *
 *   XSKNF_GPU_PATH_ZEROCOPY  the UMEM is pinned and mapped; the kernel reads
 *                            the frames and writes the check bytes in place
 *                            over PCIe (no copies).
 *   XSKNF_GPU_PATH_STAGED    only the batch's frame bytes are copied to a device
 *                            mirror (merged runs, or one 2-D copy for frames at
 *                            a constant stride) and checksummed in HBM; only
 *                            the 4-byte records come back and the host writes
 *                            the 2 check bytes.  A batch of frames scattered
 *                            over the UMEM runs as ZEROCOPY instead.
 *   XSKNF_GPU_PATH_RESIDENT  ZEROCOPY without a launch per batch: ONE kernel
 *                            resident on each device serves every RESIDENT
 *                            context of the process on that device (up to 64:
 *                            XSKNF_MAX_WORKERS workers x two UMEMs).  Each
 *                            context has its own ring (the submit writes the
 *                            descriptors and rings a doorbell, the wait spins
 *                            on a completion flag), 8 entries of up to 256
 *                            frames, one block each when max_batch <= 64,
 *                            else four (64 frames each), so up to 8 batches
 *                            per context (or pieces of a larger one) are
 *                            processed at once.  For the rx loop's small
 *                            batches.  The kernel leaves after 1 ms without a
 *                            batch on any ring (and after 4 ms in all) and the
 *                            next submit or wait of any context relaunches it;
 *                            creating or destroying a RESIDENT context stops
 *                            and relaunches it.  It holds one hardware queue
 *                            (GPU_MAX_HW_QUEUES is 4 by default): a process
 *                            that also launches work of its own (ZEROCOPY /
 *                            STAGED contexts, torch) may find a launch queued
 *                            behind it for up to those 4 ms when its streams
 *                            outnumber the hardware queues.  (Measured with 4
 *                            RESIDENT and 4 ZEROCOPY workers in one process:
 *                            no such wait, each side 10-40 % slower per batch
 *                            than alone -- DESIGN 5.3.)  Creating a context returns
 *                            -ENOSPC past 64 rings per device.
 * One context = one worker thread.  A launched context keeps up to five batches in
 * flight (five slots, each with its own HIP stream: four out plus the one being
 * submitted; a deeper hook's submit waits for the oldest): the copies and kernel of
 * one overlap another's, and the host's share of one overlaps the device's share of
 * the others.  A RESIDENT context keeps up to eight (its ring's entries, as many as
 * XSKNF_MAX_HOOK_DEPTH).
 * xsknf_gpu_ctx_process_batch() is synchronous: when it returns, verdicts and
 * check bytes are in host memory (a batch larger than 65536 frames runs as
 * pieces through the slots; if a piece fails to start, the pieces already
 * started are completed before the error returns).  xsknf_gpu_ctx_submit() returns once the batch
 * is enqueued, with a ticket; xsknf_gpu_ctx_wait(ticket) returns once that
 * batch and every earlier one is complete (verdicts written, check bytes in
 * the UMEM).  A submit may itself complete older batches to free a slot.  The
 * frames of batches in flight must not be touched by the caller, and
 * `verdicts` must stay valid, until their wait.
 */
#define XSKNF_GPU_PATH_ZEROCOPY 0
#define XSKNF_GPU_PATH_STAGED 1
#define XSKNF_GPU_PATH_RESIDENT 2

struct xsknf_gpu_ctx;

struct xsknf_gpu_ctx_stats {
	uint64_t batches;
	uint64_t frames;
	uint64_t bytes_h2d;
	uint64_t bytes_d2h;
	uint64_t resident_batches;   /* ring entries the device's resident kernel completed (RESIDENT) */
	uint64_t resident_launches;  /* launches of that kernel so far, for every context of the device */
};

XSKNF_GPU_API int xsknf_gpu_ctx_create(struct xsknf_gpu_ctx **ctx, int device, int path,
		uint32_t max_batch, uint32_t frame_len_hint);
/* Pin (and for ZEROCOPY map) the host UMEM [umem, umem + size). */
XSKNF_GPU_API int xsknf_gpu_ctx_register_umem(struct xsknf_gpu_ctx *ctx, void *umem, uint64_t size);
XSKNF_GPU_API int xsknf_gpu_ctx_process_batch(struct xsknf_gpu_ctx *ctx,
		const struct xsknf_gpu_desc *descs, uint32_t n, uint32_t ingress_ifindex,
		const struct xsknf_csum_opts *opts, int32_t *verdicts);
XSKNF_GPU_API int xsknf_gpu_ctx_submit(struct xsknf_gpu_ctx *ctx, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, const struct xsknf_csum_opts *opts, int32_t *verdicts,
		uint64_t *ticket);
XSKNF_GPU_API int xsknf_gpu_ctx_wait(struct xsknf_gpu_ctx *ctx, uint64_t ticket);
XSKNF_GPU_API int xsknf_gpu_ctx_get_stats(const struct xsknf_gpu_ctx *ctx, struct xsknf_gpu_ctx_stats *stats);
XSKNF_GPU_API int xsknf_gpu_ctx_destroy(struct xsknf_gpu_ctx *ctx);

/* ---- batch hook for the AF_XDP runtime (include/xsknf.h) ------------------
 * The checksummer NF as an xsknf_batch_processor_fn: it replaces the per-frame
 * xsknf_packet_processor() loop of process_batch_1if / process_batch
 * (src/xsknf.c:654-672, :500-522).  Each worker gets its own context (device
 * worker_idx % device count, `path` as above), created on the worker's first
 * batch for each UMEM it sees, so no call crosses threads.  Register with
 *   xsknf_set_batch_processor((xsknf_batch_processor_fn)xsknf_gpu_hook_process, hook);
 * Stop the workers before xsknf_gpu_hook_destroy(), and destroy the hook
 * before xsknf_cleanup() unmaps the UMEMs. */
struct xsknf_gpu_hook;

XSKNF_GPU_API int xsknf_gpu_hook_create(struct xsknf_gpu_hook **hook, const struct xsknf_csum_opts *opts,
		uint32_t workers, int path, uint32_t max_batch, uint32_t frame_len_hint);
XSKNF_GPU_API int xsknf_gpu_hook_process(void *hook, uint32_t worker_idx, void *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n, uint32_t ingress_ifindex, int32_t *verdicts);
/* The same NF as a two-phase hook (xsknf_batch_submit_fn / xsknf_batch_complete_fn):
 *   xsknf_set_batch_processor_async((xsknf_batch_submit_fn)xsknf_gpu_hook_submit,
 *                                   (xsknf_batch_complete_fn)xsknf_gpu_hook_complete, hook);
 * submit enqueues the batch on the worker's context (xsknf_gpu_ctx_submit),
 * complete waits for its ticket (xsknf_gpu_ctx_wait): the worker receives the
 * next batch while the GPU checksums this one. */
XSKNF_GPU_API int xsknf_gpu_hook_submit(void *hook, uint32_t worker_idx, void *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n, uint32_t ingress_ifindex, int32_t *verdicts,
		uint64_t *ticket);
XSKNF_GPU_API int xsknf_gpu_hook_complete(void *hook, uint32_t worker_idx, void *umem, uint64_t ticket);
/* Sum of the worker's context stats. */
XSKNF_GPU_API int xsknf_gpu_hook_get_stats(const struct xsknf_gpu_hook *hook, uint32_t worker_idx,
		struct xsknf_gpu_ctx_stats *stats);
XSKNF_GPU_API int xsknf_gpu_hook_destroy(struct xsknf_gpu_hook *hook);

/* ---- one process over several devices (BASELINE config 4) ----------------
 * The reference scales one worker per NIC queue (src/xsknf.c:992, workers
 * started per queue at :1046-1100); frames never cross workers.  The hook above
 * is that model on a node of GPUs (worker w on device w % devices).  These
 * calls are for a global batch that starts on ONE device: it is split into
 * contiguous descriptor ranges balanced by frame bytes, each range's UMEM span
 * and rebased descriptors are moved from the root device to its own by grouped
 * RCCL point-to-point sends over xGMI (one communicator per device,
 * ncclCommInitAll), every device checksums its shard on its own stream, and the
 * counters of all shards are summed by an RCCL all-reduce.  The results equal
 * one device's pass over the whole batch (tests/test_gpu_multi.py). */

/* The byte-balanced split of n descriptors into nshards contiguous ranges:
 * shard k is frames [bounds[k], bounds[k+1]) (bounds: nshards + 1 entries),
 * cut after the first frame whose running sum of lengths reaches
 * total * k / nshards (xsknf_amd/shard.py shard_by_bytes); spans (NULL, or
 * 2 * nshards entries) = each shard's UMEM byte span [lo, hi) over its frames
 * inside [0, umem_size) ({0, 0} for none).  Host arrays; no GPU call. */
XSKNF_GPU_API int xsknf_gpu_shard_plan(const struct xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_size,
		uint32_t nshards, uint64_t *bounds, uint64_t *spans);
/* A shard's descriptors relative to its span's first byte b0 (plain aligned-mode
 * addresses); a descriptor outside [0, umem_size) gets an address past any
 * UMEM (1 << 47): its verdict is -1 and no byte is touched, as before.  Host
 * arrays; no GPU call. */
XSKNF_GPU_API int xsknf_gpu_shard_rebase(const struct xsknf_gpu_desc *descs, uint64_t n, uint64_t b0,
		uint64_t umem_size, struct xsknf_gpu_desc *out);

struct xsknf_gpu_multi;

/* [frames, frame bytes, drops (-1), forwards (>= 0), sum of the 16-bit words at
 * +40 of every frame of >= 42 bytes (an ihl-5 frame's UDP check), the same
 * weighted by ((global UMEM offset) mod 65521) + 1] */
#define XSKNF_GPU_MULTI_COUNTERS 6

#define XSKNF_GPU_SHARD_PACKED 1u   /* shard_info.flags: moved by xsknf_gpu_multi_scatter_packed */

struct xsknf_gpu_shard_info {
	int32_t device;          /* HIP device of the shard */
	uint32_t flags;          /* XSKNF_GPU_SHARD_PACKED */
	uint64_t frame_lo, frame_hi;   /* frames [lo, hi) of the global batch */
	uint64_t span_lo, span_hi;     /* its bytes [lo, hi) of the root's UMEM (packed: 0 and the
	                                  shard's packed bytes) */
	uint64_t frame_bytes;          /* sum of its frame lengths */
	uint8_t *umem;                 /* device buffers of the shard on its device */
	struct xsknf_gpu_desc *descs;
	int32_t *verdicts;
};

/* The packed layout of xsknf_gpu_multi_scatter_packed (no GPU): for shards
 * [bounds[k], bounds[k+1]) of n descriptors over a UMEM at device address
 * umem_addr, each frame gets a 16-byte aligned slot in its shard's packed
 * buffer, at the same address mod 16 as in the UMEM; packed[f] is frame f's
 * descriptor there (its length and options kept; a descriptor outside the
 * UMEM gets an address past any span and no slot), sizes[k] shard k's packed
 * bytes.  A frame of len bytes at address a mod 16 = r takes round16(r + len). */
XSKNF_GPU_API int xsknf_gpu_shard_pack_plan(const struct xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_addr,
		uint64_t umem_size, uint32_t nshards, const uint64_t *bounds, struct xsknf_gpu_desc *packed,
		uint64_t *sizes);
/* One RCCL communicator per device of devices[0..ndev) (NULL: devices 0..ndev-1,
 * each at most once), a stream each. */
XSKNF_GPU_API int xsknf_gpu_multi_create(struct xsknf_gpu_multi **m, const int *devices, int ndev);
/* Split the global batch -- `umem` (umem_size bytes) resident on device
 * devices[root], `descs` its n descriptors in host memory -- by
 * xsknf_gpu_shard_plan and move every shard to its device: one grouped set of
 * ncclSend / ncclRecv, the root's own shard as a send to itself.  Shard buffers
 * are allocated on first use and kept for later scatters of the same size or
 * smaller.  *seconds (may be NULL): wall time of the transfers. */
XSKNF_GPU_API int xsknf_gpu_multi_scatter(struct xsknf_gpu_multi *m, int root, const uint8_t *umem,
		uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint64_t n, double *seconds);
/* Checksum every device's shard (xsknf_gpu_checksum_batch_lens on its own
 * stream, all devices in flight at once); returns when all are done.  ms (may be
 * NULL, ndev entries): each device's HIP-event time. */
XSKNF_GPU_API int xsknf_gpu_multi_process(struct xsknf_gpu_multi *m, uint32_t ingress_ifindex,
		const struct xsknf_csum_opts *opts, uint32_t frame_len_max, uint32_t frame_len_mean, float *ms);
/* The XSKNF_GPU_MULTI_COUNTERS counters of every shard, summed over the devices
 * by ncclAllReduce (the root's copy, to host memory).  -EOPNOTSUPP after a
 * packed scatter (a packed shard no longer holds its frames' UMEM offsets,
 * which the weighted sum needs; its results come back by _return). */
XSKNF_GPU_API int xsknf_gpu_multi_counters(struct xsknf_gpu_multi *m, uint64_t *out);
/* As xsknf_gpu_multi_scatter, moving only the frames' bytes: on the root a
 * kernel copies each shard's frames into 16-byte aligned slots of a packed
 * buffer (a frame keeps its address mod 16; the bytes that share its first and
 * last 16-byte chunk travel with it), and each shard receives its packed bytes
 * plus descriptors that address them (aligned-mode addresses; descriptors
 * outside the UMEM keep their length and get an address past any span).  The
 * root's own shard is packed straight into its shard buffer (its descriptors
 * still go as a send to itself).  A UMEM of 2 KiB chunks holding IMIX frames
 * moves ~1/5 of its span bytes.
 * seconds (may be NULL): the packing and the moves. */
XSKNF_GPU_API int xsknf_gpu_multi_scatter_packed(struct xsknf_gpu_multi *m, int root, const uint8_t *umem,
		uint64_t umem_size, const struct xsknf_gpu_desc *descs, uint64_t n, double *seconds);
/* The whole batch's results back to the root, after either scatter: every
 * device runs the summing pass over its shard in records-only mode (fused_stores
 * 3: the shard is only read), sends its 4-byte record / verdict per frame to
 * the root into verdicts[0..n) (device memory on the root, the scatter's frame
 * order), and a kernel on the root writes each record's check into `umem` (the
 * root UMEM the scatter read, at the frame the caller's descriptor names) and
 * turns it into the forward verdict.  `umem` and `verdicts` then hold what one
 * device's xsknf_gpu_checksum_batch over the whole batch leaves.  -EBUSY when
 * xsknf_gpu_multi_process has checksummed the shards in place since the
 * scatter (a second pass is not the first: a frame whose UDP header overlaps
 * its IP addresses sums the check the first wrote); scatter again.  ms (may be
 * NULL, ndev entries): each device's summing pass, HIP events; seconds (may be
 * NULL): the whole return. */
XSKNF_GPU_API int xsknf_gpu_multi_return(struct xsknf_gpu_multi *m, uint32_t ingress_ifindex,
		const struct xsknf_csum_opts *opts, uint32_t frame_len_max, uint32_t frame_len_mean, uint8_t *umem,
		int32_t *verdicts, float *ms, double *seconds);
/* ---- the plan computed on the root device ----
 * For a batch whose descriptors already lie in the root's device memory (next
 * to its UMEM): the cuts, spans / packed layout and byte sums above, computed
 * by kernels on that device instead of one CPU thread, bit-identical to
 * xsknf_gpu_shard_plan, _shard_rebase and _shard_pack_plan for every input.
 * The per-frame outputs stay on the device; the host reads back one small
 * array (the cuts, the spans or sizes, the byte sums). */
#define XSKNF_GPU_PLAN_SPAN 0     /* spans + rebased descriptors (xsknf_gpu_multi_scatter's plan) */
#define XSKNF_GPU_PLAN_PACKED 1   /* sizes + packed descriptors (xsknf_gpu_multi_scatter_packed's plan) */
/* *bytes = the device workspace xsknf_gpu_shard_plan_dev needs for n descriptors
 * (positive, non-decreasing in n, the same for every nshards in 1..64).  Host
 * arithmetic; no GPU call.  -EINVAL for nshards 0 or > 64 or a NULL bytes. */
XSKNF_GPU_API int xsknf_gpu_shard_plan_dev_workspace(uint64_t n, uint32_t nshards, uint64_t *bytes);
/* Plan n descriptors at `descs` (memory of the current device, 16-byte aligned)
 * of a UMEM at device address umem_addr into 1 <= nshards <= 64 shards, on
 * `stream` (a hipStream_t; NULL: the default stream):
 *   bounds[nshards + 1]   the cuts of xsknf_gpu_shard_plan;
 *   frame_bytes[nshards]  each shard's sum of frame lengths (may be NULL);
 *   XSKNF_GPU_PLAN_SPAN:   spans_or_sizes[2 * nshards] = the spans of
 *     xsknf_gpu_shard_plan, out_descs[f] = frame f's descriptor relative to its
 *     shard's span (xsknf_gpu_shard_rebase per shard);
 *   XSKNF_GPU_PLAN_PACKED: spans_or_sizes[nshards] = the sizes and out_descs the
 *     packed descriptors of xsknf_gpu_shard_pack_plan (umem_addr gives the
 *     frames' addresses mod 16).
 * bounds, spans_or_sizes (may be NULL) and frame_bytes are host arrays, filled
 * when the call returns (it waits for `stream`); out_descs (n records, 16-byte
 * aligned, not overlapping descs) and workspace (workspace_bytes >= what
 * _workspace reports, 8-byte aligned) are device memory.  n == 0 succeeds
 * without a launch (all outputs 0).  -EINVAL, before any GPU call, for nshards
 * 0 or > 64, a NULL bounds, an unknown mode, and with n > 0 a NULL or
 * misaligned descs / out_descs / workspace or a workspace too small.  The cut
 * rule compares in double exactly as the host does (running sums below 2^53
 * bytes are exact there). */
XSKNF_GPU_API int xsknf_gpu_shard_plan_dev(const struct xsknf_gpu_desc *descs, uint64_t n, uint64_t umem_addr,
		uint64_t umem_size, uint32_t nshards, int mode, struct xsknf_gpu_desc *out_descs, uint64_t *bounds,
		uint64_t *spans_or_sizes, uint64_t *frame_bytes, void *workspace, uint64_t workspace_bytes,
		void *stream);
/* xsknf_gpu_multi_scatter (mode XSKNF_GPU_PLAN_SPAN) or _scatter_packed
 * (XSKNF_GPU_PLAN_PACKED) for descriptors in DEVICE memory: descs_dev (n
 * records, 16-byte aligned) lies on devices[root] like `umem`.  The plan is
 * computed there by xsknf_gpu_shard_plan_dev's kernels (the workspace is kept
 * in the object), the descriptors are kept for _return by a device-to-device
 * copy (the caller may reuse its buffer once the call returns), and the shards
 * move exactly as from the host variants: afterwards the object is in the state
 * the host variant leaves for the same batch, for _process, _counters, _return,
 * _shard_info and _fetch alike.
 * *seconds (may be NULL): from the first planning step to the end of the moves
 * (root and shard buffer allocation included; the host variants' `seconds`
 * start after their planning and staging).  *plan_seconds (may be NULL): the
 * planning kernels and the read-back of their result alone. */
XSKNF_GPU_API int xsknf_gpu_multi_scatter_dev(struct xsknf_gpu_multi *m, int root, const uint8_t *umem,
		uint64_t umem_size, const struct xsknf_gpu_desc *descs_dev, uint64_t n, int mode, double *seconds,
		double *plan_seconds);
XSKNF_GPU_API int xsknf_gpu_multi_shard_info(const struct xsknf_gpu_multi *m, int shard,
		struct xsknf_gpu_shard_info *info);
/* Copy shard `shard`'s UMEM span (span_hi - span_lo bytes), its rebased
 * descriptors and its verdicts to host memory (any of them may be NULL). */
XSKNF_GPU_API int xsknf_gpu_multi_fetch(const struct xsknf_gpu_multi *m, int shard, uint8_t *umem_out,
		struct xsknf_gpu_desc *descs_out, int32_t *verdicts_out);
XSKNF_GPU_API int xsknf_gpu_multi_destroy(struct xsknf_gpu_multi *m);

/* ---- routing a checksummed batch: per-interface tx lists and the fill list ----
 * The second half of the reference's batch loop (process_batch, src/xsknf.c:
 * 503-522, and process_batch_1if, :654-672) for a batch whose verdicts are
 * known: every frame is filed by its verdict, a dropped frame into to_drop[]
 * and any other into to_tx[verdict][], in receive order, and those lists are
 * what goes into the fill ring (u64 addr, :538-540, :685-687) and into the
 * destination's tx ring ({addr, len}, :573-578, :706-709).  The checksum calls
 * above and xsknf_gpu_multi_return leave one int32 verdict per frame next to the
 * descriptors, in device memory; these calls turn that state into ring-ready
 * lists, on the device or (the model the device is held to) on one CPU thread,
 * with the same result bit for bit.
 *
 * The bin of frame f (D = drop):
 *   num_interfaces == 1   process_batch_1if's rule (xsknf_rt.c dispose_1if):
 *                         verdicts[f] == -1 gives D, any other value interface 0;
 *   num_interfaces > 1    xsknf_rt.c dispose_multi's: v < 0 or (uint32_t)v >=
 *                         num_interfaces gives D, else interface v (the reference
 *                         would index to_tx[] with such a v unchecked).
 * counts[i], i < num_interfaces, is the number of frames in bin i and
 * counts[num_interfaces] the number of dropped frames; base_i = counts[0] + ... +
 * counts[i - 1], ntx = the sum over all interfaces.  The partition is stable:
 * with r the number of frames g < f in f's bin,
 *   a tx frame of bin i  tx_descs[base_i + r] = {descs[f].addr, descs[f].len, 0}
 *                        (the address as received, untranslated: `orig`, :507;
 *                        options 0), and order[base_i + r] = f;
 *   a dropped frame      fill_addrs[r] = descs[f].addr, and order[ntx + r] = f.
 * Interface i's tx list is tx_descs[base_i .. base_i + counts[i]).  Entries of
 * tx_descs at or past ntx and of fill_addrs at or past the drop count are not
 * written; descs and verdicts are only read.  The outputs must not overlap the
 * inputs or each other.  `order` (may be NULL) is what a gather of the frames'
 * bytes into a packed buffer would consume (the copy of :563-571 into another
 * UMEM needs only the lists: xsknf_gpu_forward_frames below).
 *
 * A record left by a records-only pass (fused_stores 3: a word tagged
 * XSKNF_GPU_RECORD_TAG, 0x4...) is NOT a verdict: apply the records first (as
 * xsknf_gpu_multi_return and the STAGED host path do); routed as it stands, such
 * a word is just a value that names no interface. */
#define XSKNF_GPU_ROUTE_MAX_INTERFACES 32   /* XSKNF_MAX_INTERFACES, src/xsknf.h:11 */

/* *bytes = the device workspace xsknf_gpu_route_batch needs for n frames
 * (positive, non-decreasing in n).  Host arithmetic; no GPU call.  -EINVAL for
 * num_interfaces 0 or > 32 or a NULL bytes. */
XSKNF_GPU_API int xsknf_gpu_route_workspace(uint32_t n, uint32_t num_interfaces, uint64_t *bytes);
/* Route n frames on the current device, on `stream` (a hipStream_t; NULL: the
 * default stream).  descs (16-byte aligned) and verdicts are device memory, as
 * are tx_descs (n records, 16-byte aligned), fill_addrs (n words), order (n
 * words, may be NULL) and workspace (8-byte aligned, workspace_bytes >= what
 * _workspace reports for n and num_interfaces).
 * counts (HOST memory, num_interfaces + 1 words, may be NULL):
 *   given   filled when the call returns: the call waits for `stream`;
 *   NULL    the call only enqueues; the same num_interfaces + 1 words are the
 *           first u64 words of `workspace` once the stream gets there (they are
 *           there in either case).
 * n == 0 succeeds without a launch: a given counts is all 0, nothing else is
 * written (the workspace neither, and it may be NULL).
 * -EINVAL, before any GPU call: num_interfaces 0 or > 32; descs or tx_descs not
 * 16-byte aligned, fill_addrs or workspace not 8-byte aligned, verdicts or order
 * not 4-byte aligned; and with n > 0 a NULL descs, verdicts, tx_descs,
 * fill_addrs or workspace, or a workspace too small.  -EIO on a HIP error, with
 * xsknf_gpu_last_error() set. */
XSKNF_GPU_API int xsknf_gpu_route_batch(const struct xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n,
		uint32_t num_interfaces, struct xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs, uint32_t *order,
		uint64_t *counts, void *workspace, uint64_t workspace_bytes, void *stream);
/* The same on host arrays, one thread, no GPU call.  -EINVAL for num_interfaces
 * 0 or > 32 and, with n > 0, a NULL descs, verdicts, tx_descs or fill_addrs
 * (order and counts may be NULL). */
XSKNF_GPU_API int xsknf_gpu_route_host(const struct xsknf_gpu_desc *descs, const int32_t *verdicts, uint32_t n,
		uint32_t num_interfaces, struct xsknf_gpu_desc *tx_descs, uint64_t *fill_addrs, uint32_t *order,
		uint64_t *counts);

/* ---- forwarding routed frames into their tx interface's UMEM ----------------
 * The third part of the reference's batch loop (process_batch, src/xsknf.c:
 * 548-584): when the destination interface has a UMEM of its own (rx_xsk->buffer
 * != xsks[i].buffer, :563-571) every forwarded frame's bytes are copied into
 * that UMEM at the same address before its descriptor goes into the tx ring;
 * an interface that shares the rx UMEM gets the descriptors alone (:572-579).
 * These calls do that copy for the tx lists xsknf_gpu_route_batch leaves, on
 * the device or (the model the device is held to) on one CPU thread, with the
 * same destination bytes and stats.
 *
 * tx_descs and counts are exactly what the router leaves: interface i's list is
 * tx_descs[base_i .. base_i + counts[i]), base_i = counts[0] + ... + counts[i - 1];
 * counts has num_interfaces + 1 words (the last, the drops, is not used).
 * tx_umems and tx_umem_sizes are HOST arrays of num_interfaces entries, read
 * before the call returns.  tx_umems[i] NULL or equal to rx_umem: interface i
 * shares the rx UMEM, and its entries are not copied, not range-checked and not
 * counted.  For every other interface each entry {addr, len} copies exactly len
 * bytes from rx_umem + off to tx_umems[i] + off, with
 *   off = (addr & XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK) + (addr >> 48),
 * the runtime's addr_offset() (xsknf_rt.c dispose_multi).  The reference indexes
 * both UMEMs with the untranslated `orig` (:565-566), which in unaligned mode
 * carries the offset in its upper 16 bits and is a wild address; in aligned mode
 * the two are the same.  We follow the runtime.
 * An entry is copied only if off <= size && len <= size - off holds for both
 * rx_umem_size and tx_umem_sizes[i]; otherwise it is skipped and counted in
 * stats[2].  len == 0 is a copied frame of 0 bytes.  No byte of any destination
 * UMEM outside [off, off + len) of a copied frame is written; the rx UMEM and
 * tx_descs are only read.  The frames of a batch are distinct chunks, as
 * everywhere in this header: two entries naming the same bytes write the same
 * values twice.
 *
 * -EINVAL for both calls, before anything is read through the pointers:
 * num_interfaces 0 or > 32; a NULL tx_umems or tx_umem_sizes; rx_umem or a
 * non-NULL tx_umems[i] not 16-byte aligned; a non-NULL tx_umems[i] other than
 * rx_umem whose [p, p + size) overlaps [rx_umem, rx_umem + rx_umem_size); two
 * different non-NULL destination UMEMs that overlap each other (the same UMEM
 * under two interfaces is fine); tx_descs not 16-byte aligned, counts or
 * stats_dev not 8-byte aligned; and, with entries to look at, a NULL rx_umem,
 * tx_descs, counts or stats_dev. */
/* stats: [0] frames copied, [1] bytes copied, [2] frames skipped (out of range) */
#define XSKNF_GPU_FORWARD_STATS 3

/* On the current device, on `stream` (a hipStream_t; NULL: the default stream).
 * rx_umem, the pointers in tx_umems, tx_descs, counts_dev and stats_dev are
 * device memory.  The counts are read ON THE DEVICE, so a route with counts ==
 * NULL and this call can be enqueued back to back with the route's workspace
 * pointer as counts_dev and no host read-back between.  n is only an upper bound
 * on the tx total -- the capacity of tx_descs, which sizes the grid; entries at
 * or past the real total (or n) are never read.
 * stats_dev (3 u64, required) is zeroed on the stream first and holds the stats
 * once the stream gets there.  stats (HOST, 3 u64, may be NULL): given, the call
 * waits for `stream` and fills it; NULL, the call only enqueues.
 * n == 0 succeeds with nothing touched on the device (the device pointers may be
 * NULL); n > 0 with no interface to copy for (all NULL or rx_umem) zeroes
 * stats_dev and launches nothing.  A given stats is all 0 in both cases.
 * -EIO on a HIP error, with xsknf_gpu_last_error() set. */
XSKNF_GPU_API int xsknf_gpu_forward_frames(const uint8_t *rx_umem, uint64_t rx_umem_size,
		uint8_t *const *tx_umems, const uint64_t *tx_umem_sizes, uint32_t num_interfaces,
		const struct xsknf_gpu_desc *tx_descs, const uint64_t *counts_dev, uint32_t n,
		uint64_t *stats_dev, uint64_t *stats, void *stream);
/* The same on host arrays: one thread, a memcpy per entry, no GPU call.  The
 * number of entries is the sum of counts[0 .. num_interfaces); stats may be
 * NULL, and with no entry so may rx_umem, tx_descs and counts. */
XSKNF_GPU_API int xsknf_gpu_forward_host(const uint8_t *rx_umem, uint64_t rx_umem_size,
		uint8_t *const *tx_umems, const uint64_t *tx_umem_sizes, uint32_t num_interfaces,
		const struct xsknf_gpu_desc *tx_descs, const uint64_t *counts, uint64_t *stats);

/* ---- the firewall NF: a 5-tuple ACL lookup to one verdict per frame ----------
 * The reference's second NF with the per-frame callback
 * (examples/firewall/firewall_user.c:128-186): parse Ethernet / IPv4 / TCP or
 * UDP, look the 13-byte 5-tuple up in an exact-match ACL, return the rule's
 * action (-1: drop; otherwise a tx interface index; 0 where no rule matches).
 * These calls do that for a whole batch, on the device or (the model the device
 * is held to) on one CPU thread.  The verdicts are what xsknf_gpu_route_batch
 * consumes; the UMEM is only read, and ingress_ifindex plays no part.
 *
 * Per frame, with f its bytes at umem + off,
 *   off = (addr & XSKNF_GPU_UNALIGNED_BUF_ADDR_MASK) + (addr >> 48),
 * and len its length:
 *   0. not (off <= umem_size && len <= umem_size - off)   -> -1, no byte read
 *   1. len < 14                                           -> -1
 *   2. f[12..13] != 08 00                                 ->  0
 *   3. len < 34                                           -> -1
 *   4. next = 14 + 4 * (f[14] & 15)       (the ihl nibble is not validated: 0..15;
 *                                          below 5 the ports overlap the IP header)
 *   5. f[23] == 6 (TCP):  next + 20 > len                 -> -1
 *      f[23] == 17 (UDP): next + 8 > len                  -> -1
 *      any other protocol                                 ->  0
 *   6. key = { saddr f[26..29], daddr f[30..33], sport f[next..next+1],
 *              dport f[next+2..next+3], proto f[23] }, all as they lie in the
 *      frame (network order), as the reference's struct session_id holds them
 *   7. the action of the rule whose key equals this key, or 0 if there is none.
 *
 * The ACL is an exact-match map, the last rule winning among equal keys
 * (khashmap_update_elem replaces the value).  Nothing else of the reference's
 * khashmap is kept: the table is open addressing with linear probing over a
 * power-of-two number of 16-byte key slots {saddr, daddr, sport | dport << 16,
 * proto}, proto 0 marking an empty slot, and the actions in a parallel int32
 * array that is read only on a hit (20 bytes per slot in all); the hash is a
 * multiply / xor-shift mix of the key's four words (xsknf_amd/csrc/acl_table.h).
 * At least one slot is always empty, so every probe sequence ends. */
#define XSKNF_GPU_ACL_MAX_RULES 1000000u   /* MAX_ACL_SIZE, examples/firewall/firewall.h */
#define XSKNF_GPU_ACL_MAX_SLOTS (1u << 24)

struct xsknf_gpu_acl_rule {
	uint32_t saddr, daddr;   /* network order (as in_addr.s_addr) */
	uint16_t sport, dport;   /* network order */
	uint8_t proto;           /* 6 or 17; a rule with any other can never match */
	uint8_t pad[3];          /* ignored */
	int32_t action;          /* any int32: -1 drops, the rest is the caller's (atoi's result) */
};

struct xsknf_gpu_acl;        /* opaque */

struct xsknf_gpu_acl_info {
	uint32_t rules;          /* distinct keys in the table */
	uint32_t slots;          /* key slots (a power of two > rules) */
	uint32_t max_probe;      /* slots looked at for the worst-placed rule (0 for an empty ACL), kept across updates */
	uint32_t tombstones;     /* slots that mark a deleted key (xsknf_gpu_acl_update); 0 after _create */
	uint64_t device_bytes;   /* 20 * slots, and the hit counters' share once enabled (0: built where no device was visible) */
};

/* Read the reference's ACL text (init_acl, firewall_user.c:53-116): the rule
 * count, then records `saddr daddr sport dport PROTO ACTION` separated by any
 * white space; dotted-quad addresses (inet_aton), decimal ports of which the
 * low 16 bits count (htons), PROTO TCP or UDP, ACTION DROP (-1) or atoi's
 * reading of it (0 for a word that is no number).  At most `cap` rules are
 * written to rules_out (may be NULL with cap 0) and *n_out is the file's count;
 * the whole file is validated either way.  No GPU call.
 * Where the reference exits, we return: -errno when the file cannot be opened
 * (-ENOENT ...), -EINVAL for an unknown protocol or a count that differs from the
 * records.  Where the reference goes on silently we return -EINVAL as well: an
 * address inet_aton rejects (the reference keeps the previous record's address);
 * an address longer than 15, a protocol longer than 3 or an action longer than
 * 4 characters (the reference overruns its buffers); a count or a port that is
 * not a decimal number below 2^32, or a last record cut short (the reference's
 * fscanf loop then reads garbage or never ends); more than
 * XSKNF_GPU_ACL_MAX_RULES rules (the reference overruns its element pool).
 * -ENOSPC when cap is less than the count (*n_out is set: ask again). */
XSKNF_GPU_API int xsknf_gpu_acl_parse(const char *path, struct xsknf_gpu_acl_rule *rules_out, uint32_t cap,
		uint32_t *n_out);
/* Build the table from n rules on the calling thread (deterministic: the same
 * rules give the same table) and upload it to the current device, where it
 * stays until _destroy; a host copy is kept for xsknf_gpu_firewall_host.
 * slots == 0: the smallest power of two >= 2 n, at least 64.  Otherwise slots
 * must be a power of two, at most XSKNF_GPU_ACL_MAX_SLOTS and greater than the
 * number of distinct keys.  Rules with a protocol other than 6 and 17 are left
 * out; n == 0 gives a valid ACL that matches nothing.  In a process that sees
 * no HIP device the ACL is built on the host alone (device_bytes 0): it serves
 * xsknf_gpu_firewall_host, and xsknf_gpu_firewall_batch returns -ENODEV for it
 * -- there is no CPU path behind the device call.  -EINVAL for a NULL
 * acl_out, a NULL rules with n > 0 or a bad slots; -ENOMEM; -EIO on a HIP error
 * (xsknf_gpu_last_error()). */
XSKNF_GPU_API int xsknf_gpu_acl_create(struct xsknf_gpu_acl **acl_out, const struct xsknf_gpu_acl_rule *rules,
		uint32_t n, uint32_t slots);
XSKNF_GPU_API int xsknf_gpu_acl_info(const struct xsknf_gpu_acl *acl, struct xsknf_gpu_acl_info *info);
/* Free the table on the device and the host, and the updates' buffers (no
 * batch that uses it and no update may be in flight).  -EINVAL for NULL. */
XSKNF_GPU_API int xsknf_gpu_acl_destroy(struct xsknf_gpu_acl *acl);

/* Change the rules of a live ACL: n ops applied in index order to the
 * exact-match map.  PUT stores the rule's key with its action or replaces the
 * key's action; DELETE removes the key (its action is ignored; an absent key is
 * no error); the last op on a key wins.  A PUT whose proto is neither 6 nor 17
 * is left out, as _create leaves such a rule out, and a DELETE of such a key
 * does nothing.
 *
 * Everything is validated before anything changes.  -EINVAL: a NULL acl, a NULL
 * ops with n > 0, an op other than 0 and 1.  -ENOSPC: the map after all ops
 * would hold `slots` or more distinct keys, or more than
 * XSKNF_GPU_ACL_MAX_RULES; the slot count never changes (a larger table is
 * _create's).  -ENOMEM.  In all these cases neither table is touched.  n == 0
 * succeeds and launches nothing.
 *
 * The host table is updated before the call returns: xsknf_gpu_firewall_host
 * and xsknf_gpu_lbfw_host see the new rules at once.  The device table, on the
 * current device (the one the ACL was created on), is updated asynchronously
 * on `stream` (a hipStream_t; NULL: the default stream): a batch enqueued on
 * that stream before the call sees the old rules, one enqueued after it the new
 * ones, and the host waits for nothing in between.  ops is not referenced
 * after the call returns: what the stream needs is copied into pinned buffers
 * that belong to the ACL, one per update in flight, reused once the stream has
 * passed them and released by _destroy.  A batch that reads this ACL on another
 * stream must be ordered against the update by the caller, with an event;
 * lookups that run beside an update are undefined (a slot's 16-byte key and its
 * 4-byte action are two stores).  -EIO on a HIP error (xsknf_gpu_last_error()):
 * the host table holds the new rules and the device table may not; destroy it.
 *
 * Once the stream has passed the update the device table equals the host table
 * byte for byte, keys and actions, in every slot; both are a deterministic
 * function of _create's arguments and the sequence of update calls.  An object
 * built in a process with no device visible updates its host table alone and
 * ignores `stream`.
 *
 * How (xsknf_amd/csrc/acl_table.h, acl.cpp): a deleted key's slot becomes the
 * tombstone {0, 0, 0, 0xffffffff}, which a probe walks over and no frame's key
 * equals; a new key takes the first tombstone of its probe sequence.  The
 * device receives one 24-byte record {slot, key, action} per changed slot and
 * scatters them (acl_update_device.hip).  When more than a quarter of the slots
 * would be tombstones, or no slot would stay empty, the call rebuilds the host
 * table in place (the live rules reinserted in ascending slot order, no
 * tombstone left) and sends the whole table instead. */
#define XSKNF_GPU_ACL_PUT 0u
#define XSKNF_GPU_ACL_DELETE 1u
struct xsknf_gpu_acl_op {
	struct xsknf_gpu_acl_rule rule;
	uint32_t op;             /* XSKNF_GPU_ACL_PUT or _DELETE */
};                           /* 24 bytes */
XSKNF_GPU_API int xsknf_gpu_acl_update(struct xsknf_gpu_acl *acl, const struct xsknf_gpu_acl_op *ops, uint32_t n,
		void *stream);
/* Every live rule of the host table (which == XSKNF_GPU_ACL_HOST_TABLE) or the
 * device table (_DEVICE_TABLE; waits for the device), ascending by {saddr, daddr,
 * sport | dport << 16, proto} compared as numbers in that order, pad 0.  *n_out
 * is the table's count; at most cap rules are written (-ENOSPC if cap is
 * smaller; rules_out may be NULL with cap 0).  For tests and monitoring.
 * -EINVAL for a NULL acl or n_out or another `which`; -ENODEV for the device
 * table of a host-only object. */
#define XSKNF_GPU_ACL_HOST_TABLE 0
#define XSKNF_GPU_ACL_DEVICE_TABLE 1
XSKNF_GPU_API int xsknf_gpu_acl_dump(const struct xsknf_gpu_acl *acl, int which, struct xsknf_gpu_acl_rule *rules_out,
		uint32_t cap, uint32_t *n_out);

/* Per-rule hit counters, as `iptables -v` and nft counters give them: opt-in
 * per ACL object.  An ACL that never calls _counters_enable behaves, allocates,
 * sends update records and launches exactly as without these calls.
 *
 * _counters_enable (with no batch and no update in flight; idempotent) gives
 * each table, host and device, one {packets, bytes} pair of uint64_t per slot as
 * a side array -- the 16-byte key slots and the action array keep their layout
 * -- and XSKNF_GPU_ACL_TOTALS uint64_t totals, all 0.  The device's share is
 * 16 bytes per slot plus 32 for the totals, part of device_bytes from this
 * call on; the first update that rebuilds the table (below) adds a second
 * counter array and a slot map, 20 bytes per slot more, from then on.
 *
 * Two independent sets, like the load balancer's two session tables: the host
 * set counts the frames of xsknf_gpu_firewall_host and xsknf_gpu_lbfw_host, the
 * device set those of xsknf_gpu_firewall_batch and xsknf_gpu_lbfw_batch, and
 * neither is ever copied into the other.  The host calls take the ACL as const
 * and still add to its host set, with plain adds: on an ACL with counters they
 * must be made one at a time (without counters they only read, as before).
 *
 * A frame that reaches rule 7 (in lbfw: rule 6a, the gate) and finds its key
 * adds 1 to that rule's packets and its descriptor's len to that rule's bytes,
 * whatever the action, 0 included.  The totals, over every frame handed to
 * such a call:
 *   [0] frames
 *   [1] frames that hit a rule
 *   [2] frames that reached the lookup and found no rule (in lbfw: the frames
 *       that go on to the load balancer)
 *   [3] frames decided before the lookup (rules 0-5, outside the UMEM)
 * [0] = [1] + [2] + [3], and [1] equals the sum of packets over the rules that
 * were live for the whole interval.  All adds are integer adds, exact whatever
 * their order; on the device they are device-scope atomics, so two batches on
 * two streams that read the same ACL both count in full.  A batch enqueued
 * before an update counts against the old rules, one enqueued after it against
 * the new ones.  An lbfw batch counts each frame once, whichever of its paths
 * it takes (the gate decides a frame in one place only).
 *
 * Updates, per table, in op order within a call: a PUT of a key the map holds
 * keeps that key's counters (replacing an action is not a new rule); a DELETE
 * of a present key ends them; a PUT of an absent key starts at 0/0 -- so DELETE
 * k followed by PUT k in one call resets k, even where k lands in the same
 * slot.  A rebuild carries every surviving key's counters to its new slot,
 * also past the puts and deletes of the same call.  The host table does all
 * this at once, the device table in stream order: the host waits for nothing
 * and reads nothing back, and once the stream has passed the update the
 * device's per-key counters are what applying the ops between the two
 * neighbouring batches gives.
 *
 * -EINVAL for NULL; -ENOMEM; -EIO on a HIP error.  A host-only object enables
 * and counts on the host alone. */
#define XSKNF_GPU_ACL_TOTALS 4
struct xsknf_gpu_acl_counter {
	uint64_t packets, bytes;
};
XSKNF_GPU_API int xsknf_gpu_acl_counters_enable(struct xsknf_gpu_acl *acl);
/* xsknf_gpu_acl_dump with counters_out[i] the counters of rules_out[i]: the
 * same order, cap, *n_out and -ENOSPC, -ENODEV for the device set of a
 * host-only object; the device form waits for the device.  totals_out (may be
 * NULL) receives the set's XSKNF_GPU_ACL_TOTALS totals.  -EINVAL, before any
 * work: a NULL acl, an object without counters, another `which`, a NULL n_out,
 * a NULL rules_out or counters_out with cap > 0. */
XSKNF_GPU_API int xsknf_gpu_acl_counters_dump(const struct xsknf_gpu_acl *acl, int which,
		struct xsknf_gpu_acl_rule *rules_out, struct xsknf_gpu_acl_counter *counters_out, uint32_t cap,
		uint32_t *n_out, uint64_t *totals_out);
/* Zero one set, counters and totals: the host set at once, the device set in
 * stream order on `stream` (ignored for the host set).  -EINVAL for a NULL acl,
 * an object without counters or another `which`; -ENODEV for the device set of
 * a host-only object; -EIO. */
XSKNF_GPU_API int xsknf_gpu_acl_counters_clear(struct xsknf_gpu_acl *acl, int which, void *stream);

/* verdicts[i] = the firewall's verdict for descs[i], i < n, on the current
 * device (the one the ACL was created on), asynchronously on `stream` (a
 * hipStream_t; NULL: the default stream).  umem (16-byte aligned), descs
 * (16-byte aligned) and verdicts (4-byte aligned) are device memory.  The frame
 * bytes are read as aligned 4-byte words that each hold at least one byte of
 * rule 0's [off, off + len), so up to 3 bytes around a frame at the UMEM's edge
 * are read with it: they lie inside any device allocation.  Nothing but
 * verdicts[0 .. n) is written.  n == 0 succeeds without a launch.  -EINVAL,
 * before any GPU call: a NULL acl, a misaligned umem, descs or verdicts, and
 * with n > 0 a NULL umem, descs or verdicts.  -EIO on a HIP error, with
 * xsknf_gpu_last_error() set. */
XSKNF_GPU_API int xsknf_gpu_firewall_batch(const uint8_t *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n, const struct xsknf_gpu_acl *acl, int32_t *verdicts,
		void *stream);
/* The same on host arrays over the ACL's host copy: one thread, byte reads
 * only, no GPU call and no alignment asked.  -EINVAL for a NULL acl and, with
 * n > 0, a NULL umem, descs or verdicts. */
XSKNF_GPU_API int xsknf_gpu_firewall_host(const uint8_t *umem, uint64_t umem_size,
		const struct xsknf_gpu_desc *descs, uint32_t n, const struct xsknf_gpu_acl *acl, int32_t *verdicts);

/* ---- the load balancer NF: session table, NAT rewrite, one verdict per frame ---
 * The reference's L4 load balancer with the per-frame callback
 * (examples/load_balancer/load_balancer_user.c:396-553, load_balancer.h): a
 * frame of a known session is rewritten towards its backend or its client; a
 * frame to a virtual service that has no session picks a backend, stores the
 * forward and the backward session and is rewritten; everything else passes.
 * These calls do that for a whole batch, on the device or (the model the device
 * is held to) on one CPU thread, with exactly the result of the reference's
 * loop: the frames of a batch are processed in index order against one table,
 * and a session stored by frame i is seen by every frame j > i.
 *
 * Per frame, with f and len as for the firewall (rule 0 gives off), nif =
 * num_interfaces and PASS = nif > 1 ? (ingress_ifindex + 1) % nif : -1:
 *   0. not (off <= umem_size && len <= umem_size - off)   -> -1, no byte touched
 *   1. len < 14                                           -> -1
 *   2. f[12..13] != 08 00                                 -> PASS
 *   3. len < 34                                           -> -1
 *   4. next = 14 + 4 * (f[14] & 15)        (not validated: 0..15)
 *   5. f[23] == 6: next + 20 > len -> -1;  f[23] == 17: next + 8 > len -> -1;
 *      any other protocol -> PASS
 *   6. sid = { saddr f[26..29], daddr f[30..33], sport f[next..next+1],
 *              dport f[next+2..next+3], proto f[23] } as the values lie in the frame
 *   7. the session table holds sid: its value `rep` is used, go to 10
 *   8. no service {daddr, dport, proto}                   -> PASS
 *   9. backend = the service's record number jhash(sid, 13 bytes, 0) % backends
 *      (the kernel's jhash, bit-exact); rep = {TO_BACKEND, its addr, port, mac,
 *      ifindex} is stored under sid; then {TO_CLIENT, daddr, dport, f[6..11],
 *      ingress_ifindex & 0xffff} is stored under {backend addr, saddr, backend
 *      port, sport, proto}, replacing the value of a key already there
 *  10. UPDATE, lines 521-550 in their order: rep.addr and rep.port replace the
 *      destination address and port (TO_BACKEND) or the source ones; f[6..11] =
 *      f[0..5], f[0..5] = rep.mac; the IPv4 check f[24..25] and then the L4
 *      check (f[next+16..] for TCP, f[next+6..] for UDP, a zero UDP check
 *      included) are updated incrementally with csum_add's end-around carry and
 *      the two-fold csum_fold of load_balancer.h:54-59, the complements of the
 *      old check and the old port taken after promotion to 32 bits.  For ihl < 5
 *      these fields overlap and the order of the reads and writes shows.
 *      The verdict is rep.ifindex (0..65535).
 *  11. with ageing enabled (xsknf_gpu_lb_aging_enable below): a frame that takes
 *      its session from the table (rule 7) stamps that session with the table's
 *      clock, and rule 9 stamps every session it stores with it, the forward
 *      one and the backward one whether new or replacing.  A failed insert
 *      stamps nothing, and neither does a frame that passes, is dropped, lies
 *      outside the UMEM or is decided by the lbfw NF's ACL (rule 6a).
 * Multi-byte values are the frame's bytes read little-endian, as the reference
 * reads them on the hosts it runs on.
 *
 * Deviations from the reference: services arrive as arrays (its load_services
 * leaves ifindex uninitialised for every interface but `local`: line 177
 * discards the result); a "missing backend" cannot occur (services are built
 * from their backend lists); where the reference overruns its element pool, an
 * insert of a new key into a table that holds max_sessions fails and the frame
 * is still rewritten (the reference's own `goto UPDATE` error path), a failed
 * forward insert skipping the backward one.  Nothing of its khashmap is kept:
 * the session table is open addressing over a power-of-two number of 32-byte
 * slots with the ACL's hash (xsknf_amd/csrc/lb_table.h); jhash only picks the
 * backend.
 *
 * The descriptors of a batch address disjoint byte ranges, which AF_XDP
 * guarantees; overlapping frames are undefined. */
#define XSKNF_GPU_LB_MAX_SERVICES 1024u       /* MAX_SERVICES, load_balancer.h */
#define XSKNF_GPU_LB_MAX_BACKENDS 131072u     /* MAX_BACKENDS */
#define XSKNF_GPU_LB_MAX_SESSIONS 2000000u    /* MAX_SESSIONS */
#define XSKNF_GPU_LB_MAX_SLOTS (1u << 24)
#define XSKNF_GPU_LB_MAX_BATCH (1u << 24)     /* frames per xsknf_gpu_lb_batch */
#define XSKNF_GPU_LB_TO_CLIENT 0              /* enum direction, load_balancer.h */
#define XSKNF_GPU_LB_TO_BACKEND 1
#define XSKNF_GPU_LB_HOST_TABLE 0             /* xsknf_gpu_lb_sessions_dump's `which` */
#define XSKNF_GPU_LB_DEVICE_TABLE 1
/* stats: [0] frames, [1] rewritten (reached UPDATE), [2] passed (a PASS rule,
 * whatever its value), [3] dropped (-1 by rules 0-5), [4] sessions created,
 * [5] inserts failed, [6] batches that took the ordered path, [7] 0 (the lbfw
 * NF below: frames its ACL decided) */
#define XSKNF_GPU_LB_STATS 8

/* One backend of one service.  A service's backend number is the record's order
 * among that service's records (the reference's file order). */
struct xsknf_gpu_lb_backend {
	uint32_t vaddr;          /* the service: network order */
	uint16_t vport;          /* network order */
	uint8_t proto;           /* 6 or 17 */
	uint8_t pad;             /* ignored */
	uint32_t addr;           /* the backend: network order */
	uint16_t port;           /* network order */
	uint8_t mac[6];
	uint16_t ifindex;        /* the verdict of a frame sent to this backend */
	uint8_t pad2[2];         /* ignored */
};

struct xsknf_gpu_lb_session_key {   /* struct session_id, padded to 16 bytes */
	uint32_t saddr, daddr;   /* network order */
	uint16_t sport, dport;   /* network order */
	uint8_t proto;           /* 6 or 17 */
	uint8_t pad[3];          /* ignored; 0 in a dump */
};

struct xsknf_gpu_lb_session_value {   /* struct replace_info in 16 bytes */
	uint32_t addr;
	uint16_t port;
	uint16_t ifindex;
	uint8_t mac[6];
	uint8_t dir;             /* XSKNF_GPU_LB_TO_CLIENT or _TO_BACKEND */
	uint8_t pad;             /* ignored; 0 in a dump */
};

struct xsknf_gpu_lb;         /* opaque */

struct xsknf_gpu_lb_info {
	uint32_t services, backends;
	uint32_t max_sessions, slots;
	uint32_t host_sessions;      /* stored in the host table */
	uint32_t device_sessions;    /* stored in the device table (synchronizes the device) */
	uint64_t device_bytes;       /* 0: built where no device was visible */
};

/* Build the service and backend tables from n records on the calling thread
 * (deterministic) and upload them to the current device together with an empty
 * session table of `slots` slots that holds at most max_sessions sessions; an
 * independent, equally sized host session table serves xsknf_gpu_lb_host.
 * slots == 0: the smallest power of two >= 2 * max_sessions, at least 64;
 * otherwise a power of two >= 2 * max_sessions, at most XSKNF_GPU_LB_MAX_SLOTS.
 * In a process that sees no HIP device the object is host-only (device_bytes
 * 0) and xsknf_gpu_lb_batch returns -ENODEV for it.  -EINVAL: a NULL lb_out, a
 * NULL backends with n > 0, a record whose proto is neither 6 nor 17, more than
 * XSKNF_GPU_LB_MAX_BACKENDS records or XSKNF_GPU_LB_MAX_SERVICES services,
 * max_sessions above XSKNF_GPU_LB_MAX_SESSIONS, a bad slots.  -ENOMEM; -EIO on
 * a HIP error (xsknf_gpu_last_error()). */
XSKNF_GPU_API int xsknf_gpu_lb_create(struct xsknf_gpu_lb **lb_out, const struct xsknf_gpu_lb_backend *backends,
		uint32_t n, uint32_t max_sessions, uint32_t slots);
XSKNF_GPU_API int xsknf_gpu_lb_info(const struct xsknf_gpu_lb *lb, struct xsknf_gpu_lb_info *info);
/* Free the tables on the device and the host (no batch may be in flight). */
XSKNF_GPU_API int xsknf_gpu_lb_destroy(struct xsknf_gpu_lb *lb);

/* Store n sessions in BOTH session tables, in order, a later value replacing an
 * earlier one of the same key (the reference's --passthrough and --local
 * modes).  Call it only with no batch in flight: it waits for the device and
 * rewrites the device table from the host.  Everything is validated before
 * anything is stored: -EINVAL for a NULL argument with n > 0, a dir other than
 * 0 and 1 or a proto other than 6 and 17.  -ENOSPC when a new key meets a table
 * that holds max_sessions: the sessions before it stay stored. */
XSKNF_GPU_API int xsknf_gpu_lb_sessions_put(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_session_key *keys,
		const struct xsknf_gpu_lb_session_value *values, uint32_t n);
/* Every session of the host table (which == XSKNF_GPU_LB_HOST_TABLE) or the
 * device table (_DEVICE_TABLE; waits for the device), ascending by {saddr, daddr,
 * sport | dport << 16, proto} compared as numbers in that order.  *n_out is the
 * table's count; at most cap records are written (-ENOSPC if cap is smaller).
 * For tests and monitoring.  -ENODEV for the device table of a host-only object. */
XSKNF_GPU_API int xsknf_gpu_lb_sessions_dump(const struct xsknf_gpu_lb *lb, int which,
		struct xsknf_gpu_lb_session_key *keys, struct xsknf_gpu_lb_session_value *values, uint32_t cap,
		uint32_t *n_out);

/* Removing sessions.  The two session tables are independent, so every call
 * names one: the plain forms work on the DEVICE table, asynchronously on
 * `stream`, on the device the object was made on; the _host forms work on the
 * host table on the calling thread.  A device form reads nothing back and the
 * host waits for nothing: a batch enqueued on that stream before the call sees
 * the old table, a batch enqueued after it the new one, and the table's count
 * drops by what was removed, so a table at max_sessions has room again.  `keys`
 * is host memory that is not referenced after the call returns.  result (host
 * forms) / result_dev (device forms: device memory, 8-byte aligned, written on
 * the stream) is XSKNF_GPU_LB_REMOVE_RESULT uint64 and may be NULL.
 *
 * _sessions_remove: set semantics over the table as it stands when the stream
 * reaches the call.  L = the listed keys that the table holds (duplicates
 * count once, an absent key is no error, a key whose proto is neither 6 nor 17
 * matches nothing; pad is ignored).  Without XSKNF_GPU_LB_REMOVE_PAIR exactly L
 * is removed.  With it the partner of each member of L goes too: for a
 * TO_BACKEND session {saddr, daddr, sport, dport, p} -> {addr, port} that is the
 * key {addr, saddr, port, sport, p} (rule 9's backward key), for a TO_CLIENT
 * one {daddr, addr, dport, port, p} -- but only if the table holds it, its
 * direction is the opposite one and its own partner is the listed key, so that
 * an unpaired _sessions_put entry or a backward session that another flow has
 * replaced takes no stranger with it.  Nothing is transitive.
 * result[_REMOVED] counts the distinct sessions removed.
 *
 * _drain_backend: every TO_BACKEND session whose value is {addr, port} and every
 * TO_CLIENT session whose key's source is {addr, port}, of protocol proto: both
 * halves of every flow of that backend.  The backend stays in its service
 * (xsknf_gpu_lb_backends_update takes it out).
 *
 * _sessions_clear: every session of one table (`which` as for _sessions_dump;
 * stream is used for the device table only).
 *
 * A removed slot stays a tombstone that lookups walk over and inserts do not
 * reuse; a removal that leaves more than slots / 4 of them rebuilds the table
 * free of tombstones (result[_COMPACTED] = 1), on the device without the host
 * knowing.  The first device removal allocates a spare table of the session
 * table's size, from then on part of device_bytes.  _sessions_put, _dump and
 * _info are correct on a table that has seen removals.
 *
 * Everything is validated before any work: -EINVAL for a NULL lb, a NULL keys
 * with n > 0, unknown flag bits, a misaligned result_dev, a proto other than 6
 * and 17 (_drain_backend) or a bad which.  -ENODEV for a device form on a
 * host-only object.  -ENOMEM.  -EIO on a HIP error (xsknf_gpu_last_error()).
 * n == 0 succeeds, launches nothing and writes zeros to a non-NULL result. */
#define XSKNF_GPU_LB_REMOVE_PAIR 1u           /* flags */
#define XSKNF_GPU_LB_REMOVED 0                /* result: sessions removed */
#define XSKNF_GPU_LB_COMPACTED 1              /* result: 1 if the table was rebuilt free of tombstones */
#define XSKNF_GPU_LB_REMOVE_RESULT 2
XSKNF_GPU_API int xsknf_gpu_lb_sessions_remove(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_session_key *keys,
		uint32_t n, uint32_t flags, uint64_t *result_dev, void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_sessions_remove_host(struct xsknf_gpu_lb *lb,
		const struct xsknf_gpu_lb_session_key *keys, uint32_t n, uint32_t flags, uint64_t *result);
XSKNF_GPU_API int xsknf_gpu_lb_drain_backend(struct xsknf_gpu_lb *lb, uint32_t addr, uint16_t port, uint8_t proto,
		uint64_t *result_dev, void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_drain_backend_host(struct xsknf_gpu_lb *lb, uint32_t addr, uint16_t port,
		uint8_t proto, uint64_t *result);
XSKNF_GPU_API int xsknf_gpu_lb_sessions_clear(struct xsknf_gpu_lb *lb, int which, void *stream);

/* Ageing: ending the flows that have been idle too long.  The reference leaves
 * this out ("This map should be handled in a LRU way ... This is not done for
 * simplicity", load_balancer_user.c:51-56); without it a table that has reached
 * max_sessions fails every new flow's insert until the caller names sessions to
 * remove, which it cannot: the batches create them on the device.  Ageing is
 * opt-in per object, and an object that never enables it behaves, allocates and
 * launches exactly as before.
 *
 * _aging_enable: call it with no batch in flight (it may wait for the device).
 * Each session table gets one uint32_t last-seen stamp per slot, a side array --
 * the slots' layout stays -- and a clock word.  Both clocks start at 0 and every
 * session already stored is stamped with its table's clock.  Idempotent.  The
 * device table's stamps and clock, 4 B per slot (64 MiB at
 * XSKNF_GPU_LB_MAX_SLOTS) and 16 B, are part of device_bytes; the spare table of
 * the removals gets stamps of the same size with its own allocation, or here
 * if it already exists.  From then on rule 11 holds for xsknf_gpu_lb_batch,
 * xsknf_gpu_lbfw_batch and their _host forms, _sessions_put stamps each
 * session it stores or replaces with the clock of the table it stores into, and
 * every rebuild of a table (after any removal) carries each surviving session's
 * stamp with it.
 *
 * _clock: sets one table's clock to `now`, in the caller's own unit (`which` as
 * for _sessions_dump).  The host table's clock changes at once.  The device
 * table's changes in stream order: a batch enqueued on `stream` before the call
 * stamps with the old value, a batch after it with the new one; the call reads
 * nothing back and waits for nothing.  All stamps of one batch are equal.
 *
 * _sessions_expire (device table, on `stream`) / _sessions_expire_host: set
 * semantics over the table as it stands when the stream reaches the call.
 * idle(k) = (uint32_t)(clock - stamp[k]) > max_idle; the subtraction is
 * unsigned, so a clock that wraps is handled as long as the caller keeps real
 * idle times below 2^32 ticks (expire before a session's stamp is a full turn
 * behind).  The checked partner of a session is REMOVE_PAIR's: the table holds
 * the partner key, its direction is the opposite one and its own partner is
 * this key.  A session is removed if and only if it is idle and either has no
 * checked partner or its checked partner is idle too: both halves of a flow
 * leave together or stay together, so a flow with traffic in one direction only
 * keeps its backward half.  A session without a checked partner -- an unpaired
 * _sessions_put entry, a backward session that another flow has replaced --
 * decides alone.  The result words, the tombstones, the rebuild past slots / 4,
 * the dropping counts, the spare table and a NULL result are the other
 * removals'.
 *
 * _sessions_ages: _sessions_dump's order, cap, n_out and -ENOSPC, with ages[i] =
 * (uint32_t)(clock - stamp) in place of the value and the table's clock in
 * *clock_out (may be NULL).  The device table's form waits for the device.  For
 * tests and monitoring.
 *
 * Everything is validated before any work.  -EINVAL: a NULL lb, an object
 * without ageing (_clock, _sessions_expire*, _sessions_ages), a bad which, a
 * misaligned result_dev, a NULL n_out, or NULL keys or ages with cap > 0.
 * -ENODEV for the device table of a host-only object.  -ENOMEM.  -EIO on a HIP
 * error (xsknf_gpu_last_error()). */
XSKNF_GPU_API int xsknf_gpu_lb_aging_enable(struct xsknf_gpu_lb *lb);
XSKNF_GPU_API int xsknf_gpu_lb_clock(struct xsknf_gpu_lb *lb, int which, uint32_t now, void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_sessions_expire(struct xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result_dev,
		void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_sessions_expire_host(struct xsknf_gpu_lb *lb, uint32_t max_idle, uint64_t *result);
XSKNF_GPU_API int xsknf_gpu_lb_sessions_ages(const struct xsknf_gpu_lb *lb, int which,
		struct xsknf_gpu_lb_session_key *keys, uint32_t *ages, uint32_t cap, uint32_t *n_out, uint32_t *clock_out);

/* The services and backends of a live object.  The object's services are the
 * ordered record list xsknf_gpu_lb_create was given; the n ops edit that list
 * in index order.
 *   ADD     if the record's service {vaddr, vport, proto} holds one or more
 *           backends with the record's {addr, port}, their mac and ifindex are
 *           replaced and their backend numbers stay.  Otherwise the record is
 *           appended as the last backend of its service; a service that does
 *           not exist is created.
 *   REMOVE  every backend {addr, port} of that service is removed and the
 *           service's later backends move down by one number each.  An absent
 *           backend or service is no error; mac and ifindex are ignored.  A
 *           service left with no backend ceases to exist: rule 8 then passes
 *           its new flows.
 * After the call the object behaves, for every later batch, exactly as one made
 * by xsknf_gpu_lb_create from the edited list: the same backend numbers feed
 * rule 9's jhash % backends.  The order of services among themselves shows
 * nowhere.  Neither session table is touched: a stored session keeps the addr,
 * port, mac and ifindex it was stored with, and the flows of a removed backend
 * go on until they are drained (xsknf_gpu_lb_drain_backends below).
 *
 * Host and device, as for xsknf_gpu_acl_update: the host copy is new before the
 * call returns -- xsknf_gpu_lb_host, xsknf_gpu_lbfw_host and xsknf_gpu_lb_info
 * (services, backends) see it at once -- and the device copy is updated
 * asynchronously on `stream`, on the device the object was made on.  A batch of
 * either NF enqueued on that stream before the call sees the old services, one
 * enqueued after it the new ones; other streams are the caller's to order with
 * an event.  The call waits for nothing (the allocations of a first call
 * excepted).  ops is not referenced after the return: what the stream needs is
 * copied into pinned buffers that belong to the object, one per update in
 * flight, reused once the stream has passed it and freed by
 * xsknf_gpu_lb_destroy.  The first update of an object with a device half
 * allocates a region for the largest tables (2 * XSKNF_GPU_LB_MAX_SERVICES
 * service slots and XSKNF_GPU_LB_MAX_BACKENDS backends, 2.03 MiB), from then on
 * part of device_bytes; the tables of creation stay allocated until _destroy,
 * for the batches that were enqueued before.  A host-only object updates its
 * host copy and ignores stream.
 *
 * Everything is validated before anything changes.  -EINVAL: a NULL lb, a NULL
 * ops with n > 0, an op other than 0 and 1, a proto other than 6 and 17 (ADD or
 * REMOVE).  -ENOSPC: the list after all ops would hold more than
 * XSKNF_GPU_LB_MAX_BACKENDS records or more than XSKNF_GPU_LB_MAX_SERVICES
 * services.  -ENOMEM.  In all these cases neither copy changes.  n == 0
 * succeeds and launches nothing.  -EIO on a HIP error (xsknf_gpu_last_error()):
 * the host copy is new, the device copy may not be; destroy the object.
 *
 * _backends_dump: the records of the host copy (which ==
 * XSKNF_GPU_LB_HOST_TABLE) or of the device copy (_DEVICE_TABLE: waits for the
 * device, reads its two tables back and decodes them), services ascending by
 * {vaddr, vport | proto << 16} compared as numbers, each service's backends by
 * number, pads 0.  cap, n_out, -ENOSPC and -ENODEV are as for _sessions_dump.
 * Once the stream has passed an update the two dumps are equal.
 *
 * _drain_backends: the union, over the n listed backends, of what
 * _drain_backend removes -- both halves of every flow of each -- on the table as
 * it stands when the stream reaches the call, in ONE pass over the table
 * whatever n is.  Duplicates count once; pad is ignored.  The result words, the
 * tombstones, the rebuild past slots / 4 and the first device removal's spare
 * table are the other removals'; so are the errors and n == 0, plus -EINVAL for
 * a listed proto other than 6 and 17 and for n > XSKNF_GPU_LB_MAX_BACKENDS.
 * list is not referenced after the return.
 *
 * Taking backends out of service: _backends_update (REMOVE) first, then
 * _drain_backends on the same stream.  No batch between the two can then open a
 * new flow to a backend that has already been drained. */
#define XSKNF_GPU_LB_BACKEND_ADD 0u
#define XSKNF_GPU_LB_BACKEND_REMOVE 1u
struct xsknf_gpu_lb_backend_op {
	struct xsknf_gpu_lb_backend backend;
	uint32_t op;
};
struct xsknf_gpu_lb_backend_id {
	uint32_t addr;           /* network order */
	uint16_t port;           /* network order */
	uint8_t proto;           /* 6 or 17 */
	uint8_t pad;             /* ignored */
};
XSKNF_GPU_API int xsknf_gpu_lb_backends_update(struct xsknf_gpu_lb *lb,
		const struct xsknf_gpu_lb_backend_op *ops, uint32_t n, void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_backends_dump(const struct xsknf_gpu_lb *lb, int which,
		struct xsknf_gpu_lb_backend *records, uint32_t cap, uint32_t *n_out);
XSKNF_GPU_API int xsknf_gpu_lb_drain_backends(struct xsknf_gpu_lb *lb, const struct xsknf_gpu_lb_backend_id *list,
		uint32_t n, uint64_t *result_dev, void *stream);
XSKNF_GPU_API int xsknf_gpu_lb_drain_backends_host(struct xsknf_gpu_lb *lb,
		const struct xsknf_gpu_lb_backend_id *list, uint32_t n, uint64_t *result);

/* Bytes of device workspace a batch of n frames needs (16-byte aligned, the
 * caller's, as for the router; its contents mean nothing between calls).
 * -EINVAL for a NULL bytes or n > XSKNF_GPU_LB_MAX_BATCH. */
XSKNF_GPU_API int xsknf_gpu_lb_workspace(uint32_t n, uint64_t *bytes);

/* One batch on the current device (the one lb was created on), asynchronously
 * on `stream`; nothing is read back by the call.  umem, descs (16-byte aligned),
 * verdicts (4-byte aligned), workspace (16-byte aligned) and stats_dev (8
 * uint64, 8-byte aligned, zeroed on the stream first) are device memory.
 * Written: verdicts[0 .. n), the bytes rule 10 changes in the frames that reach
 * UPDATE -- by byte and aligned 2-byte stores that lie inside the frame, so a
 * neighbour that shares a word with it is never touched --, the device session
 * table, the workspace and stats_dev.  Nothing else.  Frame bytes are read as
 * aligned 4-byte words that each hold a byte of the frame (see
 * xsknf_gpu_firewall_batch).
 * Batches whose sessions can be created independently run one lane per frame;
 * a batch in which two flows store the same session key, a stored key would
 * replace an older session, or the new sessions do not all fit is run by the
 * ordered path, ONE lane that walks the loop: exact, and slow (stats[6]).
 * n == 0 succeeds with nothing touched.  -EINVAL, before any GPU call: a NULL lb
 * or stats_dev, a misaligned pointer, n > XSKNF_GPU_LB_MAX_BATCH, and with n > 0
 * a NULL umem, descs, verdicts or workspace or workspace_bytes below
 * xsknf_gpu_lb_workspace(n).  -ENODEV for a host-only lb.  -EIO on a HIP error,
 * with xsknf_gpu_last_error() set. */
XSKNF_GPU_API int xsknf_gpu_lb_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, uint32_t num_interfaces, struct xsknf_gpu_lb *lb,
		int32_t *verdicts, void *workspace, uint64_t workspace_bytes, uint64_t *stats_dev, void *stream);
/* The same on host arrays over the host session table: one thread, the loop
 * above with byte reads and writes in the reference's order, no GPU call and no
 * alignment asked.  stats (8 uint64, may be NULL) is overwritten. */
XSKNF_GPU_API int xsknf_gpu_lb_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, uint32_t num_interfaces, struct xsknf_gpu_lb *lb,
		int32_t *verdicts, uint64_t *stats);

/* ---- the lbfw NF: the firewall's ACL as a gate in front of the load balancer ---
 * The reference's examples/lbfw (lbfw_user.c:420-594): the load balancer's
 * per-frame function with exactly two differences.  Everything else -- rules
 * 0-10, the loop's order, the two-fold csum_fold, the byte order for ihl < 5,
 * the full-table deviation, the store widths -- is the load balancer's above.
 *   PASS = (ingress_ifindex + 1) % nif at all three places (rules 2, 5, 8):
 *        one interface passes to interface 0, not -1.  nif == 0, where the
 *        reference divides by zero, is -EINVAL before any work.
 *   6a.  between rules 6 and 7: if the ACL holds sid, the verdict is that
 *        rule's action -- any int32, an action of 0 being a hit like any other
 *        -- the frame is not touched, and no session is looked up or stored.
 *        A sid the ACL does not hold goes on to rules 7-10.
 * The gate is the reference's MODE_AF_XDP.  In its MODE_COMBINED the XDP
 * program has applied the ACL already and the function skips it: here that is
 * acl == NULL (rule 6a never applies; PASS is still lbfw's).
 *
 * The calls work on the existing objects: an xsknf_gpu_acl (only read) and an
 * xsknf_gpu_lb, whose session tables are the ones xsknf_gpu_lb_batch and
 * xsknf_gpu_lb_host use: calls of both NFs on one object may alternate on one
 * stream.  The workspace is xsknf_gpu_lb_workspace(n).  stats are the load
 * balancer's with [7] = the frames the ACL decided, which count in none of
 * [1], [2], [3]: [0] = [1] + [2] + [3] + [7].
 *
 * xsknf_gpu_lbfw_batch: arguments, alignment, what is written, the ordered
 * path, n == 0 and the errors are xsknf_gpu_lb_batch's, on the current device
 * (the one BOTH objects were created on); a frame the gate decides is never
 * part of a reason for the ordered path.  In addition -EINVAL for
 * num_interfaces == 0 (first of all) and -ENODEV for an lb or a non-NULL acl
 * without a device half.  xsknf_gpu_lbfw_host: as xsknf_gpu_lb_host, over the
 * host session table and the ACL's host copy; -EINVAL for num_interfaces == 0. */
XSKNF_GPU_API int xsknf_gpu_lbfw_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, uint32_t num_interfaces, const struct xsknf_gpu_acl *acl /* may be NULL */,
		struct xsknf_gpu_lb *lb, int32_t *verdicts, void *workspace, uint64_t workspace_bytes, uint64_t *stats_dev,
		void *stream);
XSKNF_GPU_API int xsknf_gpu_lbfw_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, uint32_t num_interfaces, const struct xsknf_gpu_acl *acl /* may be NULL */,
		struct xsknf_gpu_lb *lb, int32_t *verdicts, uint64_t *stats);

/* ---- the macswap NF: every frame's two MAC addresses exchanged in place ------
 * The reference's examples/macswap with the per-frame callback
 * (macswap_user.c:34-50, macswap.h:6-36): exchange the destination and the
 * source MAC address and send the frame back out.  It is the NF the reference's
 * "pure I/O" figures are taken with; here it is the batch path with next to
 * nothing to do per frame.  These calls do it for a whole batch, on the device
 * or (the model the device is held to) on one CPU thread.  The verdicts are
 * what xsknf_gpu_route_batch consumes.
 *
 * Per frame, with f and len as for the firewall (rule 0 gives off):
 *   0. not (off <= umem_size && len <= umem_size - off)   -> -1, no byte read or written
 *   1. len < 14                                           -> -1, the frame untouched
 *                                                            whatever the action
 *   2. f[0..5] and f[6..11] are exchanged; with double_macswap != 0 they are
 *      exchanged twice (swap_mac_addresses, then swap_mac_addresses_v2), so
 *      every byte is as it was
 *   3. action DROP                                        -> -1
 *      action REDIRECT and action PASS                    -> (int32_t)((ingress_ifindex + 1u)
 *                                                            % num_interfaces)
 *      in 32-bit unsigned arithmetic: ingress 0xFFFFFFFF gives 0.
 * A quirk kept: on the AF_XDP path the reference's PASS is a REDIRECT (line 48
 * tests for DROP alone; only its XDP program hands a PASS frame to the stack).
 *
 * Deviations from the reference: rule 0 (the kernel's rx validation never shows
 * the reference such a descriptor); num_interfaces == 0 with an action other
 * than DROP, where the reference divides by zero, is -EINVAL; with
 * double_macswap the device call may leave the frame unread and unwritten (the
 * reference does the work twice so as to time it; the bytes come out the same).
 *
 * The descriptors of a batch address disjoint byte ranges, which AF_XDP
 * guarantees; overlapping frames are undefined.
 *
 * The store contract.  The only bytes stored are [off, off + 12) of the frames
 * that pass rules 0 and 1, and verdicts[0 .. n).  No store covers a byte
 * outside them, not even with the value that was read there: two 14-byte frames
 * packed back to back at an odd offset share an aligned 4-byte word, and a lane
 * that rewrote the whole word would race with its neighbour's.  The device
 * stores the aligned 4-byte words that lie wholly inside the 12 bytes as words
 * and the edges as bytes and aligned 2-byte halves.  Frame bytes are READ as the
 * aligned 4-byte words that hold a byte of [off, off + 12), so up to 3 bytes
 * around them are read with them (see xsknf_gpu_firewall_batch). */
#define XSKNF_MACSWAP_ACTION_REDIRECT 0   /* enum action, examples/macswap/macswap_user.c:18-22 */
#define XSKNF_MACSWAP_ACTION_DROP 1
#define XSKNF_MACSWAP_ACTION_PASS 2

/* The globals the reference callback reads (macswap_user.c:28-29, :32). */
struct xsknf_macswap_opts {
	uint32_t action;           /* opt_action (-c REDIRECT|DROP|PASS), default REDIRECT */
	uint32_t double_macswap;   /* opt_double_macswap (-d): 0, or anything else for twice */
	uint32_t num_interfaces;   /* config.num_interfaces (must be >= 1 unless action is DROP) */
	uint32_t reserved;         /* must be 0 */
};

/* One batch on the current device, asynchronously on `stream` (a hipStream_t;
 * NULL: the default stream).  umem (16-byte aligned), descs (16-byte aligned)
 * and verdicts (4-byte aligned) are device memory; opts is host memory, read at
 * the call: it may be changed as soon as the call returns.  Written: what the
 * store contract above names, nothing else.  n == 0 succeeds without a launch.
 * -EINVAL, before any GPU call: a NULL opts, an action above 2, a nonzero
 * reserved, num_interfaces == 0 with an action other than DROP (the validation
 * of xsknf_gpu_checksum_batch: the same callback line); a misaligned umem,
 * descs or verdicts; with n > 0 a NULL umem, descs or verdicts.  -EIO on a HIP
 * error, with xsknf_gpu_last_error() set. */
XSKNF_GPU_API int xsknf_gpu_macswap_batch(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, const struct xsknf_macswap_opts *opts, int32_t *verdicts,
		void *stream);
/* The same on host arrays: one thread, byte reads and writes only (both
 * exchanges of a double swap are carried out), no GPU call and no alignment
 * asked.  -EINVAL for the opts as above and, with n > 0, a NULL umem, descs or
 * verdicts. */
XSKNF_GPU_API int xsknf_gpu_macswap_host(uint8_t *umem, uint64_t umem_size, const struct xsknf_gpu_desc *descs,
		uint32_t n, uint32_t ingress_ifindex, const struct xsknf_macswap_opts *opts, int32_t *verdicts);

/* Text of the last HIP error seen by this library, on any thread (a copy
 * private to the calling thread). */
XSKNF_GPU_API const char *xsknf_gpu_last_error(void);

/* Pool guard of the current device (synchronizes it first): how many waves of
 * the pooled split kernel found a unit of their block that no wave claimed
 * (its frames left unsummed).  The launch's grid bound makes this unreachable;
 * a nonzero count is a library bug.  reset != 0 zeroes the count after reading.
 * No reference counterpart (a device-side invariant check for tests and
 * monitoring). */
XSKNF_GPU_API int xsknf_gpu_pool_guard_trips(uint32_t *trips, int reset);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* XSKNF_GPU_H */
