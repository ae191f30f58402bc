#!/usr/bin/env python3
"""Forwarding routed frames into their tx interface's UMEM, device against its
yardsticks.

Two batches, each resident on device 0, checksummed and routed there first:
  config3   1,048,576 frames of 1500 B, one per 2 KiB chunk;
  config4   8,388,608 IMIX frames;
each forwarded twice:
  one     one interface whose UMEM is not the rx UMEM: every frame copied;
  three   three interfaces, the middle one sharing the rx UMEM: the forwarded
          frames' verdicts are rewritten to frame index mod 3 before the route,
          so two thirds of the frames are copied, into two UMEMs.

  dev:     xsknf_gpu_forward_frames, enqueued only (stats NULL), on HIP events
           around each call, after --warmup calls, --reps times;
  memcpy:  one contiguous device-to-device copy of as many bytes as the frames
           hold (torch's Tensor.copy_ between two contiguous uint8 tensors of
           one device, a hipMemcpyAsync), timed the same way;
  bound:   (2 x frame bytes + 16 B per entry) over the HBM peak;
  host:    the caller's wall time around the copies of the tx lists, the counts
           and the rx UMEM to the host, xsknf_gpu_forward_host on one thread
           and the copies of the destination UMEMs back, best of --host-reps.

The device's destination UMEMs and stats are compared with the host's (every
byte).  One JSON line per case, to stdout and to --out.

  python tools/forward_measure.py [--reps 20] [--warmup 3] [--host-reps 3] [--scale 1] [--out FILE]

A/B of the destination stores: build the library with -DXSKNF_FORWARD_NT=1 into
another directory, run this with XSKNF_GPU_LIB=<that library> --variant nontemporal-stores.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0   # MI355X HBM3E peak, TB/s


def timed(fn, stream, warmup, reps):
    """fn() enqueues on `stream`; milliseconds on events, sorted."""
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the frame counts (rehearsals)")
    ap.add_argument("--batches", default="config3,config4")
    ap.add_argument("--variant", default="plain-stores", help="a label for the library measured (XSKNF_GPU_LIB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import Checksummer, ChecksummerOptions, _lib, frames, route

    if not torch.cuda.is_available():
        sys.exit("forward_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    lines, ok = [], True
    for name, n0, length in (("config3", 1 << 20, 1500), ("config4", 8 << 20, "imix")):
        if name not in a.batches.split(","):
            continue
        n = max(1, int(n0 * a.scale))
        for case, nif, ingress in (("one", 1, 0), ("three", 3, 1)):
            umem, dd, lens = frames.device_batch(n, length, device=dev)
            cs = Checksummer(ChecksummerOptions(), num_interfaces=nif, frame_len_hint=int(lens.max()),
                             frame_len_mean=int(lens.mean()))
            v = cs.process_batch(umem, dd, ingress_ifindex=ingress)
            if nif == 3:   # the forwarded frames dealt to the three interfaces in turn
                i3 = (torch.arange(n, device=dev, dtype=torch.int32) % 3)
                v = torch.where(v >= 0, i3, v).contiguous()
            tx = torch.empty((n, 2), dtype=torch.int64, device=dev)
            fill = torch.empty(n, dtype=torch.int64, device=dev)
            ws = torch.empty(route.route_workspace(n, nif) // 8, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev)
            counts = route.route_batch_ptr(dd.data_ptr(), v.data_ptr(), n, nif, tx.data_ptr(), fill.data_ptr(), 0,
                                           ws.data_ptr(), ws.numel() * 8, stream.cuda_stream)
            own = [i for i in range(nif) if not (nif == 3 and i == 1)]
            dsts = [torch.full((umem.numel(),), 0xA5, dtype=torch.uint8, device=dev) if i in own else None
                    for i in range(nif)]
            stats_dev = torch.zeros(3, dtype=torch.int64, device=dev)
            ptrs = [0 if t is None else t.data_ptr() for t in dsts]
            sizes = [0 if t is None else t.numel() for t in dsts]

            def call(sync=False):
                return route.forward_frames_ptr(umem.data_ptr(), umem.numel(), ptrs, sizes, tx.data_ptr(),
                                                ws.data_ptr(), n, stats_dev.data_ptr(), stream.cuda_stream, sync=sync)

            ev = timed(call, stream, a.warmup, a.reps)
            stats = call(True)
            entries = sum(counts[i] for i in own)
            # the contiguous copy of the same bytes
            src = torch.empty(max(stats[1], 16), dtype=torch.uint8, device=dev).fill_(1)
            dst = torch.empty_like(src)
            cp = timed(lambda: dst.copy_(src, non_blocking=True), stream, a.warmup, a.reps)
            del src, dst
            # the host way
            print(f"forward_measure: {name}/{case}: host way x{a.host_reps}", file=sys.stderr, flush=True)
            host_ms, same = [], None      # (no host run: nothing compared)
            for r in range(a.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                htx = tx.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)
                hcounts = [int(c) for c in ws[:nif + 1].cpu().numpy().view(np.uint64)]
                hrx = umem.cpu().numpy()
                hd = [None if t is None else np.full(t.numel(), 0xA5, dtype=np.uint8) for t in dsts]
                hstats = route.forward_host(hrx, hd, htx, hcounts)
                back = [None if h is None else torch.from_numpy(h).to(dev) for h in hd]
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    same = hstats == stats and all(t is None or torch.equal(t, b) for t, b in zip(dsts, back))
                del back, hd, hrx
                print(f"forward_measure:   {host_ms[-1]:.0f} ms", file=sys.stderr, flush=True)
            ok = ok and same is not False
            nbytes = 2 * stats[1] + 16 * entries
            bound_us = nbytes / (HBM_TBS * 1e12) * 1e6
            med, cmed = ev[len(ev) // 2] * 1e3, cp[len(cp) // 2] * 1e3
            lines.append({"batch": name, "case": case, "frames": n, "num_interfaces": nif, "counts": counts,
                          "stats": stats, "equal_host": same, "reps": a.reps,
                          "variant": a.variant, "lib": os.path.relpath(_lib.LIB_PATH),
                          "forward_event_us_median": med, "forward_event_us_min": ev[0] * 1e3,
                          "forward_event_us_max": ev[-1] * 1e3,
                          "memcpy_bytes": stats[1], "memcpy_event_us_median": cmed, "memcpy_event_us_min": cp[0] * 1e3,
                          "memcpy_event_us_max": cp[-1] * 1e3, "median_over_memcpy": med / cmed,
                          "bytes": nbytes, "bound_us": bound_us, "median_over_bound": med / bound_us,
                          "copied_tbs": 2 * stats[1] / (med * 1e-6) / 1e12,
                          "host_way_ms_min": min(host_ms) if host_ms else None,
                          "host_way_over_median": min(host_ms) * 1e3 / med if host_ms else None})
            print(json.dumps(lines[-1]), flush=True)
            del umem, dd, v, tx, fill, ws, dsts
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
