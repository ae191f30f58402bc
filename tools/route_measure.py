#!/usr/bin/env python3
"""Routing a checksummed batch, device against host.

Two batches, each resident on device 0 and checksummed there first:
  config4   8,388,608 IMIX frames, one per 2 KiB chunk;
  config3   1,048,576 frames of 1500 B;
each routed twice: one interface (ingress 0), and three interfaces (ingress 1)
with 1 % of the frames turned into edge cases (short, non-IPv4, non-UDP), so
that the drop list and two tx lists are in play.

  dev:  xsknf_gpu_route_batch with `order`, enqueued only (counts NULL), on HIP
        events around each call, after --warmup calls, --reps times; and the
        same with the counts read back, on the host's clock (the call waits);
  host: the caller's wall time around the copies of the verdicts and the
        descriptors to the host plus xsknf_gpu_route_host on one thread.

Both give the same lists (checked, every entry).  The bound is the bytes the
three passes move (kernel_route.h: 4 B of verdict in pass 1; 4 + 16 B read and
16 B per tx frame or 8 B per drop written in pass 3, 4 B more for `order`) over
the HBM peak.  One JSON line per case, to stdout and to --out.

  python tools/route_measure.py [--reps 20] [--warmup 3] [--scale 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0   # MI355X HBM3E peak, TB/s


def edge_cases(umem, descs, n, frac, seed):
    """~frac of the frames of an aligned device batch into branches the
    reference distinguishes: IPv6 ethertype, TCP, a length below the headers."""
    import torch
    from xsknf_amd import frames

    rng = np.random.default_rng(seed)
    sel = np.sort(rng.choice(n, size=int(round(n * frac)), replace=False))
    rows = umem.view(n, frames.CHUNK)
    k = [torch.from_numpy(sel[j::3]).to(umem.device) for j in range(3)]
    rows[k[0], frames.HEADROOM + 12] = 0x86
    rows[k[0], frames.HEADROOM + 13] = 0xDD
    rows[k[1], frames.HEADROOM + 23] = 6
    d = descs.view(torch.int32).view(n, 4)
    d[k[2], 2] = 20
    return int(sel.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the frame counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import Checksummer, ChecksummerOptions, frames, route

    if not torch.cuda.is_available():
        sys.exit("route_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    lines, ok = [], True
    for name, n0, length in (("config4", 8 << 20, "imix"), ("config3", 1 << 20, 1500)):
        n = max(1, int(n0 * a.scale))
        for nif, ingress, edge in ((1, 0, 0.0), (3, 1, 0.01)):
            umem, dd, lens = frames.device_batch(n, length, device=dev)
            nedge = edge_cases(umem, dd, n, edge, frames.SEED + 7) if edge else 0
            cs = Checksummer(ChecksummerOptions(), num_interfaces=nif, frame_len_hint=int(lens.max()),
                             frame_len_mean=int(lens.mean()))
            v = cs.process_batch(umem, dd, ingress_ifindex=ingress)
            tx = torch.empty((n, 2), dtype=torch.int64, device=dev)
            fill = torch.empty(n, dtype=torch.int64, device=dev)
            od = torch.empty(n, dtype=torch.int32, device=dev)
            ws = torch.empty(route.route_workspace(n, nif) // 8, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev)

            def call(sync):
                return route.route_batch_ptr(dd.data_ptr(), v.data_ptr(), n, nif, tx.data_ptr(), fill.data_ptr(),
                                             od.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream.cuda_stream,
                                             sync=sync)

            for _ in range(a.warmup):
                call(False)
            torch.cuda.synchronize()
            ev_ms, wall_ms = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(False)
                e1.record(stream)
                e1.synchronize()
                ev_ms.append(e0.elapsed_time(e1))
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                counts = call(True)
                wall_ms.append((time.perf_counter() - t0) * 1e3)
            # the host way: verdicts and descriptors home, then one thread
            host_ms, d2h_ms = [], []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hv = v.cpu().numpy()
                hd = dd.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)
                t1 = time.perf_counter()
                htx, hfill, hod, hcounts = route.route_host(hd, hv, nif, order=True)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                d2h_ms.append((t1 - t0) * 1e3)
            ntx, ndrop = sum(hcounts[:nif]), hcounts[nif]
            same = (counts == hcounts
                    and np.array_equal(tx.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)[:ntx], htx[:ntx])
                    and np.array_equal(fill.cpu().numpy().view(np.uint64)[:ndrop], hfill[:ndrop])
                    and np.array_equal(od.cpu().numpy().view(np.uint32), hod))
            ok = ok and same
            nbytes = 4 * n + 20 * n + 16 * ntx + 8 * ndrop + 4 * n
            bound_us = nbytes / (HBM_TBS * 1e12) * 1e6
            ev_ms.sort()
            lines.append({"batch": name, "frames": n, "num_interfaces": nif, "ingress": ingress, "edge_frames": nedge,
                          "counts": counts, "lists_equal_host": bool(same), "reps": a.reps,
                          "route_event_us_median": ev_ms[len(ev_ms) // 2] * 1e3, "route_event_us_min": ev_ms[0] * 1e3,
                          "route_event_us_max": ev_ms[-1] * 1e3,
                          "route_with_counts_wall_us_median": sorted(wall_ms)[len(wall_ms) // 2] * 1e3,
                          "route_with_counts_wall_us_min": min(wall_ms) * 1e3,
                          "bytes": nbytes, "bound_us": bound_us,
                          "median_over_bound": ev_ms[len(ev_ms) // 2] * 1e3 / bound_us,
                          "host_way_ms_min": min(host_ms), "host_d2h_ms_min": min(d2h_ms)})
            print(json.dumps(lines[-1]), flush=True)
            del umem, dd, v, tx, fill, od, ws
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
