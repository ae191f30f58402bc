#!/usr/bin/env python3
"""The macswap NF's device pass against its bound, the firewall's read-only
pass and the host way: what the batch path costs when the NF does
next to nothing.

Three batches resident on device 0, one frame per 2 KiB chunk:
  config2   1,048,576 frames of 64 B;
  config3   1,048,576 frames of 1500 B;
  config4   8,388,608 IMIX frames.

Per batch, interleaved in one process, each enqueued only, on HIP events around
the call, after --warmup calls, --reps times (median, min and max):
  swap      xsknf_gpu_macswap_batch, REDIRECT, single swap;
  double    the same with double_macswap (the frames are not touched);
  firewall  xsknf_gpu_firewall_batch with an empty ACL: the existing code with
            the same descriptor read, header sector read and verdict store, and
            no frame store.
The figure to take away is swap minus firewall: what a 12-byte in-place rewrite
costs on this path.  The host way, once per batch: the caller's wall time
around a gather of every frame's first 16 bytes on the device, their copy and
the descriptors' to the host, and xsknf_gpu_macswap_host on one thread.

The device's frames and verdicts are checked against the host model on every
frame.  The bound is the least bytes the pass moves -- 16 B descriptor, one
64 B line read and written back, 4 B verdict -- over the HBM peak; the yardstick
is this project's own 64 B read probe at a 2 KiB stride, 28 us per 1M sectors
(DESIGN 3).  One JSON line per row, to stdout and to --out.

  python tools/macswap_measure.py [--reps 20] [--warmup 3] [--scale 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0            # MI355X HBM3E peak, TB/s
PROBE_US_PER_M = 28.0    # 64 B read probe, 2 KiB stride
WINDOW = 16              # bytes of a frame the host way brings home (12 are exchanged)
FRAME_BYTES = 16 + 64 + 64 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the frame counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import firewall, frames, macswap

    if not torch.cuda.is_available():
        sys.exit("macswap_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    acl = firewall.Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE))
    lines, ok = [], True
    H = frames.HEADROOM
    for name, n0, length in (("config2", 1 << 20, 64), ("config3", 1 << 20, 1500), ("config4", 8 << 20, "imix")):
        n = max(1, int(n0 * a.scale))
        umem, dd, lens = frames.device_batch(n, length, device=dev)
        rows = umem.view(n, frames.CHUNK)
        v = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        before = rows[:, H:H + WINDOW].contiguous().cpu().numpy()

        def swap(double=False):
            macswap.macswap_batch_ptr(umem.data_ptr(), umem.numel(), dd.data_ptr(), n, 0, v.data_ptr(),
                                      stream.cuda_stream, double_macswap=double, num_interfaces=2)

        calls = {"swap": swap, "double": lambda: swap(True),
                 "firewall": lambda: firewall.firewall_batch_ptr(umem.data_ptr(), umem.numel(), dd.data_ptr(), n, acl,
                                                                 v.data_ptr(), stream.cuda_stream)}
        for _ in range(a.warmup):   # an even number of swaps in all leaves the frames as they began
            for c in calls.values():
                c()
        torch.cuda.synchronize()
        ev = {k: [] for k in calls}
        swaps = a.warmup
        for _ in range(a.reps):
            for k, c in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                c()
                e1.record(stream)
                e1.synchronize()
                ev[k].append(e0.elapsed_time(e1) * 1e3)
            swaps += 1
        if swaps % 2:
            swap()
        torch.cuda.synchronize()
        same_start = bool(np.array_equal(rows[:, H:H + WINDOW].contiguous().cpu().numpy(), before))
        # the host way: 16 bytes per frame and the descriptors home, then one thread
        t0 = time.perf_counter()
        hu = rows[:, H:H + WINDOW].contiguous().cpu().numpy().reshape(-1)
        hd = dd.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1).copy()
        t1 = time.perf_counter()
        hd["addr"] = np.arange(n, dtype=np.uint64) * np.uint64(WINDOW)
        hd["len"] = np.minimum(hd["len"], WINDOW)   # (every frame here has at least 16 bytes)
        hu2, hv = macswap.macswap_host(hu, hd, 0, num_interfaces=2)
        host_ms, d2h_ms = (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3
        # one more device swap, checked against the host's on every frame
        swap()
        torch.cuda.synchronize()
        same = bool(np.array_equal(v.cpu().numpy(), hv) and
                    np.array_equal(rows[:, H:H + WINDOW].contiguous().cpu().numpy().reshape(-1), hu2))
        ok = ok and same and same_start and int(lens.min()) >= WINDOW
        bound_us = n * FRAME_BYTES / (HBM_TBS * 1e12) * 1e6
        med = {}
        for k in calls:
            ev[k].sort()
            med[k] = ev[k][len(ev[k]) // 2]
        for k in calls:
            row = {"batch": name, "frames": n, "call": k, "reps": a.reps, "event_us_median": med[k],
                   "event_us_min": ev[k][0], "event_us_max": ev[k][-1], "us_per_1m_frames": med[k] / n * 1e6,
                   "over_read_probe": med[k] / n * 1e6 / PROBE_US_PER_M, "frames_equal_host": same,
                   "frames_restored": same_start}
            if k == "swap":
                row.update({"bytes": n * FRAME_BYTES, "bound_us": bound_us, "median_over_bound": med[k] / bound_us,
                            "swap_minus_firewall_us": med["swap"] - med["firewall"],
                            "swap_minus_firewall_us_per_1m": (med["swap"] - med["firewall"]) / n * 1e6,
                            "host_way_ms": host_ms, "host_d2h_ms": d2h_ms})
            lines.append(row)
            print(json.dumps(row), flush=True)
        del umem, dd, v, rows
        torch.cuda.empty_cache()
    acl.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
