#!/usr/bin/env python3
"""The root distribution's planning, host against device.

Config 4's shape -- `frames` IMIX frames, one per 2 KiB chunk -- with the UMEM
and the descriptors resident on device 0 at the start, packed mode, over every
visible device:

  host: the caller's wall time around the descriptors' copy to the host plus
        xsknf_gpu_multi_scatter_packed (which plans on one CPU thread and stages
        two copies of the descriptors), next to the `seconds` that call reports;
  dev:  xsknf_gpu_multi_scatter_dev's `seconds` / `plan_seconds`, next to the
        caller's wall time around it.

Both leave the same shards (checked: every shard's info and descriptors).  The
UMEM's bytes are zeros: no time here depends on them.  One JSON line per
repetition and a summary line, to stdout and to --out.

  python tools/plan_dev_measure.py [--frames 8388608] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0   # MI355X HBM3E peak, TB/s: the planner's bound is its bytes over this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import frames, multi

    n = a.frames
    dev = torch.device("cuda:0")
    ndev = torch.cuda.device_count()
    rng = np.random.default_rng(frames.SEED)
    hd = np.zeros(n, dtype=frames.DESC_DTYPE)
    hd["addr"] = np.arange(n, dtype=np.uint64) * np.uint64(frames.CHUNK) + np.uint64(frames.HEADROOM)
    hd["len"] = frames.imix_lengths(n, rng)
    size = n * frames.CHUNK
    umem = torch.zeros(size, dtype=torch.uint8, device=dev)
    dd = torch.from_numpy(hd.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    torch.cuda.synchronize()
    lines = []

    def shards(m):
        out = []
        for k in range(ndev):
            info = m.shard_info(k)
            _, _, sd = m.fetch(k, descs=True)
            out.append(([info[x] for x in ("frame_lo", "frame_hi", "span_lo", "span_hi", "frame_bytes", "flags")], sd))
        return out

    with multi.MultiDevice(range(ndev)) as m:
        # once each untimed: the root and shard buffers are allocated on first use
        m.scatter_packed(0, umem.data_ptr(), size, hd)
        want = shards(m)
        m.scatter_dev(0, umem.data_ptr(), size, dd.data_ptr(), n, packed=True)
        got = shards(m)
        same = all(w[0] == g[0] and np.array_equal(w[1], g[1]) for w, g in zip(want, got))
        for rep in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            back = dd.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)
            t1 = time.perf_counter()
            secs = m.scatter_packed(0, umem.data_ptr(), size, back)
            t2 = time.perf_counter()
            dsecs, dplan = m.scatter_dev(0, umem.data_ptr(), size, dd.data_ptr(), n, packed=True)
            t3 = time.perf_counter()
            lines.append({"rep": rep, "host_wall_ms": (t2 - t0) * 1e3, "host_descs_d2h_ms": (t1 - t0) * 1e3,
                          "host_reported_ms": secs * 1e3, "dev_wall_ms": (t3 - t2) * 1e3, "dev_seconds_ms": dsecs * 1e3,
                          "dev_plan_ms": dplan * 1e3})
    # the packed plan reads the descriptors twice and writes one set: 48 B per frame
    bound_us = 48.0 * n / (HBM_TBS * 1e12) * 1e6
    best = min(lines, key=lambda r: r["dev_seconds_ms"])
    summary = {"frames": n, "devices": ndev, "mode": "packed", "shards_equal": bool(same),
               "host_wall_ms_min": min(r["host_wall_ms"] for r in lines),
               "host_reported_ms_min": min(r["host_reported_ms"] for r in lines),
               "dev_seconds_ms_min": best["dev_seconds_ms"],
               "dev_plan_ms_min": min(r["dev_plan_ms"] for r in lines),
               "plan_bound_us": bound_us,
               "plan_over_bound": min(r["dev_plan_ms"] for r in lines) * 1e3 / bound_us if n else None}
    text = "\n".join(json.dumps(r) for r in lines + [summary])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
