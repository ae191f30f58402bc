#!/usr/bin/env python3
"""The firewall's device lookup against its bounds and the host way.

Three batches resident on device 0, one frame per 2 KiB chunk, their frames
rewritten to IPv4 TCP / UDP (ihl 5) with random 5-tuples:
  config2   1,048,576 frames of 64 B;
  config3   1,048,576 frames of 1500 B;
  config4   8,388,608 IMIX frames;
each against ACLs of 1, 1,000 and 1,000,000 random rules, at hit shares 0 and 1/2
(half of the frames carry the key of a rule drawn at random).

  dev:  xsknf_gpu_firewall_batch, enqueued only, on HIP events around each call,
        after --warmup calls, --reps times: median, min and max;
  host: the caller's wall time around a gather of every frame's first 96 bytes on
        the device, their copy and the descriptors' to the host, and
        xsknf_gpu_firewall_host on one thread (once per row).

Both give the same verdicts (checked, every frame).  The bound is the least
bytes the lookup moves -- 16 B descriptor, one 64 B sector of headers, one 16 B
key slot, 4 B verdict, 4 B of action per hit -- over the HBM peak.  The two
yardsticks are this project's own measurements of the same access pattern
(DESIGN 3): the 64 B read probe at a 2 KiB stride, 28 us per 1M sectors, and the
lane kernel's NIC-offload step, 33.5 us per 1M frames (the same sector read plus
a verdict store).  One JSON line per row, to stdout and to --out.

  python tools/firewall_measure.py [--reps 20] [--warmup 3] [--scale 1] [--out FILE]
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
NIC_US_PER_M = 33.5      # lane kernel, NIC-offload step
WINDOW = 96              # bytes of a frame the host way brings home (14 + 60 + 20 at most are read)


def random_rules(rng, n):
    from xsknf_amd import firewall

    r = np.zeros(n, dtype=firewall.RULE_DTYPE)
    raw = r.view(np.uint8).reshape(-1, 20)
    raw[:, :12] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    r["proto"] = np.where(rng.integers(0, 2, n) == 1, 6, 17)
    r["action"] = rng.integers(-1, 3, n)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the frame and rule counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import firewall, frames

    if not torch.cuda.is_available():
        sys.exit("firewall_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(frames.SEED + 14)
    acls = []
    for nr0 in (1, 1000, 1000000):
        nr = max(1, int(nr0 * a.scale)) if nr0 > 1 else 1
        rules = random_rules(rng, nr)
        t0 = time.perf_counter()
        acl = firewall.Acl.from_rules(rules)
        acls.append((rules, acl, (time.perf_counter() - t0) * 1e3))
    lines, ok = [], True
    H = frames.HEADROOM
    for name, n0, length in (("config2", 1 << 20, 64), ("config3", 1 << 20, 1500), ("config4", 8 << 20, "imix")):
        n = max(1, int(n0 * a.scale))
        umem, dd, lens = frames.device_batch(n, length, device=dev)
        rows = umem.view(n, frames.CHUNK)
        rows[:, H + 12], rows[:, H + 13], rows[:, H + 14] = 8, 0, 0x45
        v = torch.empty(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        for rules, acl, build_ms in acls:
            for share in (0.0, 0.5):
                # the tuples: random, and for `share` of the frames a rule's
                key = np.empty((n, 13), dtype=np.uint8)
                key[:, :12] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
                key[:, 12] = np.where(rng.integers(0, 2, n) == 1, 6, 17)
                hit = np.flatnonzero(rng.random(n) < share)
                key[hit] = rules.view(np.uint8).reshape(-1, 20)[rng.integers(0, rules.shape[0], hit.size), :13]
                k = torch.from_numpy(key).to(dev)
                rows[:, H + 23] = k[:, 12]
                rows[:, H + 26:H + 38] = k[:, :12]
                del k
                torch.cuda.synchronize()

                def call():
                    firewall.firewall_batch_ptr(umem.data_ptr(), umem.numel(), dd.data_ptr(), n, acl, v.data_ptr(),
                                                stream.cuda_stream)

                for _ in range(a.warmup):
                    call()
                torch.cuda.synchronize()
                ev = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    e1.synchronize()
                    ev.append(e0.elapsed_time(e1) * 1e3)
                ev.sort()
                # the host way: header bytes and descriptors home, then one thread
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w = min(WINDOW, int(lens.min()))
                hu = rows[:, H:H + w].contiguous().cpu().numpy().reshape(-1)
                hd = dd.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1).copy()
                t1 = time.perf_counter()
                hd["addr"] = np.arange(n, dtype=np.uint64) * np.uint64(w)
                hd["len"] = np.minimum(hd["len"], w)   # (nothing past 94 bytes is looked at)
                hv = firewall.firewall_host(hu, hd, acl)
                host_ms, d2h_ms = (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3
                same = bool(np.array_equal(v.cpu().numpy(), hv))
                ok = ok and same
                hits = int(hit.size)
                nbytes = n * (16 + 64 + 16 + 4) + 4 * hits
                bound_us = nbytes / (HBM_TBS * 1e12) * 1e6
                med = ev[len(ev) // 2]
                i = acl.info
                lines.append({"batch": name, "frames": n, "rules": i["rules"], "slots": i["slots"],
                              "max_probe": i["max_probe"], "table_bytes": i["device_bytes"],
                              "acl_build_ms": build_ms, "hit_share": share, "hit_frames": hits,
                              "nonzero_verdicts": int(np.count_nonzero(hv)), "verdicts_equal_host": same,
                              "reps": a.reps, "event_us_median": med, "event_us_min": ev[0], "event_us_max": ev[-1],
                              "bytes": nbytes, "bound_us": bound_us, "median_over_bound": med / bound_us,
                              "us_per_1m_frames": med / n * 1e6,
                              "over_read_probe": med / n * 1e6 / PROBE_US_PER_M,
                              "over_nic_offload_step": med / n * 1e6 / NIC_US_PER_M,
                              "host_way_ms": host_ms, "host_d2h_ms": d2h_ms})
                print(json.dumps(lines[-1]), flush=True)
        del umem, dd, v, rows
        torch.cuda.empty_cache()
    for _, acl, _ in acls:
        acl.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
