#!/usr/bin/env python3
"""Updating a live load balancer's backends and draining a list of them.

The object: 2,000,000 sessions in 4,194,304 slots, one service of 8,192
backends, filled by a batch of 1,000,000 new flows (two sessions per flow, about
244 per backend).  For every list size n in 1, 16, 256, 4096:
  update   ONE xsknf_gpu_lb_backends_update of n REMOVE ops, of the service's
           first n backends, so that every later one moves (the creation order
           is restored outside the timed region);
  drain    ONE xsknf_gpu_lb_drain_backends of those n backends;
  single   n calls of xsknf_gpu_lb_drain_backend, one per backend, on an equal
           table (refilled outside the timed region).
Half the backends hold half the sessions, 1,000,000 tombstones, just under the
bound of slots / 4 = 1,048,576: no call compacts, so every row streams the table
and nothing else.  Each is timed two ways:
  event_us  HIP events on the stream around the call(s): what the device pays;
  call_us   wall clock around the C call(s): what the caller pays (the host
            waits for nothing).
Median, min and max of --reps after --warmup; one JSON line per row, to stdout
and to --out.

  python tools/lb_backends_measure.py [--reps 10] [--warmup 2] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

FLOWS = 1_000_000
BACKENDS = 8192
VADDR, VPORT = 0x0a000001, 0x5000
SIZES = (1, 16, 256, 4096)


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch
    from xsknf_amd import _lib, frames, lb

    if not torch.cuda.is_available():
        sys.exit("lb_backends_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    s = ctypes.c_void_p(stream.cuda_stream or None)
    bk = np.zeros(BACKENDS, dtype=lb.BACKEND_DTYPE)
    bk["vaddr"], bk["vport"], bk["proto"] = VADDR, VPORT, 17
    bk["addr"] = 0xc0a80001 + np.arange(BACKENDS)
    bk["port"], bk["ifindex"] = 0x901f, np.arange(BACKENDS) % 4
    fr = np.random.default_rng(4421).integers(0, 256, (FLOWS, 64), dtype=np.uint8)
    fr[:, 12], fr[:, 13], fr[:, 14], fr[:, 23] = 8, 0, 0x45, 17
    fr[:, 26:30] = (np.arange(FLOWS, dtype="<u4") + np.uint32(1)).view(np.uint8).reshape(FLOWS, 4)
    fr[:, 30:34] = np.full(FLOWS, VADDR, dtype="<u4").view(np.uint8).reshape(FLOWS, 4)
    fr[:, 34:36] = np.full(FLOWS, 0x1234, dtype="<u2").view(np.uint8).reshape(FLOWS, 2)
    fr[:, 36:38] = np.full(FLOWS, VPORT, dtype="<u2").view(np.uint8).reshape(FLOWS, 2)
    descs = np.zeros(FLOWS, dtype=frames.DESC_DTYPE)
    descs["addr"] = np.arange(FLOWS, dtype=np.uint64) * 64
    descs["len"] = 64
    du0 = torch.from_numpy(fr.reshape(-1)).to(dev)
    du = du0.clone()
    dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    dv = torch.empty(FLOWS, dtype=torch.int32, device=dev)
    ws = torch.empty(lb.lb_workspace(FLOWS), dtype=torch.uint8, device=dev)
    st = torch.zeros(8, dtype=torch.int64, device=dev)
    res = torch.zeros(2, dtype=torch.int64, device=dev)
    lines = []

    def row(name, extra):
        lines.append({"row": name, **extra})
        print(json.dumps(lines[-1]), flush=True)

    with lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS) as L:
        assert L.info["slots"] == 1 << 22
        h = L.handle

        def fill():
            _lib.check(lib.xsknf_gpu_lb_sessions_clear(h, lb.DEVICE_TABLE, s), "clear")
            du.copy_(du0)
            lb.lb_batch_ptr(du.data_ptr(), du.numel(), dd.data_ptr(), FLOWS, 0, 4, L, dv.data_ptr(), ws.data_ptr(),
                            ws.numel(), st.data_ptr(), stream.cuda_stream)

        def timed(prepare, call):
            ev, wall, out = [], [], None
            for i in range(a.warmup + a.reps):
                prepare()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                w0 = time.perf_counter()
                call()
                w1 = time.perf_counter()
                e1.record(stream)
                e1.synchronize()
                if i >= a.warmup:
                    ev.append(e0.elapsed_time(e1) * 1e3)
                    wall.append((w1 - w0) * 1e6)
                out = res.cpu().numpy().tolist()
            return {"event_us": spread(ev), "call_us": spread(wall), "result": out, "reps": a.reps}

        fill()
        torch.cuda.synchronize()
        assert L.info["device_sessions"] == 2 * FLOWS and int(st[6]) == 0, "the fill left the parallel path"
        for n in SIZES:
            gone = np.ascontiguousarray(bk[:n])   # the first n: every later backend moves down
            rm = np.zeros(n, dtype=lb.BACKEND_OP_DTYPE)
            rm["backend"], rm["op"] = gone, lb.BACKEND_REMOVE
            ad = np.zeros(2 * BACKENDS, dtype=lb.BACKEND_OP_DTYPE)   # every backend out, then in again in creation's order
            ad["backend"][:BACKENDS], ad["backend"][BACKENDS:] = bk, bk
            ad["op"][:BACKENDS] = lb.BACKEND_REMOVE
            ids = np.zeros(n, dtype=lb.BACKEND_ID_DTYPE)
            ids["addr"], ids["port"], ids["proto"] = gone["addr"], gone["port"], 17

            def restore():
                _lib.check(lib.xsknf_gpu_lb_backends_update(h, ad.ctypes.data, ad.size, s), "restore")

            t = timed(restore, lambda: _lib.check(lib.xsknf_gpu_lb_backends_update(h, rm.ctypes.data, n, s), "remove"))
            restore()
            row(f"update, {n} REMOVE ops of {BACKENDS} backends", {"event_us": t["event_us"], "call_us": t["call_us"],
                                                                   "reps": a.reps, "backends_after": L.info["backends"]})
            t = timed(fill, lambda: _lib.check(lib.xsknf_gpu_lb_drain_backends(h, ids.ctypes.data, n, res.data_ptr(), s),
                                               "drain_backends"))
            after = L.info["device_sessions"]
            row(f"drain_backends, a list of {n}", {**t, "sessions_after": after})

            def singles():
                for r in ids:
                    _lib.check(lib.xsknf_gpu_lb_drain_backend(h, int(r["addr"]), int(r["port"]), 17, res.data_ptr(), s),
                               "drain_backend")

            t = timed(fill, singles)
            row(f"drain_backend, {n} calls", {"event_us": t["event_us"], "call_us": t["call_us"], "reps": a.reps,
                                              "sessions_after": L.info["device_sessions"],
                                              "same_table_as_the_list_drain": L.info["device_sessions"] == after})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
