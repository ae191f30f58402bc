#!/usr/bin/env python3
"""Ageing of the load balancer's device table.

The object of tools/lb_remove_measure.py: 2,000,000 sessions in 4,194,304 slots,
16 backends of one service, filled by a batch of 1,000,000 new flows.  Per row
the table is rebuilt outside the timed region, then ONE call is timed two ways:
  event_us  HIP events on the stream around the call: what the device pays;
  call_us   wall clock around the C call: what the caller pays (the host waits
            for nothing).
Rows:
  expire   nothing idle; half idle (500,000 flows had forward traffic since, so
           1,500,000 slots are idle and probe for their partner and 1,000,000
           sessions leave, one short of the rebuild's bound); all idle (2,000,000
           leave, and the call rebuilds the then empty table);
  drain    xsknf_gpu_lb_drain_backend of one backend of 16 over the same table,
           in the same process: the one-pass removal expire is compared with;
  clock    xsknf_gpu_lb_clock alone;
  batch    1,000,000 hits and 1,000,000 new flows, on an object without ageing
           and on one with it, interleaved rep by rep.
--no-ageing-only runs the two batch rows on an object without ageing and calls
nothing the parent commit lacks; with --package-root naming a built tree of the
parent commit (its xsknf_amd package and library run, as for
tools/lb_remove_measure.py) it gives the parent's figure and its run-to-run
spread for the comparison "a batch without ageing against the parent".
Median, min and max of --reps after --warmup; one JSON line per row, to stdout
and appended to --out.

  python tools/lb_age_measure.py [--reps 10] [--warmup 2] [--no-ageing-only] [--package-root DIR] [--tag NAME] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOWS = 1_000_000   # two sessions each: XSKNF_GPU_LB_MAX_SESSIONS
HALF = 500_000
VADDR, VPORT = 0x0a000001, 0x5000


def flow_frames(count, sport):
    """One 64-byte UDP frame (ihl 5) per flow: source address 1 .. count, one source port."""
    from xsknf_amd import frames

    fr = np.random.default_rng(4411).integers(0, 256, (count, 64), dtype=np.uint8)
    fr[:, 12], fr[:, 13], fr[:, 14], fr[:, 23] = 8, 0, 0x45, 17
    fr[:, 26:30] = (np.arange(count, dtype="<u4") + np.uint32(1)).view(np.uint8).reshape(count, 4)
    fr[:, 30:34] = np.full(count, VADDR, dtype="<u4").view(np.uint8).reshape(count, 4)
    fr[:, 34:36] = np.full(count, sport, dtype="<u2").view(np.uint8).reshape(count, 2)
    fr[:, 36:38] = np.full(count, VPORT, dtype="<u2").view(np.uint8).reshape(count, 2)
    d = np.zeros(count, dtype=frames.DESC_DTYPE)
    d["addr"] = np.arange(count, dtype=np.uint64) * 64
    d["len"] = 64
    return fr.reshape(-1), d


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-ageing-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))

    import torch
    from xsknf_amd import _lib, lb

    if not torch.cuda.is_available():
        sys.exit("lb_age_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    s = ctypes.c_void_p(stream.cuda_stream or None)
    bk = np.zeros(16, dtype=lb.BACKEND_DTYPE)
    bk["vaddr"], bk["vport"], bk["proto"] = VADDR, VPORT, 17
    bk["addr"] = 0xc0a80001 + np.arange(16)
    bk["port"], bk["ifindex"] = 0x901f, np.arange(16) % 4
    umem, descs = flow_frames(FLOWS, 0x1234)
    du0 = torch.from_numpy(umem).to(dev)
    du = du0.clone()
    dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    dv = torch.empty(FLOWS, dtype=torch.int32, device=dev)
    ws = torch.empty(lb.lb_workspace(FLOWS), dtype=torch.uint8, device=dev)
    st = torch.zeros(8, dtype=torch.int64, device=dev)
    res = torch.zeros(2, dtype=torch.int64, device=dev)
    lines = []

    def row(name, extra):
        lines.append({"row": name, "tag": a.tag, "library": os.path.relpath(_lib.LIB_PATH, os.path.abspath(a.package_root)), **extra})
        print(json.dumps(lines[-1]), flush=True)

    def run(L, count):
        """A batch of the first `count` flows' frames, from a restored UMEM."""
        du.copy_(du0)
        lb.lb_batch_ptr(du.data_ptr(), du.numel(), dd.data_ptr(), count, 0, 4, L, dv.data_ptr(), ws.data_ptr(),
                        ws.numel(), st.data_ptr(), stream.cuda_stream)

    def batch_only(L, count):
        lb.lb_batch_ptr(du.data_ptr(), du.numel(), dd.data_ptr(), count, 0, 4, L, dv.data_ptr(), ws.data_ptr(),
                        ws.numel(), st.data_ptr(), stream.cuda_stream)

    def clear(L):
        _lib.check(lib.xsknf_gpu_lb_sessions_clear(L.handle, lb.DEVICE_TABLE, s), "clear")

    def timed(prepare, call, read=None):
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
            out = read().cpu().numpy().tolist() if read is not None else None
        return {"event_us": spread(ev), "call_us": spread(wall), "result": out, "reps": a.reps}

    def batches(objects):
        """{name: L}: 1,000,000 hits and 1,000,000 new flows on each, the objects taking turns rep by rep."""
        for kind in ("hits", "new flows"):
            ev = {name: [] for name in objects}
            stats = {}
            for i in range(a.warmup + a.reps):
                for name, L in objects.items():
                    clear(L)
                    if kind == "hits":
                        run(L, FLOWS)
                    du.copy_(du0)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    batch_only(L, FLOWS)
                    e1.record(stream)
                    e1.synchronize()
                    if i >= a.warmup:
                        ev[name].append(e0.elapsed_time(e1) * 1e3)
                    stats[name] = st.cpu().numpy().tolist()
            for name in objects:
                s8 = stats[name]
                ok = (s8[1] == FLOWS and s8[6] == 0 and s8[4] == (0 if kind == "hits" else 2 * FLOWS))
                row(f"batch of {FLOWS} {kind}, {name}", {"event_us": spread(ev[name]), "stats": s8, "as_expected": ok,
                                                        "reps": a.reps})

    with lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS) as off:
        assert off.info["slots"] == 1 << 22
        if a.no_ageing_only:
            batches({"no ageing": off})
        else:
            with lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS) as on:
                on.aging_enable()
                h = on.handle

                def clock(now):
                    _lib.check(lib.xsknf_gpu_lb_clock(h, lb.DEVICE_TABLE, now, s), "clock")

                def expire(max_idle):
                    _lib.check(lib.xsknf_gpu_lb_sessions_expire(h, max_idle, res.data_ptr(), s), "expire")

                def full(hits):
                    """2,000,000 sessions stamped 0; the first `hits` flows' forward halves stamped 10; the clock at 20."""
                    clear(on)
                    clock(0)
                    run(on, FLOWS)
                    clock(10)
                    if hits:
                        run(on, hits)
                    clock(20)

                full(0)
                assert on.info["device_sessions"] == 2 * FLOWS and int(st[6]) == 0, "the fill left the parallel path"
                for name, hits, max_idle, want in (("nothing idle", 0, 20, [0, 0]), ("half idle", HALF, 15, [2 * HALF, 0]),
                                                   ("all idle", 0, 15, [2 * FLOWS, 1])):
                    t = timed(lambda: full(hits), lambda: expire(max_idle), lambda: res)
                    row(f"expire, {name}", {**t, "as_expected": t["result"] == want,
                                            "sessions_after": on.info["device_sessions"]})
                t = timed(lambda: full(0), lambda: _lib.check(lib.xsknf_gpu_lb_drain_backend(
                    h, int(bk[3]["addr"]), int(bk[3]["port"]), 17, res.data_ptr(), s), "drain"), lambda: res)
                row("drain 1 backend of 16 (ageing on: the same table)", {**t, "sessions_after": on.info["device_sessions"]})
                t = timed(lambda: None, lambda: clock(33))
                row("clock", {"event_us": t["event_us"], "call_us": t["call_us"], "reps": a.reps})
                batches({"no ageing": off, "ageing on": on})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
