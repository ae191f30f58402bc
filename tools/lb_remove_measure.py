#!/usr/bin/env python3
"""Removing sessions from the load balancer's device table.

The default object: 2,000,000 sessions in 4,194,304 slots, 16 backends of one
service, filled by a batch of 1,000,000 new flows (two sessions per flow).  Per
row the table is rebuilt outside the timed region, then ONE call is timed two
ways:
  event_us  HIP events on the stream around the call: what the device pays (the
            key list's copy, the removal launch, the four compaction launches);
  call_us   wall clock around the C call: what the caller pays (the copy into
            the pinned buffer and the enqueueing; the host waits for nothing).
Rows:
  remove   1, 1,000 and 100,000 keys, with and without REMOVE_PAIR, from the full
           table with no tombstones (no compaction in the call) and from the same
           table with slots / 4 tombstones (the call crosses the bound and
           compacts the 2,000,000 live sessions less what it removes);
  drain    one backend of 16, likewise;
  clear    xsknf_gpu_lb_sessions_clear of the device table;
  hits     an lb_batch of 1,000,000 hits, one per flow, on the 2,000,000 live
           sessions with no tombstones, and on the same sessions stored into a
           table that held 1,000,000 tombstones (just under the bound of
           1,048,576): what the batch kernels' probes pay for walking over them.
--baseline times the only way there was before these calls, on the same table:
dump, filter on the host, destroy, create, sessions_put the survivors (wall
clock).  --package-root names the tree whose xsknf_amd package and library run
(default: this one), so that a build of the parent commit can run the baseline.
Median, min and max of --reps after --warmup; one JSON line per row, to stdout
and to --out (appended to with --baseline).

  python tools/lb_remove_measure.py [--reps 10] [--warmup 2] [--baseline] [--package-root DIR] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

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


def flow_keys(count, sport):
    from xsknf_amd import lb

    k = np.zeros(count, dtype=lb.KEY_DTYPE)
    k["saddr"] = np.arange(count, dtype=np.uint32) + np.uint32(1)
    k["daddr"], k["sport"], k["dport"], k["proto"] = VADDR, sport, VPORT, 17
    return k


def spread(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))

    import torch
    from xsknf_amd import _lib, lb

    if not torch.cuda.is_available():
        sys.exit("lb_remove_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    bk = np.zeros(16, dtype=lb.BACKEND_DTYPE)
    bk["vaddr"], bk["vport"], bk["proto"] = VADDR, VPORT, 17
    bk["addr"] = 0xc0a80001 + np.arange(16)
    bk["port"], bk["ifindex"] = 0x901f, np.arange(16) % 4
    umem, descs = flow_frames(FLOWS, 0x1234)
    keys = flow_keys(FLOWS, 0x1234)
    du0 = torch.from_numpy(umem).to(dev)
    du = du0.clone()
    dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    dv = torch.empty(FLOWS, dtype=torch.int32, device=dev)
    ws = torch.empty(lb.lb_workspace(FLOWS), dtype=torch.uint8, device=dev)
    st = torch.zeros(8, dtype=torch.int64, device=dev)
    lines = []

    def row(name, extra):
        lines.append({"row": name, **extra})
        print(json.dumps(lines[-1]), flush=True)

    def run(L, count, src=None):
        """A batch of the first `count` frames of `src` (default: the 1,000,000 flows), from a restored UMEM."""
        du.copy_(du0 if src is None else src)
        lb.lb_batch_ptr(du.data_ptr(), du.numel(), dd.data_ptr(), count, 0, 4, L, dv.data_ptr(), ws.data_ptr(),
                        ws.numel(), st.data_ptr(), stream.cuda_stream)

    if a.baseline:
        bk3 = int(bk[3]["addr"])

        def listed(m):
            want = keys["saddr"][:m]
            return lambda k, v: (np.isin(k["saddr"], want) & (v["dir"] == 1)) | (np.isin(k["daddr"], want) & (v["dir"] == 0))
        picks = {"remove 1 key, pair": listed(1), "remove 1000 keys, pair": listed(1000),
                 "remove 100000 keys, pair": listed(100000),
                 "drain 1 backend of 16": lambda k, v: ((v["dir"] == 1) & (v["addr"] == bk3)) | ((v["dir"] == 0) & (k["saddr"] == bk3)),
                 "clear": lambda k, v: np.ones(k.shape[0], dtype=bool)}
        k = np.zeros(2 * FLOWS, dtype=lb.KEY_DTYPE)
        v = np.zeros(2 * FLOWS, dtype=lb.VALUE_DTYPE)
        for name, pick in picks.items():
            t, removed = [], 0
            for _ in range(max(2, a.reps // 4)):
                L = lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS)
                run(L, FLOWS)
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                n = ctypes.c_uint32(0)
                _lib.check(lib.xsknf_gpu_lb_sessions_dump(L.handle, lb.DEVICE_TABLE, k.ctypes.data, v.ctypes.data, k.size,
                                                          ctypes.byref(n)), "dump")
                keep = ~pick(k[:n.value], v[:n.value])
                L.close()
                L = lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS)
                L.sessions_put(k[:n.value][keep], v[:n.value][keep])
                torch.cuda.synchronize()
                t.append((time.perf_counter() - w0) * 1e6)
                removed = int(keep.size - keep.sum())
                assert L.info["device_sessions"] == n.value - removed
                L.close()
            row("baseline (dump, filter, destroy, create, put): " + name,
                {"wall_us": spread(t), "removed": removed, "reps": len(t), "library": _lib.LIB_PATH})
    else:
        umem_b, _ = flow_frames(HALF, 0x4321)   # 500,000 other flows: the sessions that become tombstones
        keys_b = flow_keys(HALF, 0x4321)
        db0 = torch.zeros_like(du0)
        db0[:umem_b.size] = torch.from_numpy(umem_b).to(dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        with lb.LoadBalancer.from_backends(bk, max_sessions=2 * FLOWS) as L:
            assert L.info["slots"] == 1 << 22
            h = L.handle
            s = ctypes.c_void_p(stream.cuda_stream or None)

            def clear():
                _lib.check(lib.xsknf_gpu_lb_sessions_clear(h, lb.DEVICE_TABLE, s), "clear")

            def remove(k, flags):
                _lib.check(lib.xsknf_gpu_lb_sessions_remove(h, k.ctypes.data, k.shape[0], flags, res.data_ptr(), s), "remove")

            def full(tombstones):
                """2,000,000 sessions; with `tombstones`, in a table that holds slots / 4 of them."""
                clear()
                if tombstones:   # 524,288 flows stored and removed, then stored again with the rest
                    run(L, 1 << 19)
                    remove(keys[:1 << 19], 1)
                run(L, FLOWS)

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

            full(False)
            assert L.info["device_sessions"] == 2 * FLOWS and int(st[6]) == 0, "the fill left the parallel path"
            for tombs in (False, True):
                for m in (1, 1000, 100000):
                    for pair in (0, 1):
                        # the keys from the list's far end: never among the flows behind the tombstones
                        k = np.ascontiguousarray(keys[FLOWS - m:])
                        t = timed(lambda: full(tombs), lambda: remove(k, pair))
                        ok = t["result"] == [m * (1 + pair), int(tombs)]
                        row(f"remove {m} keys{', pair' if pair else ''}{', compacting' if tombs else ''}",
                            {**t, "as_expected": ok, "sessions_after": L.info["device_sessions"]})
            for tombs in (False, True):
                t = timed(lambda: full(tombs), lambda: _lib.check(lib.xsknf_gpu_lb_drain_backend(
                    h, int(bk[3]["addr"]), int(bk[3]["port"]), 17, res.data_ptr(), s), "drain"))
                row(f"drain 1 backend of 16{', compacting' if tombs else ''}", {**t, "sessions_after": L.info["device_sessions"]})
            t = timed(lambda: full(False), clear)
            row("clear", {"event_us": t["event_us"], "call_us": t["call_us"], "reps": a.reps,
                          "sessions_after": L.info["device_sessions"]})

            # the batch kernels' probes over tombstones
            restore = timed(lambda: None, lambda: du.copy_(du0))["event_us"]
            for tombs in (False, True):
                clear()
                r = None
                if tombs:
                    run(L, HALF, db0)
                    remove(keys_b, 1)
                    torch.cuda.synchronize()
                    r = res.cpu().numpy().tolist()
                run(L, FLOWS)                       # stored after the tombstones: every probe walks over them
                t = timed(lambda: None, lambda: run(L, FLOWS))
                s8 = st.cpu().numpy().tolist()
                row(f"batch of {FLOWS} hits, {2 * FLOWS} live sessions, {2 * HALF if tombs else 0} tombstones",
                    {"event_us": t["event_us"], "minus_restore_us": t["event_us"]["median"] - restore["median"],
                     "restore_us": restore, "stats": s8, "all_hits": s8[1] == FLOWS and s8[4] == 0,
                     "tombstones_from": r, "sessions": L.info["device_sessions"], "reps": a.reps})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.baseline else "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
