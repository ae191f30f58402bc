#!/usr/bin/env python3
"""The load balancer's device batch against the host loop and the firewall.

1,048,576 frames of 64 B (ihl 5, UDP), one per 64-byte slot, resident on device 0:
  a  hits      every frame's session was put before the batch (forward direction);
  b  new       each of the first 1,000,000 frames is the only frame of a new flow
               towards one of 16 services with 8 backends each: 2,000,000 sessions
               stored, the table's cap (a fresh object per call);
  c  host      xsknf_gpu_lb_host on the same inputs as a and b, one thread, wall time;
  d  firewall  xsknf_gpu_firewall_batch over the same frames with a 1,000-rule ACL:
               the same parse and one read-only lookup;
  e  ordered   a batch of --ordered-frames new flows into a table too small for
               them: the whole batch on the one-lane path.
a, b, d, e: HIP events around the enqueueing call, after --warmup calls, --reps
times: median, min and max (b and e rebuild their object per call, outside the
events).  a and b are checked against the host call's UMEM and verdicts.  One
JSON line per row, to stdout and to --out.

  python tools/lb_measure.py [--reps 10] [--warmup 2] [--frames 1048576] [--ordered-frames 16384] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch(rng, n, vaddr, vport):
    """n frames towards services (vaddr[i], vport[i]) drawn at random, distinct clients."""
    from xsknf_amd import frames

    fr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    fr[:, 12], fr[:, 13], fr[:, 14], fr[:, 23] = 8, 0, 0x45, 17
    s = rng.integers(0, len(vaddr), n)
    fr[:, 26:30] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)   # distinct source addresses
    fr[:, 30:34] = np.asarray(vaddr, dtype="<u4")[s].view(np.uint8).reshape(n, 4)
    fr[:, 36:38] = np.asarray(vport, dtype="<u2")[s].view(np.uint8).reshape(n, 2)
    d = np.zeros(n, dtype=frames.DESC_DTYPE)
    d["addr"] = np.arange(n, dtype=np.uint64) * 64
    d["len"] = 64
    return fr.reshape(-1), d


def timed(torch, stream, reps, warmup, call, prepare=None):
    ev = []
    for i in range(warmup + reps):
        ctx = prepare() if prepare else None
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call(ctx)
        e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            ev.append(e0.elapsed_time(e1) * 1e3)
        if ctx is not None and hasattr(ctx, "close"):
            ctx.close()
    ev.sort()
    return {"event_us_median": ev[len(ev) // 2], "event_us_min": ev[0], "event_us_max": ev[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--ordered-frames", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import firewall, lb

    if not torch.cuda.is_available():
        sys.exit("lb_measure: no GPU (there is no CPU fallback for a measurement)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(4404)
    n = a.frames
    nsvc, per = 16, 8
    bk = np.zeros(nsvc * per, dtype=lb.BACKEND_DTYPE)
    bk["vaddr"] = np.repeat(0x0a000001 + np.arange(nsvc), per)
    bk["vport"] = np.repeat(0x5000 + np.arange(nsvc), per)
    bk["proto"] = 17
    bk["addr"] = 0xc0a80001 + np.arange(nsvc * per)
    bk["port"] = 0x901f
    bk["mac"] = rng.integers(0, 256, (nsvc * per, 6))
    bk["ifindex"] = np.arange(nsvc * per) % 4
    vaddr, vport = bk["vaddr"][::per], bk["vport"][::per]
    umem, descs = batch(rng, n, vaddr, vport)
    stream = torch.cuda.current_stream(dev)
    du0 = torch.from_numpy(umem).to(dev)
    du = du0.clone()
    dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    dv = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(lb.lb_workspace(n), dtype=torch.uint8, device=dev)
    st = torch.zeros(8, dtype=torch.int64, device=dev)
    lines, ok = [], True

    def run(L, m=n):
        lb.lb_batch_ptr(du.data_ptr(), 64 * m, dd.data_ptr(), m, 0, 4, L, dv.data_ptr(), ws.data_ptr(), ws.numel(),
                        st.data_ptr(), stream.cuda_stream)

    def row(name, extra):
        lines.append({"row": name, "frames": n, **extra})
        print(json.dumps(lines[-1]), flush=True)

    # a: all pre-populated hits
    keys = np.zeros(n, dtype=lb.KEY_DTYPE)
    raw = umem.reshape(n, 64)
    keys.view(np.uint8).reshape(n, 16)[:, 0:8] = raw[:, 26:34]
    keys.view(np.uint8).reshape(n, 16)[:, 8:12] = raw[:, 34:38]
    keys["proto"] = 17
    vals = np.zeros(n, dtype=lb.VALUE_DTYPE)
    vals["addr"], vals["port"], vals["ifindex"], vals["dir"] = 0xc0a80001, 0x901f, 1, lb.TO_BACKEND
    with lb.LoadBalancer.from_backends(bk, max_sessions=n) as L:
        L.sessions_put(keys, vals)

        def hits(_):
            du.copy_(du0)   # (inside the events: a device copy of 64 n bytes; its own time is row a0)
            run(L)
        t = timed(torch, stream, a.reps, a.warmup, hits)
        t0 = timed(torch, stream, a.reps, a.warmup, lambda _: du.copy_(du0))
        hits(None)
        torch.cuda.synchronize()
        hu = umem.copy()
        w0 = time.perf_counter()
        hv, hs = lb.lb_host(hu, descs, L, 0, 4)
        host_ms = (time.perf_counter() - w0) * 1e3
        same = bool(np.array_equal(dv.cpu().numpy(), hv) and np.array_equal(du.cpu().numpy(), hu))
        ok = ok and same
        row("a0 restore copy alone", t0)
        row("a hits", {**t, "minus_restore_us": t["event_us_median"] - t0["event_us_median"], "equal_host": same,
                       "stats": st.cpu().numpy().tolist()})
        row("c host, hits", {"wall_ms": host_ms, "stats": hs.tolist()})

    # b: all new flows (a fresh object per call; the restore copy inside the events as above);
    # two sessions per frame must fit XSKNF_GPU_LB_MAX_SESSIONS
    nb = min(n, lb.MAX_SESSIONS // 2)

    def fresh():
        return lb.LoadBalancer.from_backends(bk, max_sessions=2 * nb)

    def new(L):
        du.copy_(du0)
        run(L, nb)
    t = timed(torch, stream, a.reps, a.warmup, new, fresh)
    with fresh() as L:
        new(L)
        torch.cuda.synchronize()
        hu = umem[:64 * nb].copy()
        w0 = time.perf_counter()
        hv, hs = lb.lb_host(hu, descs[:nb], L, 0, 4)
        host_ms = (time.perf_counter() - w0) * 1e3
        same = bool(np.array_equal(dv.cpu().numpy()[:nb], hv) and np.array_equal(du.cpu().numpy()[:64 * nb], hu))
        ok = ok and same
        row("b new flows", {**t, "new_flow_frames": nb, "minus_restore_us": t["event_us_median"] - t0["event_us_median"], "equal_host": same,
                            "stats": st.cpu().numpy().tolist()})
        row("c host, new flows", {"wall_ms": host_ms, "stats": hs.tolist()})

    # d: the firewall over the same frames
    rules = np.zeros(1000, dtype=firewall.RULE_DTYPE)
    rules.view(np.uint8).reshape(-1, 20)[:, :12] = rng.integers(0, 256, (1000, 12), dtype=np.uint8)
    rules["proto"], rules["action"] = 17, 1
    with firewall.Acl.from_rules(rules) as acl:
        du.copy_(du0)
        t = timed(torch, stream, a.reps, a.warmup,
                  lambda _: firewall.firewall_batch_ptr(du.data_ptr(), 64 * n, dd.data_ptr(), n, acl, dv.data_ptr(),
                                                        stream.cuda_stream))
        row("d firewall, 1000 rules", t)

    # e: the ordered path: m new flows, room for m sessions only
    m = min(a.ordered_frames, n)

    def small():
        return lb.LoadBalancer.from_backends(bk, max_sessions=m)

    def ordered(L):
        du.copy_(du0)
        run(L, m)
    t = timed(torch, stream, max(3, a.reps // 3), 1, ordered, small)
    s = st.cpu().numpy().tolist()
    ok = ok and s[6] == 1
    row("e ordered path", {**t, "ordered_frames": m, "us_per_frame": t["event_us_median"] / m, "stats": s})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
