#!/usr/bin/env python3
"""The lbfw NF's device batch against the two calls it fuses.

tools/lb_measure.py's frames -- 1,048,576 of 64 B (ihl 5, UDP), one per 64-byte
slot, resident on device 0 -- its restore copy inside the events and its timing
(HIP events, median with min-max after warm-ups).  All rows in one run:
  lb        lb_batch, every frame's session put before the batch;
  fw        firewall_batch over the same frames, 1,000 and 1,000,000 rules;
  lbfw      lbfw_batch over the same sessions with acl=None, and with 1,000 and
            1,000,000 rules at hit share 0 (random rules: no frame matches) and
            1/2 (every odd frame carries the key of rule (i / 2) % rules instead
            of its own; the even frames still find their sessions);
  lbfw new  each of the first 1,000,000 frames the only frame of a new flow (a
            fresh object per call) behind the 1,000,000-rule ACL, hit share 0
            and 1/2.
The yardstick: the lb row plus the fw row of the same ACL is what one fused
pass must beat at hit share 0, by more than the two rows' min-max spread.  The
hit-share-1/2 rows are checked against xsknf_gpu_lbfw_host.  One JSON line per
row, to stdout and to --out.  XSKNF_GPU_LIB selects another build of the
library for an A/B (each row names the directory of the library it ran on).

  python tools/lbfw_measure.py [--reps 10] [--warmup 2] [--frames 1048576] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lb_measure import batch, timed   # noqa: E402


def random_rules(rng, count, firewall):
    rules = np.zeros(count, dtype=firewall.RULE_DTYPE)
    rules.view(np.uint8).reshape(-1, 20)[:, :12] = rng.integers(0, 256, (count, 12), dtype=np.uint8)
    rules["proto"], rules["action"] = 17, 1
    return rules


def half_hits(umem, rules):
    """umem with every odd frame's key replaced by that of rule (i / 2) % rules."""
    out = umem.copy()
    raw = out.reshape(-1, 64)
    odd = np.arange(1, raw.shape[0], 2)
    raw[odd, 26:38] = rules.view(np.uint8).reshape(-1, 20)[(odd // 2) % rules.shape[0], :12]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from xsknf_amd import _lib, firewall, lb, lbfw

    if not torch.cuda.is_available():
        sys.exit("lbfw_measure: no GPU (there is no CPU fallback for a measurement)")
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
    umem, descs = batch(rng, n, bk["vaddr"][::per], bk["vport"][::per])
    stream = torch.cuda.current_stream(dev)
    du0 = torch.from_numpy(umem).to(dev)
    du = du0.clone()
    dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    dv = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(lb.lb_workspace(n), dtype=torch.uint8, device=dev)
    st = torch.zeros(8, dtype=torch.int64, device=dev)
    lines, ok = [], True
    rules = {1000: random_rules(rng, 1000, firewall), 1000000: random_rules(rng, 1000000, firewall)}
    half = {c: torch.from_numpy(half_hits(umem, r)).to(dev) for c, r in rules.items()}

    def row(name, extra):
        lines.append({"row": name, "frames": n, "lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), **extra})
        print(json.dumps(lines[-1]), flush=True)

    def run_lbfw(A, L, src, m=n):
        du.copy_(src)   # (inside the events, as in lb_measure: its own time is the first row)
        lbfw.lbfw_batch_ptr(du.data_ptr(), 64 * m, dd.data_ptr(), m, 0, 4, A, L, dv.data_ptr(), ws.data_ptr(),
                            ws.numel(), st.data_ptr(), stream.cuda_stream)

    def run_lb(L):
        du.copy_(du0)
        lb.lb_batch_ptr(du.data_ptr(), 64 * n, dd.data_ptr(), n, 0, 4, L, dv.data_ptr(), ws.data_ptr(), ws.numel(),
                        st.data_ptr(), stream.cuda_stream)

    def equal_host(A, L, src_host, m=n):
        """The device's last result against xsknf_gpu_lbfw_host (the host table
        holds what the device table held before the call)."""
        torch.cuda.synchronize()
        hu = src_host[:64 * m].copy()
        hv, hs = lbfw.lbfw_host(hu, descs[:m], A, L, 0, 4)
        return bool(np.array_equal(dv.cpu().numpy()[:m], hv) and np.array_equal(du.cpu().numpy()[:64 * m], hu)
                    and st.cpu().numpy().tolist()[:6] == hs.tolist()[:6] and int(st[7]) == int(hs[7]))

    t0 = timed(torch, stream, a.reps, a.warmup, lambda _: du.copy_(du0))
    row("restore copy alone", t0)
    keys = np.zeros(n, dtype=lb.KEY_DTYPE)
    raw = umem.reshape(n, 64)
    keys.view(np.uint8).reshape(n, 16)[:, 0:8] = raw[:, 26:34]
    keys.view(np.uint8).reshape(n, 16)[:, 8:12] = raw[:, 34:38]
    keys["proto"] = 17
    vals = np.zeros(n, dtype=lb.VALUE_DTYPE)
    vals["addr"], vals["port"], vals["ifindex"], vals["dir"] = 0xc0a80001, 0x901f, 1, lb.TO_BACKEND
    base = {}
    with lb.LoadBalancer.from_backends(bk, max_sessions=n) as L:
        L.sessions_put(keys, vals)
        base["lb"] = timed(torch, stream, a.reps, a.warmup, lambda _: run_lb(L))
        row("lb_batch, all hits", {**base["lb"], "stats": st.cpu().numpy().tolist()})
        t = timed(torch, stream, a.reps, a.warmup, lambda _: run_lbfw(None, L, du0))
        row("lbfw_batch, acl=None, all hits", {**t, "stats": st.cpu().numpy().tolist()})
        for count, r in rules.items():
            with firewall.Acl.from_rules(r) as A:
                du.copy_(du0)
                fw = timed(torch, stream, a.reps, a.warmup,
                           lambda _: firewall.firewall_batch_ptr(du.data_ptr(), 64 * n, dd.data_ptr(), n, A, dv.data_ptr(),
                                                                 stream.cuda_stream))
                row(f"firewall_batch, {count} rules", fw)
                t = timed(torch, stream, a.reps, a.warmup, lambda _: run_lbfw(A, L, du0))
                s = st.cpu().numpy().tolist()
                # the yardstick: both rows' medians against the fused call (the restore copy is in lb's and in ours)
                total = base["lb"]["event_us_median"] + fw["event_us_median"]
                spread = (base["lb"]["event_us_max"] - base["lb"]["event_us_min"]) + (fw["event_us_max"] - fw["event_us_min"])
                row(f"lbfw_batch, {count} rules, hit share 0",
                    {**t, "stats": s, "lb_plus_firewall_us": total, "two_rows_spread_us": spread,
                     "fused_saves_us": total - t["event_us_median"],
                     "beats_the_sum_by_more_than_the_spread": bool(total - t["event_us_median"] > spread)})
                ok = ok and s[7] == 0 and s[1] == n
                t = timed(torch, stream, a.reps, a.warmup, lambda _: run_lbfw(A, L, half[count]))
                s = st.cpu().numpy().tolist()
                same = equal_host(A, L, half[count].cpu().numpy())
                ok = ok and same and s[7] == n // 2
                row(f"lbfw_batch, {count} rules, hit share 1/2", {**t, "stats": s, "equal_host": same})

    # all new flows (a fresh object per call), behind the 1,000,000-rule ACL
    nb = min(n, lb.MAX_SESSIONS // 2)

    def fresh():
        return lb.LoadBalancer.from_backends(bk, max_sessions=2 * nb)
    with firewall.Acl.from_rules(rules[1000000]) as A:
        for name, src in (("0", du0), ("1/2", half[1000000])):
            t = timed(torch, stream, a.reps, a.warmup, lambda L: run_lbfw(A, L, src, nb), fresh)
            with fresh() as L:
                run_lbfw(A, L, src, nb)
                same = equal_host(A, L, src.cpu().numpy(), nb)
                ok = ok and same
                row(f"lbfw_batch, all new flows, 1000000 rules, hit share {name}",
                    {**t, "new_flow_frames": nb, "stats": st.cpu().numpy().tolist(), "equal_host": same})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
