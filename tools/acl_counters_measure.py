#!/usr/bin/env python3
"""What an ACL's hit counters cost the firewall's device lookup.

Each point is 1,048,576 frames of 64 bytes against an ACL of 1,000 or 1,000,000
random rules, under three traffic shapes:
  distinct  frame i carries rule i mod rules: the 64 lanes of a wave hit 64 rules
  one       every frame carries the same rule: one elephant flow
  skewed    half the frames on 16 rules, the rest spread over all
and these variants, each in a process of its own (the library is chosen when it
is loaded):
  parent    the lookup of another build of the library (--parent-lib: the
            commit before the counters), through the calls both have
  plain     this build, an ACL that never enabled counters
  count     this build, counters enabled: kernel_firewall_count.h
  naive     the A/B build (make ab, --ab-lib) with XSKNF_ACL_COUNT_SHAPE=naive:
            one atomic pair per hit
  wave      the A/B build, XSKNF_ACL_COUNT_SHAPE=wave: a wave's hits on one slot
            add once (kernel_acl_count.h count_hits, what lb_propose<true> uses)
  stage     the A/B build, XSKNF_ACL_COUNT_SHAPE=stage: every hit through the
            block's LDS stage, added when the block ends
Per point and variant, after --warmup launches, --reps launches each between two
HIP events: median, min and max in microseconds (the spread is reported beside
every figure; nothing is averaged).  The counting variants check the device
totals against the launches made.  And one row for the rebuild in place of a
950,000-rule ACL (slots / 4 + 1 deletes) with and without counters, timed as
tools/acl_update_measure.py times it but without the held stream (call + device,
wall clock to the stream's end).  And the lbfw batch (tools/lbfw_measure.py's
frames and timing: 1,048,576 frames of known sessions, the restore copy inside
the events) behind 1,000 rules, with a counting ACL and without: at hit share 0
(DESIGN 4.5's case: no frame matches a rule, every frame is the load
balancer's) and at hit share 1/2 (every odd frame carries a rule's key: the
gate's wave combine at work, 32 distinct rules per wave).  One JSON line per
row, to stdout and --out.

  python tools/acl_counters_measure.py --parent-lib PATH --ab-lib build/ab/libxsknf_gpu.so \\
      [--reps 30] [--warmup 5] [--out profiles/acl_counters/acl_counters_measure.jsonl]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
SEED = 20270
RULE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1"),
                 ("pad", "u1", (3,)), ("action", "<i4")])
OP = np.dtype([("rule", RULE), ("op", "<u4")])


def random_rules(rng, n):
    r = np.zeros(n, dtype=RULE)
    r.view(np.uint8).reshape(-1, 20)[:, :12] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    r["proto"] = np.where(rng.integers(0, 2, n) == 1, 6, 17)
    r["action"] = rng.integers(1, 3, n)
    return r


def frames_of(rules, pick, rng):
    fr = rng.integers(0, 256, (pick.shape[0], 64), dtype=np.uint8)
    raw = rules.view(np.uint8).reshape(-1, 20)[pick]
    fr[:, 12], fr[:, 13], fr[:, 14] = 8, 0, 0x45
    fr[:, 23] = raw[:, 12]
    fr[:, 26:38] = raw[:, 0:12]
    descs = np.zeros((pick.shape[0], 2), dtype=np.uint64)
    descs[:, 0] = np.arange(pick.shape[0], dtype=np.uint64) * 64
    descs[:, 1] = 64
    return fr.reshape(-1), descs


def picks(rng, n_rules):
    skew = rng.integers(0, n_rules, N)
    hot = rng.random(N) < 0.5
    skew[hot] = rng.integers(0, 16, int(hot.sum()))
    return {"distinct": np.arange(N) % n_rules, "one": np.zeros(N, dtype=np.int64), "skewed": skew}


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def child(a):
    """One variant in this process: the library by ctypes alone, so that a build
    without the counters' calls serves too.  One JSON line per point."""
    import torch

    lib = ctypes.CDLL(a.lib)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.xsknf_gpu_acl_create.argtypes = [ctypes.POINTER(vp), vp, u32, u32]
    lib.xsknf_gpu_acl_destroy.argtypes = [vp]
    lib.xsknf_gpu_acl_update.argtypes = [vp, vp, u32, vp]
    lib.xsknf_gpu_firewall_batch.argtypes = [vp, u64, vp, u32, vp, vp, vp]
    counting = a.variant in ("count", "naive", "wave", "stage")
    if counting:
        lib.xsknf_gpu_acl_counters_enable.argtypes = [vp]
        lib.xsknf_gpu_acl_counters_dump.argtypes = [vp, ctypes.c_int, vp, vp, u32, ctypes.POINTER(u32), vp]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    rng = np.random.default_rng(SEED)
    for n_rules in (1000, 1000000):
        rules = random_rules(rng, n_rules)
        h = vp()
        assert lib.xsknf_gpu_acl_create(ctypes.byref(h), rules.ctypes.data, n_rules, 0) == 0
        if counting:
            assert lib.xsknf_gpu_acl_counters_enable(h) == 0
        launches = 0
        for shape, pick in picks(rng, n_rules).items():
            umem, descs = frames_of(rules, pick, rng)
            du, dd = torch.from_numpy(umem).to(dev), torch.from_numpy(descs.view(np.uint8)).to(dev)
            dv = torch.empty(N, dtype=torch.int32, device=dev)
            ts = []
            for i in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = lib.xsknf_gpu_firewall_batch(du.data_ptr(), umem.size, dd.data_ptr(), N, h, dv.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                assert rc == 0
                launches += 1
                if i >= a.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            assert bool((dv == torch.from_numpy(rules["action"][pick]).to(dev)).all())
            if counting:
                tot = np.zeros(4, dtype=np.uint64)
                n = u32(0)
                lib.xsknf_gpu_acl_counters_dump(h, 1, None, None, 0, ctypes.byref(n), tot.ctypes.data)
                assert tot.tolist() == [launches * N, launches * N, 0, 0], tot
            s = stats(ts)
            print(json.dumps({"row": "lookup", "variant": a.variant, "rules": n_rules, "shape": shape, "frames": N,
                              "reps": a.reps, "us_median": s["median"], "us_min": s["min"], "us_max": s["max"]}), flush=True)
        lib.xsknf_gpu_acl_destroy(h)
    if a.variant not in ("plain", "count"):
        return 0
    # the rebuild in place of a 950,000-rule ACL, with the counters' carry or without
    rules = random_rules(rng, 950000)
    ops = np.zeros((1 << 21) // 4 + 1, dtype=OP)
    ops["rule"] = rules[:ops.shape[0]]
    ops["op"] = 1
    ts = []
    for i in range(2 + 8):
        h = vp()
        assert lib.xsknf_gpu_acl_create(ctypes.byref(h), rules.ctypes.data, 950000, 1 << 21) == 0
        if counting:
            assert lib.xsknf_gpu_acl_counters_enable(h) == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(stream)
        rc = lib.xsknf_gpu_acl_update(h, ops.ctypes.data, ops.shape[0], stream.cuda_stream)
        e1.record(stream)
        t1 = time.perf_counter()
        e1.synchronize()
        t2 = time.perf_counter()
        assert rc == 0
        lib.xsknf_gpu_acl_destroy(h)
        if i >= 2:
            ts.append(((t1 - t0) * 1e6, (t2 - t0) * 1e6))
    c, w = stats([t[0] for t in ts]), stats([t[1] for t in ts])
    print(json.dumps({"row": "rebuild", "variant": a.variant, "rules": 950000, "slots": 1 << 21, "deletes": int(ops.shape[0]),
                      "reps": 8, "call_us_median": c["median"], "call_us_min": c["min"], "call_us_max": c["max"],
                      "to_stream_end_us_median": w["median"], "to_stream_end_us_min": w["min"],
                      "to_stream_end_us_max": w["max"]}), flush=True)
    return 0


def lbfw_child(a):
    """The lbfw rows, through the package (this build alone)."""
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from lb_measure import batch, timed
    from lbfw_measure import half_hits, random_rules as lbfw_rules
    from xsknf_amd import firewall, lb, lbfw

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(4404)
    n, nsvc, per = N, 16, 8
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
    rules = lbfw_rules(rng, 1000, firewall)
    half = torch.from_numpy(half_hits(umem, rules)).to(dev)
    keys = np.zeros(n, dtype=lb.KEY_DTYPE)
    raw = umem.reshape(n, 64)
    keys.view(np.uint8).reshape(n, 16)[:, 0:8] = raw[:, 26:34]
    keys.view(np.uint8).reshape(n, 16)[:, 8:12] = raw[:, 34:38]
    keys["proto"] = 17
    vals = np.zeros(n, dtype=lb.VALUE_DTYPE)
    vals["addr"], vals["port"], vals["ifindex"], vals["dir"] = 0xc0a80001, 0x901f, 1, lb.TO_BACKEND

    def run(A, L, src):
        du.copy_(src)
        lbfw.lbfw_batch_ptr(du.data_ptr(), 64 * n, dd.data_ptr(), n, 0, 4, A, L, dv.data_ptr(), ws.data_ptr(), ws.numel(),
                            st.data_ptr(), stream.cuda_stream)
    with lb.LoadBalancer.from_backends(bk, max_sessions=n) as L:
        L.sessions_put(keys, vals)
        for counting in (False, True):
            with firewall.Acl.from_rules(rules) as A:
                if counting:
                    A.counters_enable()
                for share, src, gated in (("0", du0, 0), ("1/2", half, n // 2)):
                    t = timed(torch, stream, a.reps, a.warmup, lambda _: run(A, L, src))
                    s = st.cpu().numpy().tolist()
                    assert s[7] == gated and s[6] == 0, s
                    print(json.dumps({"row": "lbfw", "variant": "count" if counting else "plain", "rules": 1000,
                                      "hit_share": share, "frames": n, "reps": a.reps, "us_median": t["event_us_median"],
                                      "us_min": t["event_us_min"], "us_max": t["event_us_max"]}), flush=True)
                if counting:
                    launches = 2 * (a.reps + a.warmup)
                    tot = A.counters(device=True)[2].tolist()
                    assert tot == [launches * n, launches * n // 4, launches * n * 3 // 4, 0], tot
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libxsknf_gpu.so of the commit before the counters")
    ap.add_argument("--ab-lib", default=os.path.join(ROOT, "build", "ab", "libxsknf_gpu.so"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variant:
        return lbfw_child(a) if a.variant == "lbfw" else child(a)
    mine = os.path.join(ROOT, "xsknf_amd", "lib", "libxsknf_gpu.so")
    variants = [("parent", a.parent_lib, {}), ("plain", mine, {}), ("count", mine, {}),
                ("naive", a.ab_lib, {"XSKNF_ACL_COUNT_SHAPE": "naive"}), ("wave", a.ab_lib, {"XSKNF_ACL_COUNT_SHAPE": "wave"}),
                ("stage", a.ab_lib, {"XSKNF_ACL_COUNT_SHAPE": "stage"}), ("lbfw", mine, {})]
    lines = []
    for name, lib, env in variants:
        if not lib or not os.path.exists(lib):
            print(f"acl_counters_measure: no library for {name}: skipped", file=sys.stderr)
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name, "--lib", lib, "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        if r.returncode:
            sys.exit(f"acl_counters_measure: {name} failed:\n" + r.stderr[-3000:])
        for ln in r.stdout.strip().splitlines():
            lines.append(json.loads(ln))
            print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
