#!/usr/bin/env python3
"""xsknf_gpu_acl_update on a large ACL against the only way there was to change
a rule: destroy the ACL and create it again.

The ACL: 950,000 random rules in 2^21 slots on device 0 -- not the 1,000,000 of
XSKNF_GPU_ACL_MAX_RULES, so that an update which puts more keys than it deletes
still fits the map.  Rows:
  update of 1, 1,000 and 100,000 ops -- half of them puts of new keys, a quarter
      replaces, a quarter deletes, shuffled;
  rebuild -- slots / 4 + 1 deletes in one call, which the tombstone bound
      answers with the rebuild in place and the whole table on the stream.
Every repetition starts from a freshly created ACL, so each sample sees the same
table, and that creation is the yardstick: xsknf_gpu_acl_destroy of the old
object plus xsknf_gpu_acl_create of the rule set the update leaves, wall clock.

Per row, after --warmup repetitions, --reps times: median, min and max of
  call_us     wall clock around xsknf_gpu_acl_update: the host pass, the records
              into the pinned buffer, the copy's and the kernel's enqueue;
  host_us     the same call on an ACL without a device table (a child process
              that sees no device): the host pass alone;
  enqueue_us  call_us - host_us, from the medians;
  device_us   HIP events on the stream around the call, the stream held busy by
              device copies enqueued in front until the call has returned, so
              that the events bracket the records' copy and the scatter (or the
              table's copy) and nothing of the host's time; a sample whose
              blocker had ended before the call returned is dropped and counted;
  recreate_ms the yardstick.
A fresh object's first update also allocates its pinned buffer; the update rows
keep that out with a first update of as many replaces that change nothing, the
rebuild row (40 MiB of pinned memory for the table) has it in call_us.
After every timed update the device table's dump must equal the host table's.
One JSON line per row, to stdout and to --out.

  python tools/acl_update_measure.py [--reps 20] [--warmup 3] [--scale 1] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 8.0            # MI355X HBM3E peak, TB/s
SEED = 20264


def random_rules(rng, n):
    from xsknf_amd import firewall

    r = np.zeros(n, dtype=firewall.RULE_DTYPE)
    raw = r.view(np.uint8).reshape(-1, 20)
    raw[:, :12] = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    r["proto"] = np.where(rng.integers(0, 2, n) == 1, 6, 17)
    r["action"] = rng.integers(-1, 3, n)
    return r


def workload(scale):
    """(rules, slots, rows): rows are (name, ops, rule set after the update)."""
    from xsknf_amd import firewall

    rng = np.random.default_rng(SEED)
    n_rules = max(64, int(950000 * scale))
    slots = 64
    while slots < 2 * n_rules:
        slots *= 2
    rules = random_rules(rng, n_rules)
    rows = []
    for n_ops in (1, 1000, 100000):
        n_ops = max(1, int(n_ops * scale)) if n_ops > 1 else 1
        n_put = n_ops - n_ops // 2
        n_rep, n_del = n_ops // 4, n_ops // 2 - n_ops // 4
        new = random_rules(rng, n_put)
        pick = rng.choice(n_rules, n_rep + n_del, replace=False)
        rep = rules[pick[:n_rep]].copy()
        rep["action"] = 7
        ops = np.concatenate([firewall.make_ops(new, firewall.PUT), firewall.make_ops(rep, firewall.PUT),
                              firewall.make_ops(rules[pick[n_rep:]], firewall.DELETE)])
        ops = ops[rng.permutation(ops.shape[0])]
        after = rules.copy()
        after["action"][pick[:n_rep]] = 7
        keep = np.ones(n_rules, dtype=bool)
        keep[pick[n_rep:]] = False
        rows.append((f"update_{n_ops}", ops, np.concatenate([after[keep], new]), n_put, n_rep, n_del))
    n_del = slots // 4 + 1
    rows.append(("rebuild", firewall.make_ops(rules[:n_del], firewall.DELETE), rules[n_del:], 0, 0, n_del))
    return rules, slots, rows


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]} if xs else None


def host_only(a):
    """The child: no device, the host pass alone.  One JSON line."""
    from xsknf_amd import _lib, firewall

    rules, slots, rows = workload(a.scale)
    lib = _lib.load()
    out = {}
    for name, ops, _, _, _, _ in rows:
        ts = []
        for i in range(a.warmup + a.reps):
            with firewall.Acl.from_rules(rules, slots) as acl:
                assert acl.info["device_bytes"] == 0
                t0 = time.perf_counter()
                rc = lib.xsknf_gpu_acl_update(acl.handle, ops.ctypes.data, ops.shape[0], None)
                t1 = time.perf_counter()
                assert rc == 0
            if i >= a.warmup:
                ts.append((t1 - t0) * 1e6)
        out[name] = stats(ts)
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the rule and op counts (rehearsals)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_only:
        return host_only(a)

    import torch
    from xsknf_amd import _lib, firewall

    if not torch.cuda.is_available():
        sys.exit("acl_update_measure: no GPU (there is no CPU fallback for a measurement)")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-only", "--reps", str(a.reps), "--warmup",
                            str(a.warmup), "--scale", str(a.scale)], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    if child.returncode:
        sys.exit("acl_update_measure: the host-only child failed:\n" + child.stderr[-2000:])
    host = json.loads(child.stdout.strip().splitlines()[-1])

    dev = torch.device("cuda:0")
    lib = _lib.load()
    rules, slots, rows = workload(a.scale)
    stream = torch.cuda.current_stream(dev)
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst.copy_(src)
    e0.record(stream)
    for _ in range(8):
        dst.copy_(src)
    e1.record(stream)
    e1.synchronize()
    copy_ms = e0.elapsed_time(e1) / 8
    lines, ok = [], True
    acl = firewall.Acl.from_rules(rules, slots)
    for name, ops, after, n_put, n_rep, n_del in rows:
        call, devt, rec, dropped = [], [], [], 0
        block_ms = 2.0
        for i in range(a.warmup + a.reps):
            # the yardstick, and the fresh table of this repetition: first the rule
            # set the update leaves (timed), then the start again (not timed)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acl.close()
            acl = firewall.Acl.from_rules(after, slots)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            acl.close()
            acl = firewall.Acl.from_rules(rules, slots)
            if name != "rebuild":
                # as many replaces that change nothing: the object's pinned buffer
                # exists, as it does for every update but an object's first
                acl.update(puts=rules[:ops.shape[0]], stream=stream)
            torch.cuda.synchronize()
            blocker = torch.cuda.Event()
            ea, eb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(int(block_ms / copy_ms) + 1):
                dst.copy_(src)
            blocker.record(stream)
            ea.record(stream)
            t2 = time.perf_counter()
            rc = lib.xsknf_gpu_acl_update(acl.handle, ops.ctypes.data, ops.shape[0], stream.cuda_stream)
            t3 = time.perf_counter()
            eb.record(stream)
            held = not blocker.query()
            eb.synchronize()
            if rc:
                sys.exit(f"acl_update_measure: {name}: rc={rc}")
            block_ms = max(block_ms, 3e3 * (t3 - t2))
            if i < a.warmup:
                continue
            rec.append((t1 - t0) * 1e3)
            call.append((t3 - t2) * 1e6)
            if held:
                devt.append(ea.elapsed_time(eb) * 1e3)
            else:
                dropped += 1
        h, d = acl.dump(), acl.dump(device=True)
        same = h.tobytes() == d.tobytes() and h.shape[0] == after.shape[0]
        ok = ok and same
        info = acl.info
        rebuilt = name == "rebuild"
        records = 0 if rebuilt else ops.shape[0]
        dev_bytes = 20 * slots if rebuilt else records * (24 + 20)
        c, dv, r = stats(call), stats(devt), stats(rec)
        line = {"row": name, "rules": int(rules.shape[0]), "slots": slots, "ops": int(ops.shape[0]), "puts_new": n_put,
                "replaces": n_rep, "deletes": n_del, "rebuild_in_place": rebuilt, "records": records,
                "rules_after": info["rules"], "tombstones_after": info["tombstones"], "max_probe_after": info["max_probe"],
                "device_equals_host": bool(same), "reps": a.reps,
                "call_us_median": c["median"], "call_us_min": c["min"], "call_us_max": c["max"],
                "host_us_median": host[name]["median"], "host_us_min": host[name]["min"], "host_us_max": host[name]["max"],
                "enqueue_us": c["median"] - host[name]["median"],
                "device_us_median": dv and dv["median"], "device_us_min": dv and dv["min"], "device_us_max": dv and dv["max"],
                "device_samples_dropped": dropped,
                "device_bytes": dev_bytes, "h2d_bytes": 20 * slots if rebuilt else 24 * records,
                "device_bound_us": dev_bytes / (HBM_TBS * 1e12) * 1e6,
                "device_over_bound": dv and dv["median"] / (dev_bytes / (HBM_TBS * 1e12) * 1e6),
                "recreate_ms_median": r["median"], "recreate_ms_min": r["min"], "recreate_ms_max": r["max"],
                "recreate_over_call": r["median"] * 1e3 / c["median"]}
        lines.append(line)
        print(json.dumps(line), flush=True)
    acl.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
