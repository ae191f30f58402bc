"""Options and ingress belong to a batch: with batches of DIFFERENT options in
flight together, every batch is processed with its own.

Consecutive batches step through tests/option_cases.py's OPTION_CYCLE (six
option sets, no two with the same forward verdict, payload multiples 1, 3, 2,
1, 0, 7919), on every host path, across the contexts that share the resident
kernel, from worker threads on mixed paths, and over device-resident launches
on separate streams.  Every case compares all verdicts and the whole UMEM with
the per-batch oracle, and first asserts -- on the oracle alone -- that each of
its batches would differ under any other member of the cycle
(tests/test_option_cases.py checks the same on the CPU).  A header read ahead
of the acquire, a slot's records applied with the previous batch's verdict, a
launch that picked up another stream's counters: each shows as a mismatch.
"""
import threading
import time

import numpy as np
import pytest

from tests import option_cases as OC
from xsknf_amd import Checksummer, ChecksummerOptions, HostPath

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cs():
    """The contexts' Checksummer: every batch brings its own options, so these
    (DROP, 5 iterations, verdict -1) are nobody's."""
    return Checksummer(ChecksummerOptions(action=1, csum_iterations=5), num_interfaces=7, frame_len_hint=1500)


def submit(hp, case, j, out):
    lo, hi, o = case.batches()[j]
    return hp.submit(case.b.descs[lo:hi], out[lo:hi], ingress_ifindex=o[0], opts=OC.csum_opts(o))


def same(case, umem, out, what=""):
    """All verdicts and the whole UMEM against the per-batch oracle; names the
    first batch that differs and the options its verdicts look like."""
    wu, wv = case.want()
    for j, (lo, hi, o) in enumerate(case.batches()):
        if not np.array_equal(out[lo:hi], wv[lo:hi]):
            bad = lo + int(np.flatnonzero(out[lo:hi] != wv[lo:hi])[0])
            like = [x for x in OC.OPTION_CYCLE if OC.fwd(x) == out[bad]]
            raise AssertionError(f"{what} batch {j} [{lo}, {hi}) under {o}: verdict {out[bad]} at frame {bad}, "
                                 f"oracle {wv[bad]}; the forward verdict of {like}")
    assert np.array_equal(out[case.n:], np.full(out.shape[0] - case.n, 7, dtype=np.int32)), what
    if not np.array_equal(umem, wu):
        at = int(np.flatnonzero(umem != wu)[0])
        f = int(np.searchsorted(case.b.frame_offsets().astype(np.int64), at, side="right")) - 1
        j = int(np.searchsorted(case.cuts, f, side="right")) - 1
        raise AssertionError(f"{what} UMEM differs from byte {at}: frame {f}, batch {j} under "
                             f"{case.opts[min(j, len(case.opts) - 1)]}")


@pytest.mark.parametrize("checks", ["zero", "nic"])
@pytest.mark.parametrize("path", ["zerocopy", "staged", "resident"])
def test_one_context_batches_in_flight(dev, cs, path, checks):
    """One context, every batch submitted without waiting: more batches than the
    5 slots and the 8 ring entries, so both are reused by a batch with other
    options (a 700-frame batch is three entries under one option set).  `nic`:
    the batches of iteration count 1 find their checks in place -- the write
    elision, and STAGED's records only where a check changes, next to batches
    that rewrite everything.  RESIDENT waits and sleeps past the kernel's idle
    exit once: the relaunch starts at an entry whose header has been rewritten."""
    case = OC.one_context(checks)
    k = OC.constants()
    assert len(case.opts) > 4 * k["entries"] > 4 * k["slots"]
    case.leak_is_visible()
    umem = case.b.umem.copy()
    out = np.full(case.b.n, 7, dtype=np.int32)
    with HostPath(cs, umem, path=path, max_batch=OC.ONE_CONTEXT_MAX_BATCH) as hp:
        tickets = []
        for j in range(len(case.opts)):
            tickets.append(submit(hp, case, j, out))
            if path == "resident" and j == len(case.opts) // 2:
                hp.wait(tickets[-1])
                time.sleep(0.03)            # past the kernel's 1 ms idle exit
        hp.wait(tickets[-1])
        st = hp.stats()
    assert st["frames"] == case.b.n
    if path == "resident":
        assert st["resident_batches"] == sum(OC.entries(hi - lo, k["entry_frames"]) for lo, hi, _ in case.batches())
        assert st["resident_launches"] >= 2
    same(case, umem, out, f"{path} {checks}")


def test_process_batch_takes_the_call_options(dev, cs):
    """HostPath.process_batch with per-call options, path by path (the blocking
    call the hook's one-call mode makes): the first batches of the cycle."""
    case = OC.one_context("zero")
    wu, wv = case.want()
    hi = case.cuts[8]
    for path in ("zerocopy", "staged", "resident"):
        umem = case.b.umem.copy()
        with HostPath(cs, umem, path=path, max_batch=OC.ONE_CONTEXT_MAX_BATCH) as hp:
            v = np.concatenate([hp.process_batch(case.b.descs[lo:h], ingress_ifindex=o[0], opts=OC.csum_opts(o))
                                for lo, h, o in case.batches()[:8]])
        assert np.array_equal(v, wv[:hi]), path
        end = int(case.b.frame_offsets()[hi])
        assert np.array_equal(umem[:end], wu[:end]) and np.array_equal(umem[end:], case.b.umem[end:]), path


@pytest.mark.parametrize("n_ctx,max_batch,batch", OC.SHARED_SHAPES,
                         ids=["8-groups-of-4", "8-groups-of-1", "40-blocks-serve-several-entries"])
def test_resident_contexts_share_one_kernel(dev, cs, n_ctx, max_batch, batch):
    """The shapes of test_gpu_parity's test of the same name, context c stepping
    the cycle from offset c: at any moment neighbouring rings, and neighbouring
    entries of one ring -- which one block serves where 40 contexts share the
    grid -- hold different forward verdicts and payload multiples."""
    cases = OC.shared_kernel(n_ctx, max_batch, batch)
    OC.all_leaks_visible(cases)
    OC.want_all(cases)
    umems = [c.b.umem.copy() for c in cases]
    outs = [np.full(c.b.n, 7, dtype=np.int32) for c in cases]
    hps = []
    try:
        for u in umems:
            hps.append(HostPath(cs, u, path="resident", max_batch=max_batch))
        tickets = [None] * n_ctx
        for j in range(len(cases[0].opts)):
            for c, (hp, case) in enumerate(zip(hps, cases)):
                tickets[c] = submit(hp, case, j, outs[c])
        for hp, t in zip(hps, tickets):
            hp.wait(t)
        stats = [hp.stats() for hp in hps]
    finally:
        for hp in hps:
            hp.close()
    ef = OC.constants()["entry_frames"]
    for c, (case, st) in enumerate(zip(cases, stats)):
        assert st["frames"] == case.n
        assert st["resident_batches"] == sum(OC.entries(hi - lo, ef) for lo, hi, _ in case.batches())
        same(case, umems[c], outs[c], f"context {c}")


def test_resident_rings_join_and_leave_under_traffic(dev, cs):
    """A ring joining and one leaving stop and relaunch the shared kernel while
    the other contexts have batches of different options in flight: the
    relaunch picks each up with its own header, none is processed twice."""
    cases = OC.join_leave()
    OC.all_leaks_visible(cases)
    OC.want_all(cases)
    umems = [c.b.umem.copy() for c in cases]
    outs = [np.full(c.b.n, 7, dtype=np.int32) for c in cases]
    hp, fed, last = {}, [0] * len(cases), {}
    try:
        for s in OC.join_leave_steps():
            if s[0] == "open":
                hp[s[1]] = HostPath(cs, umems[s[1]], path="resident", max_batch=s[2])
            elif s[0] == "feed":
                c = s[1]
                lo, hi, _ = cases[c].batches()[fed[c]]
                assert hi - lo == s[2]
                last[c] = submit(hp[c], cases[c], fed[c], outs[c])
                fed[c] += 1
            else:
                hp[s[1]].wait(last[s[1]])
                hp.pop(s[1]).close()
        for c, h in hp.items():
            h.wait(last[c])
    finally:
        for h in hp.values():
            h.close()
    assert fed == [len(c.opts) for c in cases]
    for c, case in enumerate(cases):
        same(case, umems[c], outs[c], f"context {c}")


def test_mixed_paths_from_worker_threads(dev, cs):
    """Six worker threads -- two RESIDENT, two ZEROCOPY, two STAGED contexts --
    each stepping the cycle from an offset of its own with four batches out."""
    cases = OC.worker_threads()
    paths = OC.WORKER_PATHS
    OC.all_leaks_visible(cases)
    OC.want_all(cases)
    umems = [c.b.umem.copy() for c in cases]
    outs = [np.full(c.b.n, 7, dtype=np.int32) for c in cases]
    errors, stats = [], [None] * len(paths)
    start = threading.Barrier(len(paths))

    def worker(k):
        try:
            with HostPath(cs, umems[k], path=paths[k], max_batch=OC.WORKER_BATCH) as hp:
                start.wait()
                tickets = []
                for j in range(len(cases[k].opts)):
                    tickets.append(submit(hp, cases[k], j, outs[k]))
                    if len(tickets) >= OC.WORKER_OUT:
                        hp.wait(tickets[-OC.WORKER_OUT])
                hp.wait(tickets[-1])
                stats[k] = hp.stats()
        except Exception as e:   # noqa: BLE001 -- reported below
            errors.append((k, repr(e)))
            start.abort()

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(len(paths))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads), "a worker did not finish"
    assert not errors, errors
    for k, p in enumerate(paths):
        assert stats[k]["frames"] == cases[k].n
        same(cases[k], umems[k], outs[k], f"worker {k} ({p})")


def test_launches_on_separate_streams(dev):
    """24 device-resident batches (1500 B / IMIX / 64 B, 4,096 frames) on a
    stream each, four launches per stream with none waited for, every launch
    under its own options: the per-launch record-counter sets and the
    deferred-patch state stay with the launch they belong to.  The oracle is
    applied as often with the same option sets in order (ihl 2 / 3 frames make
    every pass change the next one's input)."""
    jobs = OC.streams()
    OC.all_leaks_visible(jobs)
    OC.pool_map(lambda j: j.want(), jobs)
    css = {o: Checksummer(ChecksummerOptions(action=o[3], csum_iterations=o[2]), num_interfaces=o[1],
                          frame_len_hint=1500) for o in OC.OPTION_CYCLE}
    streams = [torch.cuda.Stream(device=dev) for _ in jobs]
    bufs = []
    for j, st in zip(jobs, streams):
        with torch.cuda.stream(st):
            umem = torch.from_numpy(j.b.umem.copy()).to(dev, non_blocking=False)
            descs = torch.from_numpy(j.b.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        bufs.append((umem, descs))
    torch.cuda.synchronize()
    res = [[] for _ in jobs]
    for rep in range(OC.STREAM_LAUNCHES):
        for k, (j, st, (umem, descs)) in enumerate(zip(jobs, streams, bufs)):
            o = j.opts[rep]
            with torch.cuda.stream(st):
                res[k].append(css[o].process_batch(umem, descs, ingress_ifindex=o[0]))
    torch.cuda.synchronize()
    time.sleep(0.05)
    torch.cuda.synchronize()
    got = [(umem.cpu().numpy(), [v.cpu().numpy() for v in vs]) for (umem, _), vs in zip(bufs, res)]
    for k, (j, (gu, gvs)) in enumerate(zip(jobs, got)):
        wu, wvs = j.want()
        for rep, (gv, wv) in enumerate(zip(gvs, wvs)):
            assert np.array_equal(gv, wv), f"stream {k} ({j.length}) launch {rep} under {j.opts[rep]}"
        assert np.array_equal(gu, wu), f"stream {k} ({j.length}) under {j.opts}"
