"""Routing a checksummed batch on the device (include/xsknf_gpu.h
xsknf_gpu_route_batch; xsknf_amd/csrc/route_device.hip, kernel_route.h).

* The device against xsknf_gpu_route_host on the same arrays, for equality:
  the counts, every field of every list entry up to the totals, `order`, and
  the sentinels the buffers held past the totals.  (tests/test_route.py holds
  route_host to an independent model on the CPU.)  Sizes: around the wave and
  the tile, and past one and two trips of the scan over the tile counts (S
  tiles a trip, read from the code).
* From the hot path and after the multi-device round trip: the lists against the
  model applied to the reference's verdicts.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import ref as R
from tests import oracles
from tests import route_cases as RC
from xsknf_amd import Checksummer, ChecksummerOptions, _lib, frames, multi, route
from xsknf_amd.checksummer import ACTION_DROP, ACTION_REDIRECT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile() -> int:
    """Frames per block of the router, from the code: the workspace holds one
    count per bin and tile, so it first grows at n = T + 1."""
    w1 = route.route_workspace(1, 1)
    lo, hi = 1, 2
    while route.route_workspace(hi, 1) == w1:
        lo, hi = hi, hi * 2
    while hi - lo > 1:            # workspace(lo) == w1 < workspace(hi)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if route.route_workspace(mid, 1) == w1 else (lo, mid)
    return lo


T = _tile()
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 300001]
NIFS = [1, 2, 3, 32]
S = RC.scan_trip()                # tile counts per trip of route_scan_counts' loop
LONG_SIZES = RC.long_sizes(S, T)  # two trips, the second of one frame; three trips, the last partial


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def descs():
    """300,001 descriptors with every bit in play, and their device copy's
    bytes.  Shared, never written."""
    d = RC.random_descs(SIZES[-1], seed=81)
    d.setflags(write=False)
    return d


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


class DevRoute:
    """One xsknf_gpu_route_batch into sentinel-filled device buffers."""

    def __init__(self, dev, dd, dv, n, nif, order=True, sync=True, ws=None):
        self.n, self.nif = n, nif
        self.tx = torch.full((n * 16,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        self.fill = torch.full((n * 8,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        self.od = torch.full((n * 4,), RC.SENTINEL8, dtype=torch.uint8, device=dev) if order else None
        self.ws = torch.empty(route.route_workspace(n, nif), dtype=torch.uint8, device=dev) if ws is None else ws
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev)
            self.counts = route.route_batch_ptr(
                dd.data_ptr() if n else 0, dv.data_ptr() if n else 0, n, nif, self.tx.data_ptr() if n else 0,
                self.fill.data_ptr() if n else 0, self.od.data_ptr() if order and n else 0, self.ws.data_ptr(),
                self.ws.numel(), self.stream.cuda_stream, sync=sync)

    def result(self):
        self.stream.synchronize()
        counts = self.counts
        if counts is None:        # the header words of the workspace
            counts = [int(c) for c in self.ws[:8 * (self.nif + 1)].cpu().numpy().view(np.uint64)]
        return (self.tx.cpu().numpy().view(frames.DESC_DTYPE), self.fill.cpu().numpy().view(np.uint64),
                None if self.od is None else self.od.cpu().numpy().view(np.uint32), counts)


def _same_as_host(got, d, v, nif, what):
    """got (over sentinel-filled buffers) == xsknf_gpu_route_host's, bit for bit."""
    n = int(d.shape[0])
    htx, hfill, hod, hcounts = RC.host_route_raw(d, v, nif)
    ntx, ndrop = sum(hcounts[:nif]), hcounts[nif]
    RC.same_as(got, (htx[:ntx], hfill[:ndrop], hod, hcounts), n, what)


def test_tile_is_read_from_the_code():
    src = open(os.path.join(ROOT, "xsknf_amd", "csrc", "kernel_route.h")).read()
    threads = int(re.search(r"kThreads = (\d+);", src).group(1))
    per = int(re.search(r"kPerThread = (\d+);", src).group(1))
    assert T == threads * per
    assert re.search(r"kTile = kThreads \* kPerThread;", src)


@pytest.mark.parametrize("nif", NIFS)
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_route_host(dev, descs, n, nif):
    """Every size around the wave, the tile and several tiles (n no multiple of
    64: the last wave has lanes past the end in every round of its rank loop),
    times every interface count, times every verdict pattern: among them a wave
    of 33 distinct bins (cycle, 32 interfaces), waves of one bin, a tile of one
    bin followed by tiles with none of it, and verdicts that name no interface."""
    d = descs[:n]
    dd = _to_dev(d, dev)
    for pattern in RC.PATTERNS:
        v = RC.verdicts(pattern, n, nif, seed=n + nif, tile=T)
        dv = _to_dev(v, dev)
        got = DevRoute(dev, dd, dv, n, nif).result()
        _same_as_host(got, d, v, nif, f"{pattern} n={n} nif={nif}")
        if n == 0:
            assert got[3] == [0] * (nif + 1)
    if nif == 32 and n >= 64:
        v = RC.verdicts("cycle", n, nif)
        assert all(len(set(v[w:w + 64])) == 33 for w in range(0, n - 63, 64))


def test_scan_trip_is_read_from_the_code():
    """S is scan::kThreads, the step of the router's scan loop; the long sizes
    are written in S and T, one frame and a partial trip past whole trips."""
    assert S == RC.code_constant("block_scan.h", r"constexpr int kThreads = (\d+);")
    assert T == RC.tile_of("kernel_route.h")
    tiles = [-(-n // T) for n in LONG_SIZES]
    assert tiles == [S + 1, 2 * S + 4] and LONG_SIZES[0] % T == 1 and LONG_SIZES[1] % 64


@pytest.fixture(scope="module")
def long_descs():
    """Descriptors for the batches past one scan trip.  Shared, never written."""
    d = RC.random_descs(LONG_SIZES[-1], seed=82)
    d.setflags(write=False)
    return d


@pytest.mark.parametrize("nif", [1, 32])
@pytest.mark.parametrize("n", LONG_SIZES)
def test_device_equals_route_host_past_one_scan_trip(dev, long_descs, n, nif):
    """More than S tiles: route_scan_counts takes a second (and third, partial)
    trip of its loop, so the later tiles' prefixes carry the earlier trips'
    totals, block_incl_scan reuses its LDS words and the header's counts are
    sums over trips.  tile-then-none: a bin whose later trips are all zero;
    late-only: interface 0's prefixes are nothing but carry."""
    d = long_descs[:n]
    dd = _to_dev(d, dev)
    for pattern in RC.LONG_PATTERNS:
        v = RC.verdicts(pattern, n, nif, seed=n + nif, tile=T, trip=S)
        if pattern == "late-only":
            assert not (RC.bins_of(v[:S * T], nif) == 0).any() and v[S * T] == 0
        dv = _to_dev(v, dev)
        _same_as_host(DevRoute(dev, dd, dv, n, nif).result(), d, v, nif, f"{pattern} n={n} nif={nif}")


@pytest.mark.parametrize("n", LONG_SIZES)
def test_counts_on_the_device_past_one_scan_trip(dev, long_descs, n):
    """counts NULL: the header words of the workspace, each a carry over all
    trips.  (uniform: whichever bin the last tile's frames fall in has a carry.)"""
    d = long_descs[:n]
    v = RC.verdicts("uniform", n, 3, seed=n)
    r = DevRoute(dev, _to_dev(d, dev), _to_dev(v, dev), n, 3, sync=False)
    assert r.counts is None
    _same_as_host(r.result(), d, v, 3, f"counts NULL n={n}")


@pytest.mark.parametrize("nif", [1, 3, 32])
def test_without_order_and_without_counts(dev, descs, nif):
    """order NULL: the lists alone.  counts NULL: the call only enqueues, and the
    counts are the first words of the workspace once the stream is done."""
    n = 2 * T + 77
    d = descs[:n]
    v = RC.verdicts("stray", n, nif, seed=5)
    dd, dv = _to_dev(d, dev), _to_dev(v, dev)
    _same_as_host(DevRoute(dev, dd, dv, n, nif, order=False).result(), d, v, nif, "order NULL")
    r = DevRoute(dev, dd, dv, n, nif, sync=False)
    assert r.counts is None
    _same_as_host(r.result(), d, v, nif, "counts NULL")
    _same_as_host(DevRoute(dev, dd, dv, n, nif, order=False, sync=False).result(), d, v, nif, "both NULL")
    # a workspace longer than asked for, used twice
    ws = torch.empty(route.route_workspace(n, nif) + 4096, dtype=torch.uint8, device=dev)
    for pattern in ("uniform", "all-drop"):
        v2 = RC.verdicts(pattern, n, nif, seed=6)
        _same_as_host(DevRoute(dev, dd, _to_dev(v2, dev), n, nif, ws=ws).result(), d, v2, nif, "reused workspace")


def test_inputs_are_only_read(dev, descs):
    n = 3 * T + 5
    d = descs[:n]
    v = RC.verdicts("stray", n, 3, seed=8)
    dd, dv = _to_dev(d, dev), _to_dev(v, dev)
    DevRoute(dev, dd, dv, n, 3).result()
    assert np.array_equal(dd.cpu().numpy(), np.ascontiguousarray(d).view(np.uint8))
    assert np.array_equal(dv.cpu().numpy(), v.view(np.uint8))


def test_other_streams_and_two_routes_at_once(dev, descs):
    """On a stream of its own, and two routes of different batches enqueued on
    two streams before either is waited for: each as when run alone."""
    na, nb_ = 5 * T + 3, 4 * T + 61
    da, db = descs[:na], descs[1000:1000 + nb_]
    va, vb = RC.verdicts("uniform", na, 3, seed=21), RC.verdicts("cycle", nb_, 32, seed=22)
    dda, dva, ddb, dvb = _to_dev(da, dev), _to_dev(va, dev), _to_dev(db, dev), _to_dev(vb, dev)
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        alone = DevRoute(dev, dda, dva, na, 3)
    _same_as_host(alone.result(), da, va, 3, "own stream")
    with torch.cuda.stream(s1):
        ra = DevRoute(dev, dda, dva, na, 3, sync=False)
    with torch.cuda.stream(s2):
        rb = DevRoute(dev, ddb, dvb, nb_, 32, sync=False)
    assert ra.stream.cuda_stream != rb.stream.cuda_stream
    _same_as_host(ra.result(), da, va, 3, "stream 1 of 2")
    _same_as_host(rb.result(), db, vb, 32, "stream 2 of 2")


def test_the_tensor_form(dev, descs):
    n = T + 9
    d = descs[:n]
    v = RC.verdicts("uniform", n, 2, seed=31)
    dd = torch.from_numpy(np.ascontiguousarray(d).view(np.int64).reshape(-1, 2).copy()).to(dev)
    dv = torch.from_numpy(v).to(dev)
    wtx, wfill, word, wcounts = RC.model(d, v, 2)
    tx, fill, od, counts = route.route_batch(dd, dv, 2, order=True)
    assert counts == wcounts and tx.shape == (n, 2) and od.dtype == torch.int32
    assert np.array_equal(tx.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)[:wtx.size], wtx)
    assert np.array_equal(fill.cpu().numpy().view(np.uint64)[:wfill.size], wfill)
    assert np.array_equal(od.cpu().numpy().view(np.uint32), word)
    assert route.route_batch(dd, dv, 2)[2] is None
    e = route.route_batch(dd[:0], dv[:0], 2, order=True)
    assert e[3] == [0, 0, 0] and e[0].shape == (0, 2)
    with pytest.raises(ValueError):
        route.route_batch(dd.cpu(), dv, 2)
    with pytest.raises(_lib.XsknfGpuError):
        route.route_batch(dd, dv, 33)


@pytest.fixture(scope="module")
def imix():
    """The 300,001-frame IMIX batch with 5 % edge cases.  Shared, never written."""
    b = frames.unaligned_batch(300001, "imix", seed=91)
    frames.inject_edge_cases(b, 0.05, seed=92)
    b.umem.setflags(write=False)
    b.descs.setflags(write=False)
    return b


@pytest.mark.parametrize("action,nif,ingress,want", [
    (ACTION_REDIRECT, 3, 1, {-1: 3784, 0: 3334, 2: 292883}),
    (ACTION_DROP, 1, 0, None),
], ids=["redirect-3if", "drop-1if"])
def test_from_the_hot_path(dev, imix, action, nif, ingress, want):
    """Checksummer.process_batch, then Checksummer.route on what it left: the
    lists are the model's over the REFERENCE's verdicts for the batch."""
    oracles.require()
    ref = imix.umem.copy()
    rv = R.process_batch(ref, imix.descs, ingress=ingress, iters=1, action=action, nif=nif)
    if want is not None:
        vals, cnt = np.unique(rv, return_counts=True)
        assert dict(zip((int(x) for x in vals), (int(c) for c in cnt))) == want
    wtx, wfill, word, wcounts = RC.model(imix.descs, rv, nif)
    assert all(wcounts[k] > 0 for k in ((0, 2, 3) if nif == 3 else (0, 1)))
    cs = Checksummer(ChecksummerOptions(action=action), num_interfaces=nif, frame_len_hint=1500)
    umem = torch.from_numpy(imix.umem.copy()).to(dev)
    dd = torch.from_numpy(imix.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    v = cs.process_batch(umem, dd, ingress_ifindex=ingress)
    tx, fill, od, counts = cs.route(dd, v, order=True)
    assert counts == wcounts
    assert np.array_equal(tx.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)[:wtx.size], wtx)
    assert np.array_equal(fill.cpu().numpy().view(np.uint64)[:wfill.size], wfill)
    assert np.array_equal(od.cpu().numpy().view(np.uint32), word)
    assert np.array_equal(v.cpu().numpy(), rv) and np.array_equal(umem.cpu().numpy(), ref)


def test_after_the_multi_device_round_trip(dev):
    """scatter_dev (packed) over every visible device, _return to the root, then
    the root's verdicts routed there: the model's lists over the reference's
    verdicts for the whole batch."""
    oracles.require()
    b = frames.unaligned_batch(20000, "imix", seed=91)
    frames.inject_edge_cases(b, 0.1, seed=92)
    n, nif, ingress = int(b.descs.shape[0]), 3, 1
    ref = b.umem.copy()
    rv = R.process_batch(ref, b.descs, ingress=ingress, iters=1, action=ACTION_REDIRECT, nif=nif)
    ndev = torch.cuda.device_count()
    big = torch.zeros(b.umem.size + 64, dtype=torch.uint8, device=dev)   # (the packing reads whole 16-byte chunks)
    umem = big[:b.umem.size]
    umem.copy_(torch.from_numpy(b.umem))
    dd = torch.from_numpy(b.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    v = torch.full((n,), 0x7eadbeef, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with multi.MultiDevice(range(ndev)) as m:
        m.scatter_dev(0, umem.data_ptr(), b.umem.size, dd.data_ptr(), n, packed=True)
        m.return_results(umem.data_ptr(), v.data_ptr(), ChecksummerOptions(), num_interfaces=nif,
                         ingress_ifindex=ingress, frame_len_max=int(b.descs["len"].max()))
        torch.cuda.synchronize(dev)
        got = DevRoute(dev, dd, v, n, nif).result()
    assert np.array_equal(v.cpu().numpy(), rv)
    RC.same_as(got, RC.model(b.descs, rv, nif), n, "after _return")
    assert all(c > 0 for c in (got[3][0], got[3][2], got[3][3]))


def _run_tool(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def test_c_host_tool_routes_the_round_trip(dev, clean_ctx):
    """tools/multi_config4 --route: the root's verdicts routed from C after the
    packed round trip, every count and list entry against xsknf_gpu_route_host
    over the oracle's verdicts.  (Run from the forkserver, never from this
    GPU-initialised process.)"""
    tool = os.path.join(ROOT, "tools", "build", "multi_config4")
    if not os.path.exists(tool):
        pytest.fail(f"{tool} is not built (make tools)")
    with clean_ctx.Pool(1) as pool:
        rc, out, err = pool.apply(_run_tool, ([tool, "4096", "--route"], 300))
    assert rc == 0, (out, err[-2000:])
    r = json.loads(out.strip().splitlines()[-1])
    assert r["frames"] == 4096 and r["route_match"] is True and r["route_ms"] > 0
    assert r["counters_match"] and r["root_umem_match"] and r["verdicts_match"]
