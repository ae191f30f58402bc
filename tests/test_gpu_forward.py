"""Forwarding routed frames into their tx interface's UMEM on the device
(include/xsknf_gpu.h xsknf_gpu_forward_frames; xsknf_amd/csrc/forward_device.hip,
kernel_forward.h).

* The device against xsknf_gpu_forward_host on the same arrays, for equality:
  every byte of every destination UMEM (the sentinels outside the frames
  included), the unchanged rx UMEM and the three stats.  (tests/test_forward.py
  holds forward_host to an independent model on the CPU.)  The lists come from a
  real xsknf_gpu_route_batch on the device.  Sizes: around the wave and the
  block, past one and two sweeps of the persistent grid (G read from the code),
  and a capacity below the tx total.
* From the hot path: process_batch, route, forward, against the reference's
  checksummed bytes.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import ref as R
from tests import forward_cases as FC
from tests import oracles
from tests import route_cases as RC
from xsknf_amd import Checksummer, ChecksummerOptions, frames, route
from xsknf_amd.checksummer import ACTION_REDIRECT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 257]      # 257: more than a 256-thread block's first tiles, the last wave partial
NIFS = [1, 3, 32]
PATTERNS = ["cycle", "one-absent", "all-drop"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def _descs(pairs):
    d = FC.aligned_descs(len(pairs))
    d["addr"] = np.array([a for a, _ in pairs], dtype=np.uint64)
    d["len"] = np.array([l for _, l in pairs], dtype=np.uint32)
    d["options"] = 7
    return d


class DevForward:
    """A routed batch forwarded on the device: xsknf_gpu_route_batch (enqueue
    only: its counts stay in the workspace) and xsknf_gpu_forward_frames, back to
    back on the current stream, into sentinel-filled destination UMEMs.
    dst_sizes[i]: bytes of interface i's own UMEM, None (NULL) or "rx".
    cap: the capacity the forward is told, where it is to be BELOW the tx total
    (the buffer still holds all n + extra entries, the routed lists whole).
    fill: the destinations' bytes before the call, one array per interface with
    a UMEM of its own (default: the sentinel everywhere)."""

    def __init__(self, dev, rx, d, v, dst_sizes, sync=True, extra=0, cap=None, fill=None):
        n, nif = int(d.shape[0]), len(dst_sizes)
        self.nif, self.n = nif, n
        self.rx = _to_dev(rx, dev)
        self.dd, self.dv = _to_dev(d, dev), _to_dev(v, dev)
        held = n + extra                 # entries past the tx total keep wild descriptors (0xA5...)
        self.tx = torch.full((max(held, 1) * 16,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        cap = held if cap is None else cap
        assert cap <= held
        self.fill = torch.full((max(n, 1) * 8,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        self.ws = torch.zeros(route.route_workspace(n, nif), dtype=torch.uint8, device=dev)
        self.dsts = [torch.full((s,), FC.SENTINEL8, dtype=torch.uint8, device=dev) if isinstance(s, int) else None
                     for s in dst_sizes]
        if fill is not None:
            for t, a in zip(self.dsts, fill):
                assert (t is None) == (a is None)
                if t is not None:
                    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.stats_dev = torch.full((3,), -1, dtype=torch.int64, device=dev)
        ptrs = [self.rx.data_ptr() if s == "rx" else (0 if t is None else t.data_ptr())
                for s, t in zip(dst_sizes, self.dsts)]
        sizes = [self.rx.numel() if s == "rx" else (0 if t is None else t.numel()) for s, t in zip(dst_sizes, self.dsts)]
        with torch.cuda.device(dev):
            self.stream = torch.cuda.current_stream(dev)
            s = self.stream.cuda_stream
            if n:
                route.route_batch_ptr(self.dd.data_ptr(), self.dv.data_ptr(), n, nif, self.tx.data_ptr(),
                                      self.fill.data_ptr(), 0, self.ws.data_ptr(), self.ws.numel(), s, sync=False)
            self.stats = route.forward_frames_ptr(self.rx.data_ptr(), self.rx.numel(), ptrs, sizes,
                                                  self.tx.data_ptr() if cap else 0, self.ws.data_ptr(), cap,
                                                  self.stats_dev.data_ptr() if cap else 0, s, sync=sync)

    def result(self):
        self.stream.synchronize()
        stats = self.stats
        if stats is None:
            stats = [int(x) for x in self.stats_dev.cpu().numpy()]
        return [None if t is None else t.cpu().numpy() for t in self.dsts], stats


def _same_as_host(fwd, rx, d, v, dst_sizes, what, cap=None):
    """The device's destinations and stats == xsknf_gpu_forward_host's over
    route_host's lists (cap: over the first `cap` entries of them); rx UMEM,
    descriptors and lists unchanged."""
    nif = len(dst_sizes)
    got, stats = fwd.result()
    tx, _, _, counts = route.route_host(d, v, nif)
    full = counts
    if cap is not None:
        counts = FC.clip_counts(counts, nif, cap)
    txa = FC.aligned_descs(tx.shape[0])
    txa[:] = tx
    rw = FC.aligned_u8(rx.size)
    rw[:] = rx
    want = [FC.aligned_u8(s, FC.SENTINEL8) if isinstance(s, int) else None for s in dst_sizes]
    wstats = route.forward_host(rw, [rw if s == "rx" else w for s, w in zip(dst_sizes, want)], txa, counts)
    assert stats == wstats, what
    FC.same_umems(got, want, what)
    assert np.array_equal(fwd.rx.cpu().numpy(), rx), f"{what}: the rx UMEM changed"
    ntx = sum(full[:nif])
    assert np.array_equal(fwd.tx.cpu().numpy()[:16 * ntx].view(frames.DESC_DTYPE), tx[:ntx]), what
    assert np.all(fwd.tx.cpu().numpy()[16 * ntx:] == RC.SENTINEL8), what
    return stats


def _sizes(nif, size):
    """FC.umem_sizes with the rx UMEM itself as one interface's where there are enough."""
    s = FC.umem_sizes(nif, size)
    if nif > 3:
        s[3] = "rx"
    return s


@pytest.fixture(scope="module")
def batch():
    """257 frames of the 13 lengths in turn (a 9000-byte frame among 1-byte ones
    in every tile), every address mod 16, half of them unaligned-mode
    addresses, and their rx UMEM.  Shared, never written."""
    fr, size = FC.mixed_frames(SIZES[-1])
    rx = FC.rx_bytes(size, seed=41)
    return fr, rx


@pytest.mark.parametrize("nif", NIFS)
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_forward_host(dev, batch, n, nif):
    fr, rx = batch
    d = _descs(fr[:n])
    sizes = _sizes(nif, rx.size)
    for pattern in PATTERNS:
        v = RC.verdicts(pattern, n, nif, seed=n + nif)
        stats = _same_as_host(DevForward(dev, rx, d, v, sizes), rx, d, v, sizes, f"{pattern} n={n} nif={nif}")
        if pattern == "all-drop" or n == 0:
            assert stats == [0, 0, 0]
    if n == 257 and nif == 3:
        v = RC.verdicts("one-absent", n, nif, seed=n + nif)
        st = _same_as_host(DevForward(dev, rx, d, v, sizes), rx, d, v, sizes, "one-absent")
        assert st[0] > 0 and st[2] > 0           # the smaller UMEM's far frames skipped


def test_capacity_larger_than_the_total(dev, batch):
    """n is only the capacity: 100 entries past the routed batch, all wild
    (addr 0xA5A5..., len 0xA5A5A5A5), and the dropped frames' slots before them."""
    fr, rx = batch
    d = _descs(fr)
    for nif in (1, 3):
        v = RC.verdicts("cycle", len(fr), nif)
        sizes = [rx.size] * nif
        _same_as_host(DevForward(dev, rx, d, v, sizes, extra=100), rx, d, v, sizes, f"extra nif={nif}")


@pytest.mark.parametrize("cap", [200, 64])
def test_capacity_smaller_than_the_total(dev, batch, cap):
    """n below the tx total (257 entries in lists of 86, 86 and 85): the first
    `cap` entries alone are forwarded and counted -- 200 cuts interface 2's list
    inside a tile, 64 interface 0's -- and every byte of the frames of the
    entries at or past `cap` keeps its sentinel, although the lists behind the
    capacity hold real descriptors."""
    fr, rx = batch
    d = _descs(fr)
    n, nif = len(fr), 3
    v = (np.arange(n) % nif).astype(np.int32)
    tx, _, _, counts = route.route_host(d, v, nif)
    assert sum(counts[:nif]) == n > cap
    owner = np.repeat(np.arange(nif), counts[:nif])
    for sizes in (_sizes(nif, rx.size), [rx.size] * nif):
        fwd = DevForward(dev, rx, d, v, sizes, cap=cap)
        stats = _same_as_host(fwd, rx, d, v, sizes, f"cap={cap} {sizes}", cap=cap)
        own = np.array([isinstance(s, int) for s in sizes])[owner]
        assert stats[0] + stats[2] == int(own[:cap].sum()) and stats[0] > 0
        got, _ = fwd.result()
        for j in np.flatnonzero(own[cap:]) + cap:
            off, ln = FC.offset_of(tx["addr"][j]), int(tx["len"][j])
            assert np.all(got[owner[j]][off:off + ln] == FC.SENTINEL8), f"entry {j} >= cap {cap} was copied"


G = FC.grid_sweep()               # entries per sweep of forward_frames' grid
LONG_TOTALS = [G + 1, 2 * G + 64 * 5 + 3]


def test_grid_sweep_is_read_from_the_code():
    """G = kMaxBlocks * (kThreads / 64) * 64, the patterns FC.grid_sweep holds
    the code to, and the long totals: one entry, and 5 tiles and 3 entries, past
    whole sweeps."""
    blocks = RC.code_constant("kernel_forward.h", r"kMaxBlocks = (\d+);")
    threads = RC.code_constant("kernel_forward.h", r"constexpr int kThreads = (\d+);")
    assert G == blocks * (threads // 64) * 64
    assert LONG_TOTALS[0] == G + 1 and LONG_TOTALS[1] // G == 2 and LONG_TOTALS[1] % 64 == 3


@pytest.fixture(scope="module")
def packed():
    """FC.packed_frames at the larger long total and its rx UMEM (about 27 MB).
    Shared, never written."""
    d, size = FC.packed_frames(LONG_TOTALS[-1])
    d.setflags(write=False)
    return d, FC.rx_bytes(size, seed=44)


def _long_run(dev, packed, n, v, sizes, what):
    """The first n packed frames (a prefix of the rx UMEM holds them all: the
    UMEM is cut to it, so the smaller destination scales with the batch)."""
    d, rx = packed
    d = d[:n]
    end = int((FC.offsets_of(d["addr"]) + d["len"]).max()) + 64 & ~15
    return d, rx[:end], _same_as_host(DevForward(dev, rx[:end], d, v, sizes(end)), rx[:end], d, v, sizes(end), what)


@pytest.mark.parametrize("n", LONG_TOTALS)
def test_device_equals_forward_host_past_one_grid_sweep(dev, packed, n):
    """A tx total above G (and above 2 G): the grid is capped at kMaxBlocks and
    every wave takes a second (third) tile, rewriting its LDS rows, under a
    64-bit tile index.  No drops, 3 interfaces in turn: own and full-size,
    shared, own and smaller (its far frames skipped)."""
    nif = 3
    v = (np.arange(n) % nif).astype(np.int32)
    d, rx, stats = _long_run(dev, packed, n, v, lambda size: FC.umem_sizes(nif, size), f"n={n}")
    tx, _, _, counts = route.route_host(d, v, nif)
    assert sum(counts[:nif]) == n > (1 if n == LONG_TOTALS[0] else 2) * G
    assert stats[0] > 0 and stats[2] > 0 and stats[0] + stats[2] == counts[0] + counts[2]
    if n > 2 * G:
        assert counts[0] + counts[1] > G                          # interface 2's list lies wholly past G
        res, lens, live = FC.past_sweep(tx, counts, FC.umem_sizes(nif, rx.size), rx.size, G)
        assert res == set(range(16)) and lens == set(FC.PACKED_LENS) | {FC.PACKED_LONG} and live > 1000


def test_cycle_verdicts_past_one_grid_sweep(dev, packed):
    """Drops included (a quarter of the frames): the tx total still exceeds G.
    Interface 0 shares the rx UMEM; the two with a UMEM of their own (smaller,
    full-size) hold every entry past G."""
    n, nif = LONG_TOTALS[-1], 3
    v = RC.verdicts("cycle", n, nif)
    d, rx, stats = _long_run(dev, packed, n, v, lambda size: [None, FC.umem_sizes(nif, size)[2], size], "cycle")
    tx, _, _, counts = route.route_host(d, v, nif)
    assert G < sum(counts[:nif]) < n and counts[0] < G < counts[0] + counts[1] + counts[2]
    res, lens, live = FC.past_sweep(tx, counts, [None, FC.umem_sizes(nif, rx.size)[2], rx.size], rx.size, G)
    assert res == set(range(16)) and lens == set(FC.PACKED_LENS) | {FC.PACKED_LONG} and live > 1000
    assert stats[0] > 0 and stats[2] > 0


def test_a_tile_of_zero_lengths_and_all_to_one_interface(dev):
    n = 130
    d = _descs([(i * FC.CHUNK + i % 16, 0) for i in range(n)])
    rx = FC.rx_bytes(n * FC.CHUNK, seed=42)
    v = np.zeros(n, dtype=np.int32)
    assert _same_as_host(DevForward(dev, rx, d, v, [rx.size]), rx, d, v, [rx.size], "zero lengths") == [n, 0, 0]
    fr, size = FC.mixed_frames(200)
    rx = FC.rx_bytes(size, seed=43)
    d = _descs(fr)
    v = np.full(200, 1, dtype=np.int32)
    st = _same_as_host(DevForward(dev, rx, d, v, [None, size]), rx, d, v, [None, size], "all to one")
    assert st == [200, sum(l for _, l in fr), 0]
    assert _same_as_host(DevForward(dev, rx, d, v, [size, None]), rx, d, v, [size, None], "all shared") == [0, 0, 0]
    assert _same_as_host(DevForward(dev, rx, d, v, [size, "rx"]), rx, d, v, [size, "rx"], "all rx") == [0, 0, 0]


def test_edges_of_the_umems(dev):
    """As on the CPU: frames ending at the last byte, one byte past the end of
    the rx UMEM and of a smaller destination, a length of 0xFFFFFFFF, offsets
    past the end; the skipped frames' destination bytes keep their sentinels."""
    size, small = 8192, 4096
    rx = FC.rx_bytes(size, seed=3)
    per_if = [
        [(size - 100, 100), (size - 100, 101), (size - 1, 1), (size, 0), (size + 1, 0), (size, 1),
         (64, 0xFFFFFFFF), (1000, 3000), ((size - 300) | (200 << 48), 100), ((size - 300) | (201 << 48), 100)],
        [(small - 100, 100), (small - 100, 101), (small - 1, 1), (small, 0), (small, 1), (small + 16, 4),
         (5, 0xFFFFFFFF), (1 << 47, 1)],
    ]
    d = _descs(per_if[0] + per_if[1])
    v = np.array([0] * len(per_if[0]) + [1] * len(per_if[1]), dtype=np.int32)
    st = _same_as_host(DevForward(dev, rx, d, v, [size, small]), rx, d, v, [size, small], "edges")
    assert st == [5 + 3, (100 + 1 + 0 + 3000 + 100) + (100 + 1 + 0), 5 + 5]


def test_enqueue_only_on_another_stream(dev, batch):
    """stats NULL: route and forward enqueued back to back on a stream of their
    own with no host sync between; the stats are stats_dev's after one sync."""
    fr, rx = batch
    d = _descs(fr)
    v = RC.verdicts("cycle", len(fr), 3)
    sizes = _sizes(3, rx.size)
    torch.cuda.synchronize(dev)
    s1 = torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        f = DevForward(dev, rx, d, v, sizes, sync=False)
    assert f.stats is None and f.stream.cuda_stream == s1.cuda_stream
    assert f.stream.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    st = _same_as_host(f, rx, d, v, sizes, "enqueue only")
    assert st[0] > 0


def test_the_tensor_form(dev, batch):
    fr, rx = batch
    d = _descs(fr)
    v = RC.verdicts("cycle", len(fr), 2)
    dd = torch.from_numpy(d.view(np.int64).reshape(-1, 2).copy()).to(dev)
    tx, _, _, counts = route.route_batch(dd, torch.from_numpy(v).to(dev), 2)
    drx = torch.from_numpy(rx.copy()).to(dev)
    dst = torch.full((rx.size,), FC.SENTINEL8, dtype=torch.uint8, device=dev)
    stats = route.forward_frames(drx, [None, dst], tx, counts)
    htx, _, _, hcounts = route.route_host(d, v, 2)
    txa = FC.aligned_descs(htx.shape[0])
    txa[:] = htx
    want = FC.aligned_u8(rx.size, FC.SENTINEL8)
    assert stats == route.forward_host(rx, [None, want], txa, hcounts) and stats[0] == hcounts[1]
    assert np.array_equal(dst.cpu().numpy(), want)
    # the counts as a device tensor, and n as the capacity
    dst.fill_(FC.SENTINEL8)
    cdev = torch.tensor(counts, dtype=torch.int64).to(dev)
    assert route.forward_frames(drx, [None, dst], tx, cdev, n=tx.shape[0]) == stats
    assert np.array_equal(dst.cpu().numpy(), want)
    with pytest.raises(ValueError):
        route.forward_frames(drx.cpu(), [None, dst], tx, counts)
    with pytest.raises(ValueError):
        route.forward_frames(drx, [None, dst.cpu()], tx, counts)


def test_from_the_hot_path(dev):
    """Checksummer.process_batch, .route, .forward on a small IMIX batch, 3
    interfaces, ingress 1: every destination UMEM holds the REFERENCE's
    checksummed bytes at the tx frames of that interface and sentinels
    elsewhere."""
    oracles.require()
    nif, ingress = 3, 1
    b = frames.unaligned_batch(4096, "imix", seed=91)
    frames.inject_edge_cases(b, 0.05, seed=92)
    ref = b.umem.copy()
    rv = R.process_batch(ref, b.descs, ingress=ingress, iters=1, action=ACTION_REDIRECT, nif=nif)
    want = [np.full(ref.size, FC.SENTINEL8, dtype=np.uint8) for _ in range(nif)]
    nframes, nbytes = 0, 0
    for a, ln, x in zip(b.descs["addr"], b.descs["len"], rv):
        if 0 <= x < nif:
            off = FC.offset_of(a)
            want[x][off:off + int(ln)] = ref[off:off + int(ln)]
            nframes += 1
            nbytes += int(ln)
    assert sum(1 for k in range(nif) if (rv == k).any()) >= 2
    cs = Checksummer(ChecksummerOptions(action=ACTION_REDIRECT), num_interfaces=nif, frame_len_hint=1500)
    umem = torch.from_numpy(b.umem.copy()).to(dev)
    dd = torch.from_numpy(b.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    v = cs.process_batch(umem, dd, ingress_ifindex=ingress)
    tx, _, _, counts = cs.route(dd, v)
    dsts = [torch.full((ref.size,), FC.SENTINEL8, dtype=torch.uint8, device=dev) for _ in range(nif)]
    stats = cs.forward(umem, dsts, tx, counts)
    assert stats == [nframes, nbytes, 0]
    for k in range(nif):
        bad = np.flatnonzero(dsts[k].cpu().numpy() != want[k])
        assert bad.size == 0, f"interface {k}: differs at {bad[:8]}"
    assert np.array_equal(umem.cpu().numpy(), ref)


def _run_tool(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def test_c_host_tool_forwards_the_round_trip(dev, clean_ctx):
    """tools/multi_config4 --forward: the routed tx list forwarded from C into a
    second UMEM on the root, every byte and the stats against
    xsknf_gpu_forward_host.  (Run from the forkserver, never from this
    GPU-initialised process.)"""
    tool = os.path.join(ROOT, "tools", "build", "multi_config4")
    if not os.path.exists(tool):
        pytest.fail(f"{tool} is not built (make tools)")
    with clean_ctx.Pool(1) as pool:
        rc, out, err = pool.apply(_run_tool, ([tool, "4096", "--forward", "--device-descs"], 300))
    assert rc == 0, (out, err[-2000:])
    r = json.loads(out.strip().splitlines()[-1])
    assert r["frames"] == 4096 and r["forward_match"] is True and r["forward_ms"] > 0
    assert r["route_match"] is True and r["root_umem_match"] and r["verdicts_match"]
