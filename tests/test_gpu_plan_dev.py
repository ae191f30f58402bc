"""The multi-device plan computed on the root GPU (include/xsknf_gpu.h
xsknf_gpu_shard_plan_dev, xsknf_gpu_multi_scatter_dev; xsknf_amd/csrc/plan_device.hip).

* The planner against the host functions it restates -- xsknf_gpu_shard_plan,
  _shard_rebase and _shard_pack_plan on the same descriptors: every cut, span /
  size, byte sum and every field of every output descriptor, for equality;
  among the sizes, batches past one and two trips of the scan over the tile
  totals (S tiles a trip, read from the code).
* xsknf_gpu_multi_scatter_dev against the host scatters on the same object and
  batch (every shard's info, bytes and descriptors equal), then the results
  against the reference's pass over the whole batch.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import oracles
from tests import route_cases as RC
from xsknf_amd import _lib, frames, multi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = np.uint64(1 << 40)          # added to an address: outside any UMEM here
UMEM_ADDR = 0x7F5A12340000        # a 16-byte aligned root address for the packed layout's address mod 16


def _tile() -> int:
    """Frames per block of the planner's scan, from the code: the workspace
    holds one prefix per tile and scan, so it first grows at n = T + 1."""
    w1 = multi.plan_dev_workspace(1)
    lo, hi = 1, 2
    while multi.plan_dev_workspace(hi) == w1:
        lo, hi = hi, hi * 2
    while hi - lo > 1:            # workspace(lo) == w1 < workspace(hi)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if multi.plan_dev_workspace(mid) == w1 else (lo, mid)
    return lo


T = _tile()
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 300001]
SHARDS = [1, 2, 3, 8, 64]
S = RC.scan_trip()                # block totals per trip of plan_scan_totals' loop
LONG_SIZES = RC.long_sizes(S, T)  # two trips, the second of one frame; three trips, the last partial


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def imix():
    """300,001 IMIX frames packed back to back at odd starts (addr = base |
    offset << 48): (descriptors, UMEM size).  Shared, never written."""
    b = frames.unaligned_batch(SIZES[-1], "imix", seed=81)
    b.descs.setflags(write=False)
    return b.descs, int(b.umem.size)


def _to_dev(descs, dev):
    return torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8).reshape(-1, 16).copy()).to(dev)


def _from_dev(t):
    return t.cpu().numpy().view(frames.DESC_DTYPE).reshape(-1)


def _same_descs(got, want, what):
    for field in ("addr", "len", "options"):
        bad = np.nonzero(got[field] != want[field])[0]
        assert bad.size == 0, f"{what}: {field} differs at {bad[:8]}: {got[field][bad[:8]]} != {want[field][bad[:8]]}"


def check_plan(dev, descs, nshards, umem_size, umem_addr=UMEM_ADDR):
    """Both modes of the device planner on `descs` against the host functions."""
    n = int(descs.shape[0])
    dd = _to_dev(descs, dev)
    ranges, spans = multi.shard_plan(descs, nshards, umem_size)
    sums = [int(descs["len"][lo:hi].astype(np.uint64).sum(dtype=np.uint64)) for lo, hi in ranges]

    g_ranges, g_spans, g_sums, out = multi.shard_plan_dev(dd.data_ptr(), n, nshards, umem_addr, umem_size,
                                                          _lib.PLAN_SPAN, device=dev)
    assert g_ranges == ranges
    assert g_spans == spans
    assert g_sums == sums
    want = np.zeros(n, dtype=frames.DESC_DTYPE)
    for (lo, hi), (b0, _) in zip(ranges, spans):
        want[lo:hi] = multi.shard_rebase(descs[lo:hi], b0, umem_size)
    _same_descs(_from_dev(out), want, "rebased")

    bounds = [0] + [hi for _, hi in ranges]
    want, sizes = multi.pack_plan(descs, bounds, umem_addr, umem_size)
    g_ranges, g_sizes, g_sums, out = multi.shard_plan_dev(dd.data_ptr(), n, nshards, umem_addr, umem_size,
                                                          _lib.PLAN_PACKED, device=dev)
    assert g_ranges == ranges
    assert g_sizes == sizes
    assert g_sums == sums
    _same_descs(_from_dev(out), want, "packed")
    return ranges, spans, sizes


def test_tile_is_read_from_the_code():
    src = open(os.path.join(ROOT, "xsknf_amd", "csrc", "kernel_plan.h")).read()
    import re
    threads = int(re.search(r"kThreads = (\d+);", src).group(1))
    per = int(re.search(r"kPerThread = (\d+);", src).group(1))
    assert T == threads * per


@pytest.mark.parametrize("nshards", SHARDS)
@pytest.mark.parametrize("n", SIZES)
def test_planner_sizes(dev, imix, n, nshards):
    """Every size around the wave, the tile and several tiles, times every shard
    count (more shards than frames included): IMIX at odd starts."""
    descs, size = imix
    check_plan(dev, descs[:n].copy(), nshards, size)


def _mix(name, imix):
    descs, size = imix
    if name == "aligned-imix":
        b = frames.aligned_batch(2 * T + 1, "imix", seed=82)
        return b.descs, int(b.umem.size)
    if name == "all-64":
        d = np.zeros(3 * T + 5, dtype=frames.DESC_DTYPE)
        d["addr"] = np.arange(d.size, dtype=np.uint64) * np.uint64(2048) + np.uint64(256)
        d["len"] = 64
        return d, d.size * 2048
    if name == "eight-100":       # 4 shards: the running sum hits 200, 400, 600 exactly
        d = np.zeros(8, dtype=frames.DESC_DTYPE)
        d["addr"] = np.arange(8, dtype=np.uint64) * np.uint64(128) + np.uint64(3)
        d["len"] = 100
        return d, 1024
    if name == "tile-boundary":   # T * 6 equal frames: cuts of 2, 3 and 6 shards fall on tile boundaries
        d = np.zeros(6 * T, dtype=frames.DESC_DTYPE)
        d["addr"] = np.arange(d.size, dtype=np.uint64) * np.uint64(96) + np.uint64(5)
        d["len"] = 90
        return d, d.size * 96
    if name == "zero-sprinkled":
        d = descs[:2 * T + 77].copy()
        d["len"][::5] = 0
        d["len"][T - 1:T + 2] = 0
        return d, size
    if name == "all-zero":        # a target of 0: every cut is 1
        d = descs[:T + 9].copy()
        d["len"] = 0
        return d, size
    if name == "every-37th-out":
        d = descs[:3 * T + 11].copy()
        d["addr"][::37] += OUT
        return d, size
    if name == "huge-lens":       # five lengths near 2^32: outside the UMEM, inside the total (past 2^32)
        d = descs[:5000].copy()
        d["len"][[0, 999, 2048, 2049, 4999]] = 0xFFFFFFF0
        return d, size
    raise ValueError(name)


MIXES = ["aligned-imix", "all-64", "eight-100", "tile-boundary", "zero-sprinkled", "all-zero", "every-37th-out",
         "huge-lens"]


# ---- past one trip of plan_scan_totals' loop (more than S tiles) ----

def test_scan_trip_is_read_from_the_code():
    assert S == RC.code_constant("block_scan.h", r"constexpr int kThreads = (\d+);")
    assert T == RC.tile_of("kernel_plan.h")
    assert [-(-n // T) for n in LONG_SIZES] == [S + 1, 2 * S + 4]


@pytest.fixture(scope="module")
def long_plan():
    """RC.plan_descs at the larger long size: (descriptors, UMEM size).  In
    every scan trip every address mod 16 meets every length.  Shared, never
    written."""
    d, size = RC.plan_descs(LONG_SIZES[-1])
    off = (d["addr"] & np.uint64((1 << 48) - 1)) + (d["addr"] >> np.uint64(48))
    for lo in (0, S * T, 2 * S * T):
        seen = set(zip((off[lo:lo + 4096] % np.uint64(16)).tolist(), d["len"][lo:lo + 4096].tolist()))
        assert seen == {(r, ln) for r in range(16) for ln in RC.PLAN_LENS}
    assert (d["addr"][1::2][200:] >> np.uint64(48)).all() and not (d["addr"][::2] >> np.uint64(48)).any()
    d.setflags(write=False)
    return d, size


@pytest.mark.parametrize("nshards", [1, 3, 64])
@pytest.mark.parametrize("n", LONG_SIZES)
def test_planner_past_one_scan_trip(dev, long_plan, n, nshards):
    """More than S tiles: plan_scan_totals carries the first trips' bytes and
    slot bytes into the later tiles' prefixes, its binary search runs over more
    than S entries, and plan_cuts / plan_pack read carry-ins a later trip wrote."""
    descs, size = long_plan
    ranges, _, _ = check_plan(dev, descs[:n].copy(), nshards, size)
    if nshards == 64 and n == LONG_SIZES[-1]:
        # cuts in both whole trips (the third, of 4 tiles, holds the batch's end: its carry is the total)
        assert {hi // T // S for _, hi in ranges} == {0, 1, 2} and ranges[-2][1] // T // S == 1


def _long_mix(name, long_plan):
    descs, size = long_plan
    if name == "trip-boundary":   # 2 * S * T equal frames: cuts on the boundary between the trips and on tile boundaries inside them
        d = np.zeros(2 * S * T, dtype=frames.DESC_DTYPE)
        d["addr"] = np.arange(d.size, dtype=np.uint64) * np.uint64(96) + np.uint64(5)
        d["len"] = 90
        return d, d.size * 96
    if name == "first-trip-empty":   # all the bytes, and every cut, lie in later trips
        d = descs.copy()
        d["len"][:S * T] = 0
        return d, size
    if name == "every-37th-out":     # the slot prefix carries across the trips apart from the length prefix
        d = descs.copy()
        d["addr"][::37] += OUT
        return d, size
    raise ValueError(name)


@pytest.mark.parametrize("mix,nshards", [("trip-boundary", 2), ("trip-boundary", 4), ("first-trip-empty", 3),
                                         ("first-trip-empty", 64), ("every-37th-out", 3), ("every-37th-out", 64)])
def test_planner_length_mixes_past_one_scan_trip(dev, long_plan, mix, nshards):
    descs, size = _long_mix(mix, long_plan)
    ranges, _, sizes = check_plan(dev, descs, nshards, size)
    if mix == "trip-boundary":
        assert [hi for _, hi in ranges] == [2 * S * T * (k + 1) // nshards for k in range(nshards)]
        assert ranges[nshards // 2][0] == S * T
    if mix == "first-trip-empty":
        assert all(lo > S * T for lo, _ in ranges[1:])
    if mix == "every-37th-out":
        out = np.zeros(descs.size, dtype=bool)
        out[::37] = True
        assert all(out[lo:hi].any() for lo, hi in ranges) and all(s > 0 for s in sizes)


@pytest.mark.parametrize("nshards", [1, 2, 3, 4, 8, 64])
@pytest.mark.parametrize("mix", MIXES)
def test_planner_length_mixes(dev, imix, mix, nshards):
    descs, size = _mix(mix, imix)
    ranges, _, _ = check_plan(dev, descs, nshards, size)
    if mix == "eight-100" and nshards == 4:
        assert ranges == [(0, 2), (2, 4), (4, 6), (6, 8)]
    if mix == "tile-boundary" and nshards in (2, 3):
        assert [hi for _, hi in ranges] == [6 * T * (k + 1) // nshards for k in range(nshards)]
    if mix == "all-zero" and nshards > 1:
        assert [lo for lo, _ in ranges] == [0] + [1] * (nshards - 1) and ranges[-1][1] == descs.size
    if mix == "huge-lens":
        assert int(descs["len"].astype(np.uint64).sum(dtype=np.uint64)) > 1 << 32


def test_planner_shard_wholly_outside_the_umem(dev):
    """4000 equal frames in 4 shards, the second shard's frames all outside the
    UMEM: its span is {0, 0} and its packed size 0; its frames still count."""
    d = np.zeros(4000, dtype=frames.DESC_DTYPE)
    d["addr"] = np.arange(4000, dtype=np.uint64) * np.uint64(2048) + np.uint64(256)
    d["len"] = 64
    d["addr"][1000:2000] += OUT
    ranges, spans, sizes = check_plan(dev, d, 4, 4000 * 2048)
    assert ranges == [(0, 1000), (1000, 2000), (2000, 3000), (3000, 4000)]
    assert spans[1] == (0, 0) and sizes[1] == 0 and spans[2][0] == 2000 * 2048 + 256


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_planner_umem_address_not_16_byte_aligned(dev, imix, shift):
    """The packed layout keeps each frame's ADDRESS mod 16, so the UMEM's own
    address mod 16 moves every slot."""
    descs, size = imix
    d = descs[:2 * T + 1].copy()
    d["addr"][::37] += OUT
    check_plan(dev, d, 3, size, umem_addr=UMEM_ADDR + shift)


@pytest.mark.slow
def test_planner_config4_shape(dev):
    """BASELINE config 4's shape: 8,388,608 IMIX frames, one per 2 KiB chunk, 8 shards."""
    n = 8 << 20
    rng = np.random.default_rng(83)
    d = np.zeros(n, dtype=frames.DESC_DTYPE)
    d["addr"] = np.arange(n, dtype=np.uint64) * np.uint64(frames.CHUNK) + np.uint64(frames.HEADROOM)
    d["len"] = frames.imix_lengths(n, rng)
    check_plan(dev, d, 8, n * frames.CHUNK)


# ---- the scatter planned on the device ----

def _batch(case):
    base_off = 0
    if case == "unaligned-edges":
        b = frames.unaligned_batch(20000, "imix", seed=91)
        frames.inject_edge_cases(b, 0.1, seed=92)
    elif case == "jumbo":
        b = frames.unaligned_batch(3000, 9000, seed=93)
    elif case == "out-of-range":
        b = frames.aligned_batch(5000, "imix", seed=94)
        b.descs["addr"][::37] += OUT
    elif case == "one-frame":
        b = frames.aligned_batch(1, 570, seed=95)
    elif case == "empty":
        b = frames.aligned_batch(1, 570, seed=96)
        b = frames.HostBatch(b.umem, b.descs[:0].copy(), b.layout)
    elif case == "odd-base-and-end":
        # packed frames from the UMEM's first byte to its last, the UMEM 7 bytes
        # into its allocation: the first and last 16-byte chunks reach outside it
        b = frames.unaligned_batch(3000, "imix", seed=97)
        a = b.descs["addr"]
        off = (a & np.uint64((1 << 48) - 1)) + (a >> np.uint64(48))
        b.descs["addr"] = off - off[0]
        end = int((b.descs["addr"] + b.descs["len"]).max())
        b = frames.HostBatch(b.umem[int(off[0]):int(off[0]) + end].copy(), b.descs, "aligned")
        base_off = 7
    else:
        raise ValueError(case)
    return b.umem, b.descs, base_off


def _shards(m, ndev):
    """Every shard's info (without its device pointers), bytes and descriptors."""
    got = []
    for k in range(ndev):
        info = m.shard_info(k)
        su, _, sd = m.fetch(k, descs=True)
        got.append(({key: info[key] for key in ("device", "flags", "frame_lo", "frame_hi", "span_lo", "span_hi",
                                                "frame_bytes")}, su, sd))
    return got


def _same_shards(got, want):
    assert len(got) == len(want)
    for k, ((gi, gu, gd), (wi, wu, wd)) in enumerate(zip(got, want)):
        assert gi == wi, f"shard {k} info"
        assert np.array_equal(gu, wu), f"shard {k} bytes"
        _same_descs(gd, wd, f"shard {k} descriptors")


def _scatter_dev_run(dev, case, packed, roots=(0,)):
    from xsknf_amd import ChecksummerOptions
    host, hd, base_off = _batch(case)
    n = int(hd.shape[0])
    ndev = torch.cuda.device_count()
    ref = host.copy()
    _, ov = oracles.time_batch(ref, hd)
    with multi.MultiDevice(range(ndev)) as m:
        for root in roots:
            rdev = torch.device("cuda", root)
            big = torch.zeros(host.size + base_off + 64, dtype=torch.uint8, device=rdev)
            umem = big[base_off:base_off + host.size]
            umem.copy_(torch.from_numpy(host))
            dd = _to_dev(hd, rdev)
            v = torch.full((max(n, 1),), 0x7eadbeef, dtype=torch.int32, device=rdev)
            torch.cuda.synchronize(rdev)
            if packed:
                m.scatter_packed(root, umem.data_ptr(), host.size, hd)
            else:
                m.scatter(root, umem.data_ptr(), host.size, hd)
            want = _shards(m, ndev)
            secs, plan_secs = m.scatter_dev(root, umem.data_ptr(), host.size, dd.data_ptr(), n, packed=packed)
            dd.zero_()            # the caller may reuse its descriptor buffer once the call returns
            torch.cuda.synchronize(rdev)
            if n:
                assert secs >= plan_secs > 0
            _same_shards(_shards(m, ndev), want)
            opts = ChecksummerOptions()
            lmax = int(hd["len"].max()) if n else 0
            if packed:
                m.return_results(umem.data_ptr(), v.data_ptr(), opts, frame_len_max=lmax)
                torch.cuda.synchronize(rdev)
                assert np.array_equal(v.cpu().numpy()[:n], ov), "verdicts"
                assert np.array_equal(umem.cpu().numpy(), ref), "root UMEM"
            else:
                m.process(opts, frame_len_max=lmax)
                assert m.counters() == multi.expected_counters(ref, hd, ov)
                for k in range(ndev):
                    info = m.shard_info(k)
                    su, sv = m.fetch(k)
                    assert np.array_equal(sv, ov[info["frame_lo"]:info["frame_hi"]]), f"shard {k} verdicts"
                    assert np.array_equal(su, ref[info["span_lo"]:info["span_hi"]]), f"shard {k} bytes"
            del big, umem, dd, v


CASES = ["unaligned-edges", "jumbo", "out-of-range", "one-frame", "empty", "odd-base-and-end"]


@pytest.mark.parametrize("packed", [False, True], ids=["span", "packed"])
@pytest.mark.parametrize("case", CASES)
def test_scatter_dev_equals_host_scatter_and_reference(dev, case, packed):
    """scatter_dev over every visible device leaves each shard exactly as the
    host scatter of the same batch on the same object does; the pass over the
    shards then gives the reference's verdicts and bytes over the whole batch."""
    _scatter_dev_run(dev, case, packed)


@pytest.mark.parametrize("packed", [False, True], ids=["span", "packed"])
def test_scatter_dev_from_the_last_device_and_after_a_root_change(dev, packed):
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("one device: no other root")
    _scatter_dev_run(dev, "unaligned-edges", packed, roots=(ndev - 1,))
    _scatter_dev_run(dev, "out-of-range", packed, roots=(0, ndev - 1, 0))


def _run_tool(cmd, timeout):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr


def test_c_host_tool_with_device_descriptors(dev, clean_ctx):
    """tools/multi_config4 --device-descs: both scatters through
    xsknf_gpu_multi_scatter_dev from C, its own checks against the CPU oracle.
    (Run from the forkserver, never from this GPU-initialised process.)"""
    tool = os.path.join(ROOT, "tools", "build", "multi_config4")
    if not os.path.exists(tool):
        pytest.fail(f"{tool} is not built (make tools)")
    with clean_ctx.Pool(1) as pool:
        rc, out, err = pool.apply(_run_tool, ([tool, "65537", "--device-descs"], 300))
    assert rc == 0, (out, err[-2000:])
    r = json.loads(out.strip().splitlines()[-1])
    assert r["frames"] == 65537 and r["device_descs"] is True
    assert r["counters_match"] and r["root_umem_match"] and r["verdicts_match"]
    assert r["plan_ms"] > 0 and r["span_scatter_ms"] >= r["span_plan_ms"] and r["packed_scatter_ms"] >= r["packed_plan_ms"]
