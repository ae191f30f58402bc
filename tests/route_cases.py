"""What tests/test_route.py (CPU) and tests/test_gpu_route.py share: an
independent numpy model of the routing (include/xsknf_gpu.h, "routing a
checksummed batch"), the verdict patterns, random descriptors and the comparison
of a result with the model -- sentinels past the totals included.  Also the
constants the long-batch tests read from the kernels' sources (the router's and
the planner's scans share block_scan.h, so tests/test_gpu_plan_dev.py and
tests/test_plan_dev.py take them, and the planner's long descriptors, from here)."""
import ctypes
import os
import re

import numpy as np

from xsknf_amd import _lib, frames

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
SENTINEL8 = 0xA5                       # every output byte before a call
SENTINEL32 = 0xA5A5A5A5
SENTINEL64 = 0xA5A5A5A5A5A5A5A5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xsknf_amd", "csrc")


def code_match(header, pattern):
    """re.search(pattern) in xsknf_amd/csrc/<header>.  A pattern the code no
    longer holds is an error: a size taken from the code must move with the code
    or fail, never quietly become a stale number."""
    src = open(os.path.join(CSRC, header)).read()
    m = re.search(pattern, src)
    assert m, f"{header} no longer matches {pattern!r}: re-derive the test sizes that were read from it"
    return m


def code_constant(header, pattern):
    """The integer the one group of `pattern` names in xsknf_amd/csrc/<header>."""
    return int(code_match(header, pattern).group(1))


def scan_trip():
    """S: the tile counts one trip of the scan loops takes (route_scan_counts,
    plan_scan_totals): scan::kThreads of block_scan.h, which both kernel files
    pin to their own kThreads and step their scan loops by."""
    s = code_constant("block_scan.h", r"namespace scan \{\s*constexpr int kThreads = (\d+);")
    for header in ("kernel_route.h", "kernel_plan.h"):
        code_match(header, r"static_assert\(scan::kThreads == kThreads,")
        code_match(header, r"for \(uint64_t i0 = 0; i0 < nb; i0 \+= kThreads\) \{")
        assert code_constant(header, r"constexpr int kThreads = (\d+);") == s
    return s


def tile_of(header):
    """T: frames per block, kThreads * kPerThread of kernel_route.h / kernel_plan.h."""
    code_match(header, r"kTile = kThreads \* kPerThread;")
    return code_constant(header, r"constexpr int kThreads = (\d+);") * code_constant(
        header, r"constexpr int kPerThread = (\d+);")


def long_sizes(s, t):
    """The smallest batches past one scan trip: a second trip whose only tile
    holds one frame; three trips, the last partial, n no multiple of 64."""
    return [s * t + 1, 2 * s * t + 3 * t + 77]


def bins_of(verdicts, nif):
    """The bin of every frame: its interface, or nif for a drop."""
    v = np.asarray(verdicts).astype(np.int64)
    if nif == 1:
        return np.where(v == -1, 1, 0)
    return np.where((v < 0) | (v >= nif), nif, v)


def model(descs, verdicts, nif):
    """(tx_descs[:ntx], fill_addrs[:ndrop], order, counts): np.flatnonzero per
    bin, concatenated."""
    b = bins_of(verdicts, nif)
    idx = [np.flatnonzero(b == k) for k in range(nif + 1)]
    txi = np.concatenate(idx[:nif]) if nif else np.zeros(0, dtype=np.int64)
    tx = np.zeros(txi.size, dtype=frames.DESC_DTYPE)
    tx["addr"] = descs["addr"][txi]
    tx["len"] = descs["len"][txi]
    return tx, descs["addr"][idx[nif]].astype(np.uint64), np.concatenate(idx).astype(np.uint32), [i.size for i in idx]


def random_descs(n, seed):
    """Descriptors with every bit in play: full 64-bit addresses, full 32-bit
    lengths, non-zero options (the lists carry options 0)."""
    rng = np.random.default_rng(seed)
    d = np.zeros(n, dtype=frames.DESC_DTYPE)
    d["addr"] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    d["len"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    d["options"] = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return d


PATTERNS = ["all-drop", "all-one", "alternating", "one-absent", "long-runs", "uniform", "stray", "cycle",
            "tile-then-none"]
# for the batches past one scan trip: tile-then-none leaves a bin empty in every
# tile of the later trips, late-only one whose tile prefixes are all carry
LONG_PATTERNS = ["uniform", "cycle", "tile-then-none", "late-only"]
PLAN_LENS = [0, 1, 64, 570, 1500, 17, 128]


def plan_descs(n):
    """(n descriptors, UMEM size) for the planner's long batches, with no UMEM
    bytes behind them (the planner reads addresses and lengths alone): the
    lengths of PLAN_LENS in turn, frame f + 1 starting f % 16 bytes after frame
    f's end (7 lengths against 16 gaps: the starts step through every address
    mod 16 against every length), every other address as base | offset << 48,
    options all different."""
    f = np.arange(n, dtype=np.uint64)
    ln = np.array(PLAN_LENS, dtype=np.uint64)[f % np.uint64(len(PLAN_LENS))]
    step = ln + f % np.uint64(16)
    start = np.cumsum(step, dtype=np.uint64) - step + np.uint64(3)
    delta = np.where((f % np.uint64(2) == 1) & (start >= 300), np.uint64(256) + f % np.uint64(7), np.uint64(0))
    d = np.zeros(n, dtype=frames.DESC_DTYPE)
    d["addr"] = (start - delta) | (delta << np.uint64(48))
    d["len"] = ln.astype(np.uint32)
    d["options"] = (f * np.uint64(2654435761) + np.uint64(1)).astype(np.uint32)
    return d, (int((start + ln).max()) + 15 & ~15) if n else 16


def verdicts(pattern, n, nif, seed=7, tile=2048, trip=256):
    """n int32 verdicts.  cycle: -1, 0 .. nif-1 in turn (nif = 32: every run of
    64 frames holds all 33 bins).  tile-then-none: interface 0 for one tile,
    then no frame of it.  late-only: no frame of interface 0 in the first `trip`
    tiles, then every third frame (the first of them included)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if pattern == "all-drop":
        v = np.full(n, -1)
    elif pattern == "all-one":
        v = np.full(n, nif - 1)
    elif pattern == "alternating":
        v = np.where(i % 2 == 0, -1, nif - 1)
    elif pattern == "one-absent":          # no frame for interface 0 (one interface: no drop)
        v = rng.integers(1, nif, n) if nif > 1 else np.zeros(n, dtype=np.int64)
        if nif > 1:
            v[rng.random(n) < 0.3] = -1
    elif pattern == "long-runs":           # runs of 5000 frames of one bin (longer than 4096, than a tile)
        v = (i // 5000) % (nif + 1) - 1
    elif pattern == "uniform":
        v = rng.integers(-1, nif, n)
    elif pattern == "stray":
        v = rng.integers(-1, nif, n)
        strays = np.array([nif, nif + 1, -2, INT32_MIN, INT32_MAX, 0x40000000, 0x40000000 | 0x4A1234,
                           0x40000000 | (nif - 1)], dtype=np.int64)
        at = rng.random(n) < 0.25
        v[at] = strays[rng.integers(0, strays.size, int(at.sum()))]
    elif pattern == "cycle":
        v = i % (nif + 1) - 1
    elif pattern == "tile-then-none":
        v = np.where(i < tile, 0, np.where(i % 3 == 0, -1, nif - 1 if nif > 1 else -1))
    elif pattern == "late-only":
        v = rng.integers(0, nif, n)        # the other bins, the drops among them, everywhere
        v[v == 0] = -1
        late = trip * tile
        v[late::3] = 0
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(v.astype(np.int32))


def host_route_raw(descs, v, nif, order=True):
    """xsknf_gpu_route_host into sentinel-filled buffers of n entries."""
    n = int(descs.shape[0])
    tx = np.full(n * 16, SENTINEL8, dtype=np.uint8).view(frames.DESC_DTYPE)
    fill = np.full(n, SENTINEL64, dtype=np.uint64)
    od = np.full(n, SENTINEL32, dtype=np.uint32) if order else None
    counts = np.full(nif + 1, SENTINEL64, dtype=np.uint64)
    d = np.ascontiguousarray(descs)
    rc = _lib.load().xsknf_gpu_route_host(d.ctypes.data if n else None, v.ctypes.data if n else None, n, nif,
                                          tx.ctypes.data if n else None, fill.ctypes.data if n else None,
                                          od.ctypes.data if order and n else None, counts.ctypes.data)
    assert rc == 0, rc
    return tx, fill, od, [int(c) for c in counts]


def same_as(got, want, n, what=""):
    """`got` = (tx_descs, fill_addrs, order or None, counts) over sentinel-filled
    buffers of n entries; `want` = model()'s.  Every field of every entry up to
    the totals, the sentinels past them."""
    tx, fill, od, counts = got
    wtx, wfill, word, wcounts = want
    assert list(counts) == list(wcounts), what
    ntx, ndrop = int(wtx.shape[0]), int(wfill.shape[0])
    assert ntx + ndrop == n and sum(wcounts) == n
    for field in ("addr", "len", "options"):
        bad = np.nonzero(tx[field][:ntx] != wtx[field])[0]
        assert bad.size == 0, f"{what}: tx_descs.{field} differs at {bad[:8]}"
    assert np.array_equal(fill[:ndrop], wfill), f"{what}: fill_addrs"
    assert np.all(tx[ntx:].view(np.uint8) == SENTINEL8), f"{what}: tx_descs written past ntx"
    assert np.all(fill[ndrop:] == np.uint64(SENTINEL64)), f"{what}: fill_addrs written past the drops"
    if od is not None:
        assert np.array_equal(od, word), f"{what}: order"
        assert np.array_equal(np.sort(od), np.arange(n, dtype=np.uint32)), f"{what}: order is no permutation"
