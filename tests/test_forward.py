"""Forwarding routed frames into their tx interface's UMEM (include/xsknf_gpu.h
xsknf_gpu_forward_*), without a GPU: the exported names, the argument checks of
both calls (forward_frames' return before any HIP call), and
xsknf_gpu_forward_host -- the model the device forward is held to -- against an
independent numpy model over whole destination UMEMs, against the reference's
own lines (src/xsknf.c:563-571) walked in 64-frame ring batches, and under
AddressSanitizer + UBSan as a stand-alone program (tests/c/san_forward.c)."""
import ctypes
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import forward_cases as FC
from tests import route_cases as RC
from xsknf_amd import Checksummer, _lib, frames, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -errno.EINVAL
NIFS = [1, 2, 3, 32]


def test_names_are_exported_and_declared():
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "xsknf_gpu.h")).read()
    for name in ("xsknf_gpu_forward_frames", "xsknf_gpu_forward_host"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert f"XSKNF_GPU_API int {name}(" in src
    assert "#define XSKNF_GPU_FORWARD_STATS 3" in src
    assert route.FORWARD_STATS == 3
    assert hasattr(Checksummer, "forward")
    for f in ("forward_host", "forward_frames_ptr", "forward_frames"):
        assert callable(getattr(route, f))


def _call(device, **kw):
    """Either call with made-up, aligned pointers (never dereferenced: every
    case here returns before anything is read through them, and before a GPU
    call).  umems: (pointer, size) per interface."""
    a = dict(rx=0x100000, rx_size=0x10000, umems=[(0x200000, 0x10000), (None, 0), (0x300000, 0x8000)], nif=None,
             tx=0x400000, counts=0x500000, n=100, stats_dev=0x600000, null_umems=False, null_sizes=False)
    a.update(kw)
    nif = len(a["umems"]) if a["nif"] is None else a["nif"]
    k = max(len(a["umems"]), 1)
    ptrs = (ctypes.c_void_p * k)(*[p for p, _ in a["umems"]])
    sizes = (ctypes.c_uint64 * k)(*[s for _, s in a["umems"]])
    vp = ctypes.c_void_p
    lib = _lib.load()
    if device:
        return lib.xsknf_gpu_forward_frames(vp(a["rx"]), a["rx_size"], None if a["null_umems"] else ptrs,
                                            None if a["null_sizes"] else sizes, nif, vp(a["tx"]), vp(a["counts"]),
                                            a["n"], vp(a["stats_dev"]), None, None)
    return lib.xsknf_gpu_forward_host(vp(a["rx"]), a["rx_size"], None if a["null_umems"] else ptrs,
                                      None if a["null_sizes"] else sizes, nif, vp(a["tx"]), vp(a["counts"]), None)


BAD = [
    dict(nif=0), dict(nif=33), dict(umems=[(0x200000, 16)] * 33),
    dict(null_umems=True), dict(null_sizes=True),
    dict(rx=0x100008), dict(rx=0x100001),
    dict(umems=[(0x200008, 0x1000)]), dict(umems=[(None, 0), (0x200004, 0x1000)]),
    # a destination inside, across the start of, across the end of and around the rx UMEM
    dict(umems=[(0x100010, 0x100)]), dict(umems=[(0xff000, 0x1010)]), dict(umems=[(0x10fff0, 0x100)]),
    dict(umems=[(0xff000, 0x20000)]), dict(umems=[(0x100000, 0x10000), (0x100010, 0x10)]),
    # two destinations overlapping without being equal
    dict(umems=[(0x200000, 0x10000), (0x208000, 0x10000)]),
    dict(umems=[(0x200000, 0x10000), (None, 0), (0x1ff000, 0x1010)]),
    dict(umems=[(0x200000, 0x10000), (0x200010, 0x10)]),
    dict(tx=0x400008), dict(tx=0x400001), dict(counts=0x500004), dict(counts=0x500001),
    dict(tx=0x400008, n=0),
]
BAD_DEVICE = [dict(stats_dev=0x600004), dict(stats_dev=0x600001), dict(stats_dev=0x600004, n=0),
              dict(rx=None), dict(tx=None), dict(counts=None), dict(stats_dev=None)]


@pytest.mark.parametrize("bad", BAD + BAD_DEVICE, ids=str)
def test_forward_frames_refuses_before_any_gpu_call(bad):
    assert _call(True, **bad) == EINVAL


def _host_call(**kw):
    """xsknf_gpu_forward_host over real (tiny) arrays, so that a case the checks
    let through reads valid memory: one entry, two interfaces."""
    rx = FC.aligned_u8(256, 1)
    dst = FC.aligned_u8(256, FC.SENTINEL8)
    tx, counts = FC.lists([[(16, 8)], []])
    c = np.array(counts, dtype=np.uint64)
    a = dict(rx=rx.ctypes.data, rx_size=256, umems=[(dst.ctypes.data, 256), (None, 0)], tx=tx.ctypes.data,
             counts=c.ctypes.data)
    a.update(kw)
    return _call(False, **a), dst


@pytest.mark.parametrize("bad", BAD, ids=str)
def test_forward_host_refuses(bad):
    """The same cases over real lists and counts (the host form reads its
    counts to know how many entries there are); the UMEM pointers stay made up,
    and none is written or read."""
    bad = dict(bad)
    keep = []
    for k in ("tx", "counts"):           # misaligned by an offset into a real array
        if k in bad:
            keep.append(FC.aligned_u8(64, 0))
            bad[k] = keep[-1].ctypes.data + (bad[k] & 15)
    if "umems" in bad:
        bad.update(rx=0x100000, rx_size=0x10000)
    rc, dst = _host_call(**bad)
    assert rc == EINVAL and np.all(dst == FC.SENTINEL8)


def test_forward_host_null_arrays():
    rc, dst = _host_call()
    assert rc == 0 and np.all(dst[16:24] == 1) and np.all(dst[:16] == FC.SENTINEL8) and np.all(dst[24:] == FC.SENTINEL8)
    for k in ("rx", "tx"):
        rc, dst = _host_call(**{k: None})
        assert rc == EINVAL and np.all(dst == FC.SENTINEL8)
    # no entry: the arrays may be NULL, the stats are 0
    stats = np.full(3, 9, dtype=np.uint64)
    ptrs = (ctypes.c_void_p * 1)(None)
    sizes = (ctypes.c_uint64 * 1)(0)
    assert _lib.load().xsknf_gpu_forward_host(None, 0, ptrs, sizes, 1, None, None, stats.ctypes.data) == 0
    assert not stats.any()


def test_equal_destinations_and_empty_ranges_are_fine():
    # the same UMEM under two interfaces; a destination of 0 bytes inside the rx range; no entries (n == 0)
    assert _call(True, umems=[(0x200000, 0x1000), (0x200000, 0x1000)], n=0) == 0
    assert _call(True, umems=[(0x100010, 0)], n=0) == 0
    assert _call(True, umems=[(0x100000, 0x10000), (None, 0)], n=0) == 0      # the rx UMEM itself
    assert _call(True, rx=None, tx=None, counts=None, stats_dev=None, n=0) == 0
    assert route.forward_frames_ptr(0x100000, 4096, [0x200000], [4096], 0, 0, 0, 0) == [0, 0, 0]
    with pytest.raises(_lib.XsknfGpuError):
        route.forward_frames_ptr(0x100000, 4096, [0x200008], [4096], 0, 0, 0, 0)
    with pytest.raises(_lib.XsknfGpuError):
        route.forward_host(FC.aligned_u8(64, 0), [], FC.aligned_descs(0), [0])


def _host_vs_model(rx, dst_sizes, tx, counts, what, shared_rx=()):
    """forward_host into sentinel-filled arrays against the model: every byte of
    every destination, the stats, the rx UMEM and the lists unchanged.
    shared_rx: interfaces whose UMEM is the rx UMEM itself."""
    want, wstats = FC.model(rx, dst_sizes, tx, counts)
    got = FC.fresh(dst_sizes)
    rx_before, tx_before = rx.copy(), tx.copy()
    rw = FC.aligned_u8(rx.size)
    rw[:] = rx
    call = [rw if i in shared_rx else g for i, g in enumerate(got)]
    stats = route.forward_host(rw, call, tx, counts)
    assert stats == wstats, what
    FC.same_umems(got, want, what)
    assert np.array_equal(rw, rx_before) and np.array_equal(tx, tx_before), what
    return stats


@pytest.mark.parametrize("nif", NIFS)
def test_forward_host_equals_the_numpy_model(nif):
    """All 13 lengths at all 16 addresses mod 16, aligned- and unaligned-mode
    addresses, dealt to the interfaces; destinations own, shared (None), own
    and smaller (its far frames out of range)."""
    fr, size = FC.mixed_frames(13 * 16)
    assert {(FC.offset_of(a) % 16, l) for a, l in fr} >= {(r, l) for r in range(16) for l in FC.LENS}
    assert any(a >> 48 for a, _ in fr)
    rx = FC.rx_bytes(size, seed=nif)
    tx, counts = FC.lists(FC.deal(fr, nif))
    sizes = FC.umem_sizes(nif, size)
    stats = _host_vs_model(rx, sizes, tx, counts, f"nif={nif}")
    if nif >= 3:
        assert stats[2] > 0 and stats[0] > 0
    # the interface's UMEM is the rx UMEM: nothing copied, nothing counted, the rx UMEM unchanged
    sizes[0] = None
    again = _host_vs_model(rx, sizes, tx, counts, f"nif={nif}, 0 is rx", shared_rx=(0,))
    assert again[0] == stats[0] - counts[0] and again[2] == stats[2]       # (interface 0's frames were all in range)


def test_the_flat_model_is_the_model():
    """FC.model_flat, the model for the long lists, against FC.model's per-entry
    loop on the mixed frames and the UMEM edges, in blocks of 7 entries."""
    fr, size = FC.mixed_frames(13 * 16)
    rx = FC.rx_bytes(size, seed=9)
    edges = [(size - 100, 100), (size - 100, 101), (size, 0), (size + 1, 0), (64, 0xFFFFFFFF), (1 << 47, 1),
             ((size - 300) | (200 << 48), 100), ((size - 300) | (201 << 48), 100), ((1 << 64) - 1, 0xFFFFFFFF)]
    for nif in NIFS:
        tx, counts = FC.lists(FC.deal(fr + edges, nif))
        sizes = FC.umem_sizes(nif, size)
        want, wstats = FC.model(rx, sizes, tx, counts)
        for block in (7, 1 << 16):
            got, stats = FC.model_flat(rx, sizes, tx, counts, block=block)
            assert stats == wstats
            FC.same_umems(got, want, f"flat model nif={nif}")


def test_forward_host_equals_the_model_past_one_grid_sweep():
    """The largest batch the device forward is held to forward_host at
    (tests/test_gpu_forward.py: more than two sweeps of its grid), as routed
    there -- dealt to 3 interfaces in turn: own and full-size, shared, own and
    smaller -- and the conditions that batch must meet for the device test to
    mean what it says."""
    g = FC.grid_sweep()
    n = 2 * g + 64 * 5 + 3
    d, size = FC.packed_frames(n)
    off = FC.offsets_of(d["addr"])
    assert np.all(off[1:] >= off[:-1] + d["len"][:-1]) and int(off[-1]) + int(d["len"][-1]) <= size
    assert (off[1:] < off[:-1] + d["len"][:-1] + np.uint64(16)).all()             # neighbours share chunks
    assert (d["addr"][1::2][100:] >> np.uint64(48)).all() and not (d["addr"][::2] >> np.uint64(48)).any()
    rx = FC.rx_bytes(size, seed=44)
    sizes = FC.umem_sizes(3, size)
    assert sizes[0] == size and sizes[1] is None and sizes[2] < size
    v = (np.arange(n) % 3).astype(np.int32)
    tx, _, _, counts = route.route_host(d, v, 3)
    assert sum(counts[:3]) == n > 2 * g and counts[0] + counts[1] > g        # interface 2's list lies past G
    res, lens, live = FC.past_sweep(tx, counts, sizes, size, g)
    assert res == set(range(16)) and lens == set(FC.PACKED_LENS) | {FC.PACKED_LONG} and live > 1000
    txa = FC.aligned_descs(n)
    txa[:] = tx
    want, wstats = FC.model_flat(rx, sizes, txa, counts)
    got = FC.fresh(sizes)
    assert route.forward_host(rx, got, txa, counts) == wstats and wstats[0] > 0 and wstats[2] > 0
    FC.same_umems(got, want, "past one grid sweep")
    # the smaller batch: one entry past the sweep
    v1 = v[:g + 1]
    _, _, _, c1 = route.route_host(d[:g + 1], v1, 3)
    assert sum(c1[:3]) == g + 1
    # cycle verdicts (a quarter dropped) over the larger batch still fill more than one sweep
    vc = RC.verdicts("cycle", n, 3)
    txc, _, _, cc = route.route_host(d, vc, 3)
    assert g < sum(cc[:3]) < n
    res, lens, live = FC.past_sweep(txc, cc, [None, sizes[2], size], size, g)
    assert res == set(range(16)) and lens == set(FC.PACKED_LENS) | {FC.PACKED_LONG} and live > 1000


@pytest.mark.parametrize("cap", [0, 1, 64, 86, 87, 200, 256, 257, 300])
def test_clipped_counts_against_the_model(cap):
    """FC.clip_counts -- what a capacity below the tx total leaves of each
    interface's list (tests/test_gpu_forward.py) -- against a count of the
    first `cap` entries' owners; forward_host over the clipped counts is the
    model's over them, and the frames of the entries at or past `cap` keep their
    sentinels."""
    fr, size = FC.mixed_frames(257)
    rx = FC.rx_bytes(size, seed=41)
    tx, counts = FC.lists(FC.deal(fr, 3))
    owner = np.repeat(np.arange(3), counts[:3])
    clipped = FC.clip_counts(counts, 3, cap)
    assert clipped == [int((owner[:cap] == i).sum()) for i in range(3)] + [0]
    sizes = [size, None, size]
    stats = _host_vs_model(rx, sizes, tx, clipped, f"cap={cap}")
    assert stats[0] == int((owner[:cap] != 1).sum()) and stats[2] == 0
    got = FC.fresh(sizes)
    route.forward_host(rx, got, tx, clipped)
    for j in range(min(cap, 257), 257):
        if owner[j] != 1:
            off, ln = FC.offset_of(tx["addr"][j]), int(tx["len"][j])
            assert np.all(got[owner[j]][off:off + ln] == FC.SENTINEL8)


def test_edges_of_the_umems():
    """A frame ending at the last byte of both UMEMs; one byte past the end of
    the rx UMEM; one byte past the end of a smaller destination; a length of
    0xFFFFFFFF; an offset past the end; a 0-byte frame at the very end."""
    size, small = 8192, 4096
    rx = FC.rx_bytes(size, seed=3)
    per_if = [
        [(size - 100, 100), (size - 100, 101), (size - 1, 1), (size, 0), (size + 1, 0), (size, 1),
         (64, 0xFFFFFFFF), (0, size), ((size - 300) | (200 << 48), 100), ((size - 300) | (201 << 48), 100)],
        [(small - 100, 100), (small - 100, 101), (small - 1, 1), (small, 0), (small, 1), (small + 16, 4),
         (5, 0xFFFFFFFF), (1 << 47, 1)],
    ]
    tx, counts = FC.lists(per_if)
    stats = _host_vs_model(rx, [size, small], tx, counts, "edges")
    # interface 0: frames 1, 3, 4, 8 and 9 of 10 are in range; interface 1: frames 1, 3 and 4 of 8
    assert stats == [5 + 3, (100 + 1 + 0 + size + 100) + (100 + 1 + 0), 5 + 5]


def test_empty_lists():
    rx = FC.rx_bytes(4096, seed=4)
    for nif in NIFS:
        tx, counts = FC.lists([[] for _ in range(nif)])
        assert _host_vs_model(rx, [4096] * nif, tx, counts, "empty") == [0, 0, 0]
    # some lists empty, among them the first and the last
    fr, size = FC.mixed_frames(40)
    rx = FC.rx_bytes(size, seed=5)
    tx, counts = FC.lists([[], fr[:7], [], [], fr[7:], []])
    assert _host_vs_model(rx, [size] * 6, tx, counts, "some empty")[0] == 40


def test_the_references_rule_in_ring_batches():
    """64-frame ring batches, aligned-mode addresses (where `orig` is the offset):
    route_host, then forward_host, against src/xsknf.c:563-571 applied by hand --
    for every interface whose buffer is not the rx buffer, every frame of its
    to_tx[] list copied at its address."""
    nif, batch, nb = 3, 64, 5
    size = batch * nb * FC.CHUNK
    rx = FC.rx_bytes(size, seed=6)
    rng = np.random.default_rng(7)
    buffers = [np.full(size, FC.SENTINEL8, dtype=np.uint8), None, np.full(size, FC.SENTINEL8, dtype=np.uint8)]
    got = FC.fresh([size, None, size])
    for b in range(nb):
        d = FC.aligned_descs(batch)
        d["addr"] = (np.arange(batch, dtype=np.uint64) + np.uint64(b * batch)) * np.uint64(FC.CHUNK) + np.uint64(256)
        d["len"] = rng.choice([64, 570, 1500], batch).astype(np.uint32)
        v = RC.verdicts("uniform", batch, nif, seed=b)
        # the reference, by hand: to_tx[ret][ntx[ret]++] = {orig, len}, then the copy loop
        to_tx = [[(int(a), int(l)) for a, l, x in zip(d["addr"], d["len"], v) if x == i] for i in range(nif)]
        for i in range(nif):
            if buffers[i] is not None:                       # rx_xsk->buffer != xsks[i].buffer
                for addr, ln in to_tx[i]:
                    buffers[i][addr:addr + ln] = rx[addr:addr + ln]
        tx, _, _, counts = route.route_host(d, v, nif)
        txa = FC.aligned_descs(batch)
        txa[:] = tx
        stats = route.forward_host(rx, got, txa, counts)
        assert stats == [len(to_tx[0]) + len(to_tx[2]), sum(l for _, l in to_tx[0] + to_tx[2]), 0]
    FC.same_umems(got, buffers, "ring batches")


def test_forward_host_is_sanitizer_clean(tmp_path):
    """xsknf_amd/csrc/forward_host.cpp under AddressSanitizer + UBSan
    (tests/c/san_forward.c: a program of its own): heap UMEMs exactly as long
    as their last frame, so a byte past a frame's end is a heap overflow."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / "san_forward")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Iinclude", "-x", "c", "tests/c/san_forward.c", "-x", "c++",
                    "-std=c++17", "xsknf_amd/csrc/forward_host.cpp", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok 2000"
