"""Routing a checksummed batch (include/xsknf_gpu.h xsknf_gpu_route_*), without a
GPU: the exported names, the argument checks of all three calls (route_batch's
return before any HIP call), and xsknf_gpu_route_host -- the model the device
router is held to -- against an independent numpy model, against the runtime's
own dispose_1if / dispose_multi rule walked in 64-frame ring batches, end to end
behind the restatement oracle, and under AddressSanitizer + UBSan as a
stand-alone program (tests/c/san_route.c)."""
import ctypes
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import route_cases as RC
from xsknf_amd import Checksummer, _lib, frames, route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -errno.EINVAL
NIFS = [1, 2, 3, 32]


def test_names_are_exported_and_listed():
    lib = _lib.load()
    for name in ("xsknf_gpu_route_workspace", "xsknf_gpu_route_batch", "xsknf_gpu_route_host"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert route.MAX_INTERFACES == 32
    assert hasattr(Checksummer, "route")
    src = open(os.path.join(ROOT, "include", "xsknf_gpu.h")).read()
    assert "#define XSKNF_GPU_ROUTE_MAX_INTERFACES 32" in src


def test_workspace_is_positive_and_non_decreasing():
    for nif in NIFS:
        last = 0
        for n in [0, 1, 2, 64, 2047, 2048, 2049, 4096, 4097, 300001, 1 << 20, 8 << 20, (1 << 32) - 1]:
            w = route.route_workspace(n, nif)
            assert w > 0 and w % 8 == 0 and w >= last, (n, nif)
            last = w
        assert route.route_workspace(8 << 20, nif) >= 8 * (nif + 1)      # the counts, at least
    assert route.route_workspace(8 << 20, 32) > route.route_workspace(8 << 20, 1)


def test_workspace_argument_checks():
    lib = _lib.load()
    out = ctypes.c_uint64()
    assert lib.xsknf_gpu_route_workspace(10, 0, ctypes.byref(out)) == EINVAL
    assert lib.xsknf_gpu_route_workspace(10, 33, ctypes.byref(out)) == EINVAL
    assert lib.xsknf_gpu_route_workspace(10, 1, None) == EINVAL
    assert lib.xsknf_gpu_route_workspace(10, 32, ctypes.byref(out)) == 0 and out.value > 0


def _batch_call(**kw):
    """xsknf_gpu_route_batch with made-up, aligned device pointers (never
    dereferenced: every case here returns before a GPU call)."""
    a = dict(descs=0x10000, verdicts=0x20000, n=100, nif=3, tx=0x30000, fill=0x40000, order=0x50000, counts=None,
             ws=0x60000, ws_bytes=route.route_workspace(100, 3))
    a.update(kw)
    vp = ctypes.c_void_p
    return _lib.load().xsknf_gpu_route_batch(vp(a["descs"]), vp(a["verdicts"]), a["n"], a["nif"], vp(a["tx"]),
                                             vp(a["fill"]), vp(a["order"]), a["counts"], vp(a["ws"]), a["ws_bytes"],
                                             None)


@pytest.mark.parametrize("bad", [
    dict(nif=0), dict(nif=33), dict(nif=0, n=0), dict(nif=33, n=0),
    dict(descs=None), dict(verdicts=None), dict(tx=None), dict(fill=None), dict(ws=None),
    dict(descs=0x10008), dict(tx=0x30008), dict(descs=0x10004), dict(tx=0x30001),
    dict(fill=0x40004), dict(ws=0x60004), dict(fill=0x40001),
    dict(verdicts=0x20002), dict(order=0x50002), dict(verdicts=0x20001), dict(order=0x50003),
    dict(descs=0x10008, n=0), dict(order=0x50002, n=0),
    dict(ws_bytes=0), dict(ws_bytes=route.route_workspace(100, 3) - 1),
    dict(n=5000, ws_bytes=route.route_workspace(4096, 3)),
    dict(nif=32, ws_bytes=route.route_workspace(100, 32) - 1),
], ids=str)
def test_route_batch_refuses_before_any_gpu_call(bad):
    assert _batch_call(**bad) == EINVAL


def test_route_batch_of_no_frames_succeeds_without_a_gpu():
    for nif in NIFS:
        counts = np.full(nif + 1, 7, dtype=np.uint64)
        assert _batch_call(n=0, nif=nif, counts=counts.ctypes.data) == 0
        assert not counts.any()
        assert _batch_call(n=0, nif=nif) == 0
        assert _batch_call(n=0, nif=nif, descs=None, verdicts=None, tx=None, fill=None, order=None, ws=None,
                           ws_bytes=0, counts=counts.ctypes.data) == 0


def test_route_host_argument_checks():
    lib = _lib.load()
    d = RC.random_descs(8, 1)
    v = np.zeros(8, dtype=np.int32)
    tx, fill, od = np.zeros(8, dtype=frames.DESC_DTYPE), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    c = np.zeros(33, dtype=np.uint64)
    P = lambda a: a.ctypes.data
    f = lib.xsknf_gpu_route_host
    assert f(P(d), P(v), 8, 0, P(tx), P(fill), P(od), P(c)) == EINVAL
    assert f(P(d), P(v), 8, 33, P(tx), P(fill), P(od), P(c)) == EINVAL
    assert f(None, None, 0, 0, None, None, None, P(c)) == EINVAL
    assert f(None, P(v), 8, 2, P(tx), P(fill), P(od), P(c)) == EINVAL
    assert f(P(d), None, 8, 2, P(tx), P(fill), P(od), P(c)) == EINVAL
    assert f(P(d), P(v), 8, 2, None, P(fill), P(od), P(c)) == EINVAL
    assert f(P(d), P(v), 8, 2, P(tx), None, P(od), P(c)) == EINVAL
    assert f(P(d), P(v), 8, 2, P(tx), P(fill), None, None) == 0          # order and counts may be NULL
    c[:] = 9
    assert f(None, None, 0, 2, None, None, None, P(c)) == 0 and not c[:3].any() and c[3] == 9
    with pytest.raises(_lib.XsknfGpuError):
        route.route_host(d, v, 0)
    with pytest.raises(_lib.XsknfGpuError):
        route.route_workspace(1, 33)


def test_route_host_of_no_frames():
    for nif in NIFS:
        tx, fill, od, counts = route.route_host(np.zeros(0, dtype=frames.DESC_DTYPE), np.zeros(0, dtype=np.int32),
                                                nif, order=True)
        assert counts == [0] * (nif + 1) and tx.size == 0 and fill.size == 0 and od.size == 0


@pytest.mark.parametrize("nif", NIFS)
@pytest.mark.parametrize("pattern", RC.PATTERNS)
def test_route_host_equals_the_numpy_model(pattern, nif):
    """Counts, all three fields of tx_descs, fill_addrs, order (a permutation),
    and the sentinels past the totals, at sizes around one and several runs."""
    for n in (1, 2, 65, 4097, 20011):
        d = RC.random_descs(n, seed=n)
        v = RC.verdicts(pattern, n, nif, seed=n + nif)
        RC.same_as(RC.host_route_raw(d, v, nif), RC.model(d, v, nif), n, f"{pattern} n={n} nif={nif}")
        # order NULL: the lists alone come out the same
        RC.same_as(RC.host_route_raw(d, v, nif, order=False), RC.model(d, v, nif), n)
    if pattern == "stray" and nif > 1:
        assert (RC.bins_of(v, nif) == nif).sum() > (v == -1).sum()       # the strays dropped
    if pattern == "stray" and nif == 1:
        assert (RC.bins_of(v, nif) == 1).sum() == (v == -1).sum()        # the strays sent


def test_route_host_equals_the_numpy_model_past_one_scan_trip():
    """The largest batch the device router is held to route_host at
    (tests/test_gpu_route.py: three trips of its scan loop), interface 0 only in
    the later trips, 32 interfaces."""
    s, t = RC.scan_trip(), RC.tile_of("kernel_route.h")
    n = RC.long_sizes(s, t)[-1]
    assert n > 2 * s * t and n % 64
    d = RC.random_descs(n, seed=82)
    v = RC.verdicts("late-only", n, 32, seed=n, tile=t, trip=s)
    assert not (v[:s * t] == 0).any() and (v[s * t::3] == 0).all()
    RC.same_as(RC.host_route_raw(d, v, 32), RC.model(d, v, 32), n, f"late-only n={n}")


def test_late_only_at_small_sizes_has_no_frame_of_interface_0():
    for nif in NIFS:
        v = RC.verdicts("late-only", 5000, nif, seed=3)
        assert not (RC.bins_of(v, nif) == 0).any()
        assert set(RC.bins_of(v, nif)) == set(range(1, nif + 1))
        v = RC.verdicts("late-only", 5000, nif, seed=3, tile=100, trip=20)
        assert np.array_equal(np.flatnonzero(RC.bins_of(v, nif) == 0), np.arange(2000, 5000, 3))


def test_the_python_wrapper_returns_the_same_lists():
    d = RC.random_descs(5000, 3)
    v = RC.verdicts("stray", 5000, 3)
    tx, fill, od, counts = route.route_host(d, v, 3, order=True)
    wtx, wfill, word, wcounts = RC.model(d, v, 3)
    assert counts == wcounts and np.array_equal(od, word)
    assert np.array_equal(tx[:wtx.size], wtx) and np.array_equal(fill[:wfill.size], wfill)
    assert route.route_host(d, v, 3)[2] is None


def _dispose_in_ring_batches(descs, v, nif, batch=64):
    """The verdicts walked as the runtime does (xsknf_amd/csrc/xsknf_rt.c
    dispose_1if / dispose_multi, restated): ring batch by ring batch, each
    frame into to_drop[] or its destination's to_tx[], then each batch's lists
    appended to the fill ring and to the destinations' tx rings."""
    fill_ring, tx_rings = [], [[] for _ in range(nif)]
    for lo in range(0, len(v), batch):
        to_drop, to_tx = [], [[] for _ in range(nif)]
        for i in range(lo, min(lo + batch, len(v))):
            p = (int(descs["addr"][i]), int(descs["len"][i]))
            x = int(v[i])
            if nif == 1:
                (to_drop if x == -1 else to_tx[0]).append(p)
            elif x < 0 or x >= nif:
                to_drop.append(p)
            else:
                to_tx[x].append(p)
        fill_ring += [a for a, _ in to_drop]
        for k in range(nif):
            tx_rings[k] += [(a, l, 0) for a, l in to_tx[k]]
    return fill_ring, tx_rings


@pytest.mark.parametrize("nif", NIFS)
@pytest.mark.parametrize("pattern", ["uniform", "stray", "long-runs", "cycle"])
def test_routing_a_batch_equals_routing_its_ring_batches(pattern, nif):
    n = 9001
    d = RC.random_descs(n, 11)
    v = RC.verdicts(pattern, n, nif, seed=12)
    tx, fill, _, counts = RC.host_route_raw(d, v, nif)
    fill_ring, tx_rings = _dispose_in_ring_batches(d, v, nif)
    assert [int(a) for a in fill[:counts[nif]]] == fill_ring
    base = 0
    for k in range(nif):
        got = tx[base:base + counts[k]]
        assert [(int(a), int(l), int(o)) for a, l, o in zip(got["addr"], got["len"], got["options"])] == tx_rings[k]
        base += counts[k]


@pytest.mark.parametrize("action,nif,ingress,want", [
    (O.REDIRECT, 3, 1, {-1: 52, 0: 46, 2: 3998}),
    (O.DROP, 1, 0, {-1: 4050, 0: 46}),
], ids=["redirect-3if", "drop-1if"])
def test_end_to_end_behind_the_oracle(action, nif, ingress, want):
    """4096 IMIX frames with 5 % edge cases through the restatement oracle, then
    routed: the oracle's verdict counts are the recorded ones, every bin they
    name is non-empty, and the lists are the model's."""
    b = frames.unaligned_batch(4096, "imix", seed=91)
    frames.inject_edge_cases(b, 0.05, seed=92)
    v = O.c_process_batch(b.umem, b.descs, ingress=ingress, iters=1, action=action, nif=nif)
    vals, cnt = np.unique(v, return_counts=True)
    assert dict(zip((int(x) for x in vals), (int(c) for c in cnt))) == want
    got = RC.host_route_raw(b.descs, v, nif)
    RC.same_as(got, RC.model(b.descs, v, nif), 4096)
    counts = got[3]
    assert counts[nif] == want[-1] and counts[0] == want[0]
    if nif == 3:
        assert counts == [46, 0, 3998, 52] and all(counts[k] > 0 for k in (0, 2, 3))


def test_route_host_is_sanitizer_clean(tmp_path):
    """xsknf_amd/csrc/route_host.cpp under AddressSanitizer + UBSan on 4000
    random and edge-case sets (tests/c/san_route.c: a program of its own), the
    output buffers exactly as long as the lists, so a write past the totals is
    a heap overflow."""
    if not shutil.which("g++"):
        pytest.skip("g++ missing")
    exe = str(tmp_path / "san_route")
    subprocess.run(["g++", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Iinclude", "-x", "c", "tests/c/san_route.c", "-x", "c++",
                    "-std=c++17", "xsknf_amd/csrc/route_host.cpp", "-o", exe], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "ok 4000"
