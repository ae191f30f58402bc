"""The device-side shard planner's C ABI without a GPU (include/xsknf_gpu.h
xsknf_gpu_shard_plan_dev_workspace / _shard_plan_dev / xsknf_gpu_multi_scatter_dev):
the names are declared, bound and exported, the workspace size is host
arithmetic, and every argument error returns -EINVAL before any GPU call.  And
the host functions the device planner is held to, against numpy models at the
largest batch the device tests use."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np

from tests import route_cases as RC
from xsknf_amd import _lib, multi, shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("xsknf_gpu_shard_plan_dev_workspace", "xsknf_gpu_shard_plan_dev", "xsknf_gpu_multi_scatter_dev")


def test_new_names_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "xsknf_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(rf"\bXSKNF_GPU_API\b[^;(]*?\b{name}\s*\(", header), name
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}\b", out), name
    assert re.search(r"#define\s+XSKNF_GPU_PLAN_SPAN\s+0\b", header) and _lib.PLAN_SPAN == 0
    assert re.search(r"#define\s+XSKNF_GPU_PLAN_PACKED\s+1\b", header) and _lib.PLAN_PACKED == 1


def test_workspace_size_is_positive_and_non_decreasing():
    sizes = [multi.plan_dev_workspace(n) for n in (0, 1, 2, 64, 1000, 4096, 4097, 300001, 8 << 20, 1 << 32)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # a u64 per tile and scan: far below the descriptors themselves
    assert multi.plan_dev_workspace(8 << 20) < (8 << 20) * 16 // 64
    # every shard count asks for the same, the header being sized for 64
    assert {multi.plan_dev_workspace(12345, k) for k in (1, 2, 8, 64)} == {multi.plan_dev_workspace(12345)}
    lib = _lib.load()
    out = ctypes.c_uint64()
    assert lib.xsknf_gpu_shard_plan_dev_workspace(10, 0, ctypes.byref(out)) == -errno.EINVAL
    assert lib.xsknf_gpu_shard_plan_dev_workspace(10, 65, ctypes.byref(out)) == -errno.EINVAL
    assert lib.xsknf_gpu_shard_plan_dev_workspace(10, 8, None) == -errno.EINVAL


def test_plan_dev_argument_errors_without_gpu():
    """Each of these returns before any HIP call: the pointers are made-up
    addresses that are never dereferenced."""
    f = _lib.load().xsknf_gpu_shard_plan_dev
    n, need = 1000, multi.plan_dev_workspace(1000)
    bounds = np.zeros(65, dtype=np.uint64)
    aux = np.zeros(128, dtype=np.uint64)
    fb = np.zeros(64, dtype=np.uint64)
    b, a, s = bounds.ctypes.data, aux.ctypes.data, fb.ctypes.data
    d, o, w = 0x7f0000001000, 0x7f0000101000, 0x7f0000201000
    E = -errno.EINVAL
    assert f(d, n, 0, 1 << 20, 0, _lib.PLAN_SPAN, o, b, a, s, w, need, None) == E       # no shards
    assert f(d, n, 0, 1 << 20, 65, _lib.PLAN_SPAN, o, b, a, s, w, need, None) == E      # too many
    assert f(d, n, 0, 1 << 20, 8, _lib.PLAN_SPAN, o, None, a, s, w, need, None) == E    # NULL bounds
    assert f(None, n, 0, 1 << 20, 8, _lib.PLAN_SPAN, o, b, a, s, w, need, None) == E    # NULL descriptors
    assert f(d, n, 0, 1 << 20, 8, _lib.PLAN_PACKED, None, b, a, s, w, need, None) == E  # NULL output
    assert f(d, n, 0, 1 << 20, 8, _lib.PLAN_PACKED, o, b, a, s, None, need, None) == E  # NULL workspace
    assert f(d, n, 0, 1 << 20, 8, _lib.PLAN_SPAN, o, b, a, s, w, need - 1, None) == E   # workspace too small
    assert f(d, n, 0, 1 << 20, 8, 2, o, b, a, s, w, need, None) == E                    # unknown mode
    assert f(d, n, 0, 1 << 20, 8, -1, o, b, a, s, w, need, None) == E
    assert f(d + 8, n, 0, 1 << 20, 8, _lib.PLAN_SPAN, o, b, a, s, w, need, None) == E   # records not 16-byte aligned
    assert f(None, 0, 0, 0, 0, _lib.PLAN_SPAN, None, b, None, None, None, 0, None) == E  # n == 0 checks them too
    assert f(None, 0, 0, 0, 8, 7, None, b, None, None, None, 0, None) == E


def test_plan_dev_of_nothing_needs_no_gpu():
    """n == 0 succeeds without a launch: all cuts, spans / sizes and sums zero."""
    f = _lib.load().xsknf_gpu_shard_plan_dev
    for mode, naux in ((_lib.PLAN_SPAN, 16), (_lib.PLAN_PACKED, 8)):
        bounds = np.full(9, 77, dtype=np.uint64)
        aux = np.full(naux, 77, dtype=np.uint64)
        fb = np.full(8, 77, dtype=np.uint64)
        assert f(None, 0, 0, 1 << 20, 8, mode, None, bounds.ctypes.data, aux.ctypes.data, fb.ctypes.data,
                 None, 0, None) == 0
        assert not bounds.any() and not aux.any() and not fb.any()


def _pack_model(descs, bounds, umem_addr, umem_size):
    """xsknf_gpu_shard_pack_plan restated in numpy: one exclusive prefix sum of
    the slot bytes over the whole batch, minus its value at each shard's start."""
    inr = shard._in_umem(descs, umem_size)
    r = ((np.uint64(umem_addr) + shard.effective_offsets(descs).astype(np.uint64)) & np.uint64(15)).astype(np.int64)
    ln = descs["len"].astype(np.int64)
    slot = np.where(inr & (ln > 0), (r + ln + 15) // 16 * 16, 0)
    pre = np.concatenate([[0], np.cumsum(slot)])
    b = np.asarray(bounds, dtype=np.int64)
    first = b[np.searchsorted(b[1:], np.arange(descs.size), side="right")]      # each frame's shard's first frame
    out = np.zeros_like(descs)
    out["len"], out["options"] = descs["len"], descs["options"]
    out["addr"] = np.where(inr, (pre[:-1] - pre[first] + r).astype(np.uint64), shard.OUT_OF_RANGE)
    return out, [int(pre[hi] - pre[lo]) for lo, hi in zip(b[:-1], b[1:])]


def test_host_plan_equals_the_numpy_models_past_one_scan_trip():
    """The host functions the device planner is held to (tests/test_gpu_plan_dev.py)
    at its largest batch -- more than two trips of the device's scan over the
    tile totals: xsknf_gpu_shard_plan / _rebase against xsknf_amd/shard.py, and
    _shard_pack_plan against a numpy restatement, with every 37th frame outside
    the UMEM."""
    s, t = RC.scan_trip(), RC.tile_of("kernel_plan.h")
    n = RC.long_sizes(s, t)[-1]
    d, size = RC.plan_descs(n)
    off = shard.effective_offsets(d)
    for lo in (0, s * t, 2 * s * t):      # in every trip every address mod 16 meets every length
        seen = set(zip((off[lo:lo + 4096] % 16).tolist(), d["len"][lo:lo + 4096].tolist()))
        assert seen == {(r, ln) for r in range(16) for ln in RC.PLAN_LENS}
    assert np.all(off[1:] >= off[:-1] + d["len"][:-1]) and int(off[-1]) + int(d["len"][-1]) <= size
    d["addr"][::37] += np.uint64(1 << 40)
    for nshards in (3, 64):
        ranges, spans = multi.shard_plan(d, nshards, size)
        assert ranges == shard.shard_by_bytes(d["len"], nshards)
        assert spans == shard.shard_spans(d, ranges, size)
        got = np.concatenate([multi.shard_rebase(d[lo:hi], b0, size) for (lo, hi), (b0, _) in zip(ranges, spans)])
        want = np.concatenate([shard.rebase_descs(d[lo:hi], b0, size) for (lo, hi), (b0, _) in zip(ranges, spans)])
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        bounds = [0] + [hi for _, hi in ranges]
        got, sizes = multi.pack_plan(d, bounds, 0x7F5A12340007, size)
        want, wsizes = _pack_model(d, bounds, 0x7F5A12340007, size)
        assert sizes == wsizes and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert {hi // t // s for _, hi in ranges} == {0, 1, 2}       # cuts in both whole trips, the end in the third


def test_scatter_dev_argument_errors_without_gpu():
    f = _lib.load().xsknf_gpu_multi_scatter_dev
    assert f(None, 0, None, 0, None, 0, _lib.PLAN_SPAN, None, None) == -errno.EINVAL
