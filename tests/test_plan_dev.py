"""The device-side shard planner's C ABI without a GPU (include/xsknf_gpu.h
xsknf_gpu_shard_plan_dev_workspace / _shard_plan_dev / xsknf_gpu_multi_scatter_dev):
the names are declared, bound and exported, the workspace size is host
arithmetic, and every argument error returns -EINVAL before any GPU call."""
import ctypes
import errno
import os
import re
import subprocess

import numpy as np

from xsknf_amd import _lib, multi

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


def test_scatter_dev_argument_errors_without_gpu():
    f = _lib.load().xsknf_gpu_multi_scatter_dev
    assert f(None, 0, None, 0, None, 0, _lib.PLAN_SPAN, None, None) == -errno.EINVAL
