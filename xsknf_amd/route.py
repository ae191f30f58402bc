"""Routing a checksummed batch: per-interface tx lists and the fill list.

The second half of the reference's batch loop (process_batch, src/xsknf.c:503-522,
and process_batch_1if, :654-672): every frame is filed by its verdict, a dropped
frame into to_drop[] and any other into to_tx[verdict][], in receive order.
`route_batch` does that on the device for verdicts and descriptors that lie there
(include/xsknf_gpu.h xsknf_gpu_route_batch; xsknf_amd/csrc/route_device.hip),
`route_host` on one CPU thread (xsknf_gpu_route_host: the model the device is
held to).  Both return

    tx_descs    n records; interface i's list is [base_i, base_i + counts[i]),
                base_i = sum(counts[:i]); each {addr, len, options 0}
    fill_addrs  n words; the first counts[num_interfaces] are the dropped frames' addresses
    order       n words or None: the frame behind every entry, the tx lists first, then the drops
    counts      num_interfaces + 1 numbers: frames per interface, then the drops

Entries past the totals are not written.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_INTERFACES = _lib.ROUTE_MAX_INTERFACES
DESC_DTYPE = np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")])


def route_workspace(n: int, num_interfaces: int) -> int:
    """Bytes of device workspace route_batch needs for n frames (no GPU)."""
    out = ctypes.c_uint64()
    _lib.check(_lib.load().xsknf_gpu_route_workspace(n, num_interfaces, ctypes.byref(out)),
               "xsknf_gpu_route_workspace")
    return int(out.value)


def route_host(descs, verdicts, num_interfaces: int, order: bool = False):
    """xsknf_gpu_route_host on numpy arrays (16-byte descriptor records, int32
    verdicts): (tx_descs, fill_addrs, order or None, counts)."""
    d = np.ascontiguousarray(descs)
    if d.dtype.itemsize != 16:
        raise ValueError("descriptors must be struct xdp_desc records (16 bytes)")
    v = np.ascontiguousarray(verdicts)
    if v.dtype != np.int32 or v.shape[0] != d.shape[0]:
        raise ValueError("verdicts must be one int32 per descriptor")
    n = int(d.shape[0])
    tx = np.zeros(n, dtype=DESC_DTYPE)
    fill = np.zeros(n, dtype=np.uint64)
    od = np.zeros(n, dtype=np.uint32) if order else None
    counts = np.zeros(max(int(num_interfaces), 0) + 1, dtype=np.uint64)
    _lib.check(_lib.load().xsknf_gpu_route_host(d.ctypes.data if n else None, v.ctypes.data if n else None, n,
                                                num_interfaces, tx.ctypes.data if n else None,
                                                fill.ctypes.data if n else None,
                                                od.ctypes.data if order and n else None, counts.ctypes.data),
               "xsknf_gpu_route_host")
    return tx, fill, od, [int(c) for c in counts]


def route_batch_ptr(descs_ptr: int, verdicts_ptr: int, n: int, num_interfaces: int, tx_descs_ptr: int,
                    fill_addrs_ptr: int, order_ptr: int, workspace_ptr: int, workspace_bytes: int, stream: int = 0,
                    sync: bool = True):
    """Raw-pointer form of xsknf_gpu_route_batch (device pointers; 0 = NULL), on
    the current device.  sync: wait for `stream` and return the counts list;
    otherwise only enqueue and return None -- the counts are then the first
    num_interfaces + 1 u64 words of the workspace once the stream gets there."""
    counts = np.zeros(max(int(num_interfaces), 0) + 1, dtype=np.uint64)
    _lib.check(_lib.load().xsknf_gpu_route_batch(
        ctypes.c_void_p(descs_ptr or None), ctypes.c_void_p(verdicts_ptr or None), n, num_interfaces,
        ctypes.c_void_p(tx_descs_ptr or None), ctypes.c_void_p(fill_addrs_ptr or None),
        ctypes.c_void_p(order_ptr or None), counts.ctypes.data if sync else None,
        ctypes.c_void_p(workspace_ptr or None), workspace_bytes, ctypes.c_void_p(stream or None)),
        "xsknf_gpu_route_batch")
    return [int(c) for c in counts] if sync else None


def route_batch(descs, verdicts, num_interfaces: int, *, order: bool = False, device=None):
    """xsknf_gpu_route_batch on torch tensors, on the current stream of their
    device: `descs` (n, 2) int64 / (n, 16) uint8 and `verdicts` int32, both
    contiguous device tensors.  Returns (tx_descs as an (n, 2) int64 tensor of
    16-byte records, fill_addrs as n int64, order as n int32 or None, counts)."""
    import torch

    if not descs.is_cuda or not verdicts.is_cuda:
        raise ValueError("descs and verdicts must be device tensors (route_host is the CPU form)")
    if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
        raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
    n = descs.numel() * descs.element_size() // 16
    if verdicts.dtype != torch.int32 or not verdicts.is_contiguous() or verdicts.numel() < n:
        raise ValueError("verdicts must be a contiguous int32 tensor with >= n entries")
    dev = descs.device if device is None else torch.device(device)
    if descs.device != dev or verdicts.device != dev:
        raise ValueError("descs and verdicts must lie on the routing device")
    with torch.cuda.device(dev):
        tx = torch.empty((n, 2), dtype=torch.int64, device=dev)
        fill = torch.empty(n, dtype=torch.int64, device=dev)
        od = torch.empty(n, dtype=torch.int32, device=dev) if order else None
        ws = torch.empty(route_workspace(n, num_interfaces) // 8, dtype=torch.int64, device=dev)
        counts = route_batch_ptr(descs.data_ptr() if n else 0, verdicts.data_ptr() if n else 0, n, num_interfaces,
                                 tx.data_ptr() if n else 0, fill.data_ptr() if n else 0,
                                 od.data_ptr() if order and n else 0, ws.data_ptr(), ws.numel() * 8,
                                 torch.cuda.current_stream(dev).cuda_stream)
    return tx, fill, od, counts
