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

`forward_frames` / `forward_host` then do the copy that ends the batch loop
(:563-571; xsknf_gpu_forward_frames, xsknf_amd/csrc/forward_device.hip): every
frame of the tx list of an interface with a UMEM of its own is copied from the rx
UMEM into that UMEM at the same offset.  Both return the stats
[frames copied, bytes copied, frames skipped as out of range].
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

MAX_INTERFACES = _lib.ROUTE_MAX_INTERFACES
FORWARD_STATS = _lib.FORWARD_STATS
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


def _umem_arrays(ptrs, sizes):
    """The host arrays of the forward calls: (uint8_t *[], uint64_t[])."""
    k = len(ptrs)
    return (ctypes.c_void_p * max(k, 1))(*[p or None for p in ptrs]), (ctypes.c_uint64 * max(k, 1))(*sizes)


def forward_host(rx_umem, tx_umems, tx_descs, counts):
    """xsknf_gpu_forward_host on numpy arrays: `rx_umem` uint8, `tx_umems` a list
    of writable uint8 arrays or None (16-byte aligned, as the C call asks),
    `tx_descs` 16-byte records and `counts` as route_host returns them (one
    number per interface; the drops after them are not used).  The destination
    arrays are written in place; returns the stats list."""
    d = np.ascontiguousarray(tx_descs)
    if d.dtype.itemsize != 16:
        raise ValueError("tx_descs must be struct xdp_desc records (16 bytes)")
    nif = len(tx_umems)
    c = np.zeros(nif + 1, dtype=np.uint64)
    k = min(len(counts), nif + 1)
    c[:k] = np.asarray(counts[:k], dtype=np.uint64)
    if int(c[:nif].sum()) > d.shape[0]:
        raise ValueError("counts name more entries than tx_descs holds")
    for t in tx_umems:
        if t is not None and (t.dtype != np.uint8 or not t.flags.c_contiguous or not t.flags.writeable):
            raise ValueError("a destination UMEM must be a writable contiguous uint8 array")
    rx = np.ascontiguousarray(rx_umem)
    if rx.dtype != np.uint8:
        raise ValueError("rx_umem must be uint8")
    ptrs, sizes = _umem_arrays([0 if t is None else t.ctypes.data for t in tx_umems],
                               [0 if t is None else t.size for t in tx_umems])
    stats = np.zeros(FORWARD_STATS, dtype=np.uint64)
    _lib.check(_lib.load().xsknf_gpu_forward_host(rx.ctypes.data, rx.size, ptrs, sizes, nif,
                                                  d.ctypes.data if d.shape[0] else None, c.ctypes.data,
                                                  stats.ctypes.data), "xsknf_gpu_forward_host")
    return [int(x) for x in stats]


def forward_frames_ptr(rx_umem_ptr: int, rx_umem_size: int, tx_umem_ptrs, tx_umem_sizes, tx_descs_ptr: int,
                       counts_ptr: int, n: int, stats_ptr: int, stream: int = 0, sync: bool = True):
    """Raw-pointer form of xsknf_gpu_forward_frames (device pointers; 0 = NULL),
    on the current device; `tx_umem_ptrs` / `tx_umem_sizes` are sequences with one
    entry per interface.  sync: wait for `stream` and return the stats list;
    otherwise only enqueue and return None -- the stats are then the 3 u64 words
    at `stats_ptr` once the stream gets there."""
    if len(tx_umem_ptrs) != len(tx_umem_sizes):
        raise ValueError("one size per UMEM pointer")
    ptrs, sizes = _umem_arrays(list(tx_umem_ptrs), list(tx_umem_sizes))
    stats = np.zeros(FORWARD_STATS, dtype=np.uint64)
    _lib.check(_lib.load().xsknf_gpu_forward_frames(
        ctypes.c_void_p(rx_umem_ptr or None), rx_umem_size, ptrs, sizes, len(tx_umem_ptrs),
        ctypes.c_void_p(tx_descs_ptr or None), ctypes.c_void_p(counts_ptr or None), n,
        ctypes.c_void_p(stats_ptr or None), stats.ctypes.data if sync else None, ctypes.c_void_p(stream or None)),
        "xsknf_gpu_forward_frames")
    return [int(x) for x in stats] if sync else None


def forward_frames(rx_umem, tx_umems, tx_descs, counts_dev, *, n=None):
    """xsknf_gpu_forward_frames on torch tensors, on the current stream of their
    device: `rx_umem` a uint8 device tensor, `tx_umems` a list with one uint8
    device tensor (a UMEM of its own, written in place) or None (shares the rx
    UMEM) per interface, `tx_descs` route_batch's, `counts_dev` a contiguous
    int64 device tensor of len(tx_umems) + 1 words (the route's workspace starts
    with them) or the counts list route_batch returned.  n: the capacity of
    tx_descs (default: all of it).  Returns the stats list."""
    import torch

    if not rx_umem.is_cuda or not tx_descs.is_cuda:
        raise ValueError("rx_umem and tx_descs must be device tensors (forward_host is the CPU form)")
    dev = rx_umem.device
    if rx_umem.dtype != torch.uint8 or not rx_umem.is_contiguous():
        raise ValueError("rx_umem must be a contiguous uint8 tensor")
    if not tx_descs.is_contiguous() or tx_descs.numel() * tx_descs.element_size() % 16 or tx_descs.device != dev:
        raise ValueError("tx_descs must be a contiguous array of 16-byte xdp_desc on rx_umem's device")
    cap = tx_descs.numel() * tx_descs.element_size() // 16
    n = cap if n is None else int(n)
    if n < 0 or n > cap:
        raise ValueError("n is the capacity of tx_descs at most")
    nif = len(tx_umems)
    for t in tx_umems:
        if t is not None and (not t.is_cuda or t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous()):
            raise ValueError("a destination UMEM must be a contiguous uint8 tensor on rx_umem's device")
    with torch.cuda.device(dev):
        if not torch.is_tensor(counts_dev):
            c = [int(x) for x in counts_dev][:nif + 1]
            counts_dev = torch.tensor(c + [0] * (nif + 1 - len(c)), dtype=torch.int64).to(dev)
        if (not counts_dev.is_cuda or counts_dev.device != dev or counts_dev.element_size() != 8
                or not counts_dev.is_contiguous() or counts_dev.numel() < nif + 1):
            raise ValueError("counts_dev must hold len(tx_umems) + 1 contiguous 8-byte words on rx_umem's device")
        stats_dev = torch.empty(FORWARD_STATS, dtype=torch.int64, device=dev)
        return forward_frames_ptr(rx_umem.data_ptr(), rx_umem.numel(),
                                  [0 if t is None else t.data_ptr() for t in tx_umems],
                                  [0 if t is None else t.numel() for t in tx_umems],
                                  tx_descs.data_ptr() if n else 0, counts_dev.data_ptr(), n, stats_dev.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
