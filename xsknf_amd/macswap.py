"""The macswap NF: every frame's destination and source MAC exchanged in place.

The reference's examples/macswap with the per-frame callback
(macswap_user.c:34-50, macswap.h): frames of at least 14 bytes get f[0..5] and
f[6..11] exchanged (twice with `double_macswap`, which leaves every byte as it
was) and the verdict (ingress_ifindex + 1) % num_interfaces -- for PASS as for
REDIRECT, the reference's own quirk -- or -1 for DROP.  The rules per frame and
the store contract are in include/xsknf_gpu.h ("the macswap NF").

`macswap_batch` does it on the device for a UMEM and descriptors that lie there
(xsknf_gpu_macswap_batch; xsknf_amd/csrc/macswap_device.hip), `macswap_host` on
one CPU thread (xsknf_gpu_macswap_host: the model the device is held to).  The
verdicts are what route.route_batch consumes.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

ACTION_REDIRECT = _lib.MACSWAP_ACTION_REDIRECT
ACTION_DROP = _lib.MACSWAP_ACTION_DROP
ACTION_PASS = _lib.MACSWAP_ACTION_PASS


def _opts(action: int, double_macswap, num_interfaces: int) -> _lib.MacswapOpts:
    return _lib.MacswapOpts(action, 1 if double_macswap else 0, num_interfaces, 0)


def macswap_host(umem, descs, ingress_ifindex: int = 0, *, action: int = ACTION_REDIRECT, double_macswap=False,
                 num_interfaces: int = 1):
    """xsknf_gpu_macswap_host on numpy arrays (a uint8 UMEM, 16-byte descriptor
    records): (a copy of the UMEM after the batch, one int32 verdict per
    descriptor).  `umem` itself is not written."""
    u = np.array(umem, copy=True, order="C")
    if u.dtype != np.uint8:
        raise ValueError("umem must be uint8")
    d = np.ascontiguousarray(descs)
    if d.dtype.itemsize != 16:
        raise ValueError("descriptors must be struct xdp_desc records (16 bytes)")
    n = int(d.shape[0])
    v = np.zeros(n, dtype=np.int32)
    o = _opts(action, double_macswap, num_interfaces)
    # (an empty UMEM still needs an address: every descriptor is then outside it)
    up = (u.ctypes.data if u.size else v.ctypes.data) if n else None
    _lib.check(_lib.load().xsknf_gpu_macswap_host(up, u.size, d.ctypes.data if n else None, n, ingress_ifindex,
                                                  ctypes.byref(o), v.ctypes.data if n else None),
               "xsknf_gpu_macswap_host")
    return u, v


def macswap_batch_ptr(umem_ptr: int, umem_size: int, descs_ptr: int, n: int, ingress_ifindex: int, verdicts_ptr: int,
                      stream: int = 0, *, action: int = ACTION_REDIRECT, double_macswap=False,
                      num_interfaces: int = 1) -> None:
    """Raw-pointer form of xsknf_gpu_macswap_batch (device pointers; 0 = NULL),
    on the current device: only enqueues on `stream`."""
    o = _opts(action, double_macswap, num_interfaces)
    _lib.check(_lib.load().xsknf_gpu_macswap_batch(
        ctypes.c_void_p(umem_ptr or None), umem_size, ctypes.c_void_p(descs_ptr or None), n, ingress_ifindex,
        ctypes.byref(o), ctypes.c_void_p(verdicts_ptr or None), ctypes.c_void_p(stream or None)),
        "xsknf_gpu_macswap_batch")


def macswap_batch(umem, descs, ingress_ifindex: int = 0, *, action: int = ACTION_REDIRECT, double_macswap=False,
                  num_interfaces: int = 1):
    """xsknf_gpu_macswap_batch on torch tensors, in place, on the current stream
    of their device: `umem` a contiguous uint8 device tensor, `descs` (n, 2)
    int64 / (n, 16) uint8, contiguous.  Returns the verdicts as an int32 device
    tensor of n entries; nothing waits for the stream."""
    import torch

    if not umem.is_cuda or not descs.is_cuda:
        raise ValueError("umem and descs must be device tensors (macswap_host is the CPU form)")
    if umem.dtype != torch.uint8 or not umem.is_contiguous():
        raise ValueError("umem must be a contiguous uint8 tensor")
    if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
        raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
    n = descs.numel() * descs.element_size() // 16
    dev = umem.device
    if descs.device != dev:
        raise ValueError("umem and descs must lie on one device")
    with torch.cuda.device(dev):
        v = torch.empty(n, dtype=torch.int32, device=dev)
        macswap_batch_ptr(umem.data_ptr() if n else 0, umem.numel(), descs.data_ptr() if n else 0, n, ingress_ifindex,
                          v.data_ptr() if n else 0, torch.cuda.current_stream(dev).cuda_stream, action=action,
                          double_macswap=double_macswap, num_interfaces=num_interfaces)
    return v
