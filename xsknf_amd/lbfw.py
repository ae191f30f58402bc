"""The lbfw NF: the firewall's ACL as a gate in front of the load balancer.

The reference's examples/lbfw (lbfw_user.c:420-594): the load balancer's
per-frame function with two differences.  PASS is `(ingress_ifindex + 1) %
num_interfaces` whatever the interface count (one interface passes to 0, not
-1; 0 interfaces is an error), and a frame whose 5-tuple the ACL holds gets
that rule's action as its verdict -- any int32, 0 included -- untouched and
without a session being looked up or stored.  The rules are in
include/xsknf_gpu.h ("the lbfw NF", on top of "the load balancer NF").

The calls work on the existing objects, a `firewall.Acl` (or None: the
reference's MODE_COMBINED, where XDP has applied the ACL already) and a
`lb.LoadBalancer`, whose session tables are shared with `lb_batch` / `lb_host`.
`lbfw_batch` runs a batch on the device (xsknf_gpu_lbfw_batch;
xsknf_amd/csrc/lb_device.hip), `lbfw_host` on one CPU thread
(xsknf_gpu_lbfw_host: the model the device is held to).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .firewall import Acl
from .lb import LB_STATS, LoadBalancer, lb_workspace

# the words of a batch's stats: the load balancer's, with the frames the ACL decided
LBFW_STATS = LB_STATS[:7] + ("acl_decided",)
assert len(LBFW_STATS) == _lib.LB_STATS


def _acl_handle(acl: Acl | None):
    return None if acl is None else acl.handle


def lbfw_host(umem, descs, acl: Acl | None, lb: LoadBalancer, ingress_ifindex: int = 0, num_interfaces: int = 1):
    """xsknf_gpu_lbfw_host on numpy arrays: `umem` (uint8, contiguous, writable)
    is rewritten IN PLACE over the host session table of `lb`, behind the host
    copy of `acl` (None: no gate).  Returns (verdicts int32, stats uint64[8])."""
    if not (isinstance(umem, np.ndarray) and umem.dtype == np.uint8 and umem.flags.c_contiguous
            and umem.flags.writeable):
        raise ValueError("umem must be a writable contiguous uint8 array (it is rewritten in place)")
    d = np.ascontiguousarray(descs)
    if d.dtype.itemsize != 16:
        raise ValueError("descriptors must be struct xdp_desc records (16 bytes)")
    n = int(d.shape[0])
    v = np.zeros(n, dtype=np.int32)
    st = np.zeros(_lib.LB_STATS, dtype=np.uint64)
    # (an empty UMEM still needs an address: every descriptor is then outside it)
    up = umem.ctypes.data if umem.size else st.ctypes.data
    _lib.check(_lib.load().xsknf_gpu_lbfw_host(up if n else None, umem.size, d.ctypes.data if n else None, n,
                                               ingress_ifindex, num_interfaces, _acl_handle(acl), lb.handle,
                                               v.ctypes.data if n else None, st.ctypes.data), "xsknf_gpu_lbfw_host")
    return v, st


def lbfw_batch_ptr(umem_ptr: int, umem_size: int, descs_ptr: int, n: int, ingress_ifindex: int, num_interfaces: int,
                   acl: Acl | None, lb: LoadBalancer, verdicts_ptr: int, workspace_ptr: int, workspace_bytes: int,
                   stats_ptr: int, stream: int = 0) -> None:
    """Raw-pointer form of xsknf_gpu_lbfw_batch (device pointers; 0 = NULL), on
    the current device: only enqueues on `stream`."""
    _lib.check(_lib.load().xsknf_gpu_lbfw_batch(
        ctypes.c_void_p(umem_ptr or None), umem_size, ctypes.c_void_p(descs_ptr or None), n, ingress_ifindex,
        num_interfaces, _acl_handle(acl), lb.handle, ctypes.c_void_p(verdicts_ptr or None),
        ctypes.c_void_p(workspace_ptr or None), workspace_bytes, ctypes.c_void_p(stats_ptr or None),
        ctypes.c_void_p(stream or None)), "xsknf_gpu_lbfw_batch")


def lbfw_batch(umem, descs, acl: Acl | None, lb: LoadBalancer, ingress_ifindex: int = 0, num_interfaces: int = 1, *,
               workspace=None, device=None):
    """xsknf_gpu_lbfw_batch on torch tensors, on the current stream of their
    device (the one `acl` and `lb` were made on): `umem` a contiguous uint8
    device tensor, rewritten IN PLACE; `descs` (n, 2) int64 / (n, 16) uint8,
    contiguous; `workspace` a uint8 device tensor of at least lb_workspace(n)
    bytes (default: a new one).  Returns (verdicts int32[n], stats int64[8]) as
    device tensors; nothing waits for the stream."""
    import torch

    if not umem.is_cuda or not descs.is_cuda:
        raise ValueError("umem and descs must be device tensors (lbfw_host is the CPU form)")
    if umem.dtype != torch.uint8 or not umem.is_contiguous():
        raise ValueError("umem must be a contiguous uint8 tensor")
    if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
        raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
    n = descs.numel() * descs.element_size() // 16
    dev = umem.device if device is None else torch.device(device)
    if umem.device != dev or descs.device != dev:
        raise ValueError("umem and descs must lie on the device of the ACL and the load balancer")
    need = lb_workspace(n)
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif (workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
              or workspace.numel() < need):
            raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on the device")
        v = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.zeros(_lib.LB_STATS, dtype=torch.int64, device=dev)
        lbfw_batch_ptr(umem.data_ptr() if n else 0, umem.numel(), descs.data_ptr() if n else 0, n, ingress_ifindex,
                       num_interfaces, acl, lb, v.data_ptr() if n else 0, workspace.data_ptr() if n else 0,
                       workspace.numel(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return v, st
