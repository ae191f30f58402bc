"""The load balancer NF: session table, NAT rewrite, one verdict per frame.

The reference's L4 load balancer with the per-frame callback
(examples/load_balancer/load_balancer_user.c:396-553): a frame of a known
session is rewritten towards its backend or its client, a frame to a virtual
service without a session picks a backend, stores the forward and the backward
session and is rewritten, everything else passes.  The rules per frame are in
include/xsknf_gpu.h ("the load balancer NF").

`LoadBalancer` holds the services, the backends and two independent session
tables (xsknf_gpu_lb_*: xsknf_amd/csrc/lb.cpp), one on the host and one on the
device that was current when it was made.  `lb_batch` runs a batch on the device
for a UMEM and descriptors that lie there (xsknf_gpu_lb_batch;
xsknf_amd/csrc/lb_device.hip), `lb_host` on one CPU thread (xsknf_gpu_lb_host:
the model the device is held to).  Both rewrite the UMEM in place; the verdicts
are what route.route_batch consumes.  Sessions end through
`LoadBalancer.sessions_remove`, `drain_backend` and `sessions_clear`
(xsknf_amd/csrc/lb_remove_device.hip for the device table): on the device they
are enqueued between batches and wait for nothing.  The services and backends
change under traffic through `LoadBalancer.backends_update`
(xsknf_amd/csrc/lb_backends_device.hip for the device copy), and
`drain_backends` ends the flows of a list of backends in one pass.  With
`LoadBalancer.aging_enable` every session carries a last-seen stamp that the
batches write; `clock` sets a table's clock and `expire` ends the flows that
have been idle too long (xsknf_amd/csrc/kernel_lb_stamp.h, kernel_lb_expire.h).
"""
from __future__ import annotations

import ctypes
import errno

import numpy as np

from . import _lib

MAX_SERVICES = _lib.LB_MAX_SERVICES
MAX_BACKENDS = _lib.LB_MAX_BACKENDS
MAX_SESSIONS = _lib.LB_MAX_SESSIONS
MAX_SLOTS = _lib.LB_MAX_SLOTS
MAX_BATCH = _lib.LB_MAX_BATCH
TO_CLIENT, TO_BACKEND = 0, 1
HOST_TABLE, DEVICE_TABLE = 0, 1
# the words of a batch's stats (XSKNF_GPU_LB_STATS)
LB_STATS = ("frames", "rewritten", "passed", "dropped", "sessions_created", "inserts_failed", "ordered_batches",
            "reserved")
assert len(LB_STATS) == _lib.LB_STATS
# addresses and ports in network order, i.e. the frame's own bytes read as
# little-endian numbers
BACKEND_DTYPE = np.dtype([("vaddr", "<u4"), ("vport", "<u2"), ("proto", "u1"), ("pad", "u1"), ("addr", "<u4"),
                          ("port", "<u2"), ("mac", "u1", (6,)), ("ifindex", "<u2"), ("pad2", "u1", (2,))])
KEY_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1"),
                      ("pad", "u1", (3,))])
VALUE_DTYPE = np.dtype([("addr", "<u4"), ("port", "<u2"), ("ifindex", "<u2"), ("mac", "u1", (6,)), ("dir", "u1"),
                        ("pad", "u1")])
# struct xsknf_gpu_lb_backend_op: a backend record and BACKEND_ADD or BACKEND_REMOVE
BACKEND_ADD, BACKEND_REMOVE = _lib.LB_BACKEND_ADD, _lib.LB_BACKEND_REMOVE
BACKEND_OP_DTYPE = np.dtype([("backend", BACKEND_DTYPE), ("op", "<u4")])
# struct xsknf_gpu_lb_backend_id: what drain_backends lists
BACKEND_ID_DTYPE = np.dtype([("addr", "<u4"), ("port", "<u2"), ("proto", "u1"), ("pad", "u1")])
assert BACKEND_DTYPE.itemsize == 24 and KEY_DTYPE.itemsize == 16 and VALUE_DTYPE.itemsize == 16
assert BACKEND_OP_DTYPE.itemsize == 28 and BACKEND_ID_DTYPE.itemsize == 8


def _records(a, itemsize: int, what: str) -> np.ndarray:
    r = np.ascontiguousarray(a)
    if r.dtype.itemsize != itemsize or r.ndim != 1:
        raise ValueError(f"{what} must be a 1-d array of {itemsize}-byte records")
    return r


class LoadBalancer:
    """struct xsknf_gpu_lb: services, backends and the session tables, on the
    host and (where the process sees one) on the current device."""

    def __init__(self, handle: int):
        self._h = handle
        self._device_half = None   # whether the object has a device half (asked once)

    @classmethod
    def from_backends(cls, backends, max_sessions: int = MAX_SESSIONS, slots: int = 0, *, device=None) -> "LoadBalancer":
        """backends: BACKEND_DTYPE records, one per backend of a service; a
        service's backend number is the record's order among that service's
        records.  max_sessions: what a session table may hold.  slots: 0 for
        the default, or a power of two >= 2 * max_sessions.  device: make it
        current for the upload (default: the current device)."""
        r = _records(backends, 24, "backends")
        h = ctypes.c_void_p()

        def create():
            _lib.check(_lib.load().xsknf_gpu_lb_create(ctypes.byref(h), r.ctypes.data if r.size else None, r.size,
                                                       max_sessions, slots), "xsknf_gpu_lb_create")
        if device is None:
            create()
        else:
            import torch
            with torch.cuda.device(device):
                create()
        made = cls(h.value)
        made._has_device_half()   # (asked now: _info waits for the device, which a later update must not)
        return made

    @property
    def handle(self) -> int:
        if not self._h:
            raise ValueError("the load balancer is closed")
        return self._h

    @property
    def info(self) -> dict:
        """services, backends, max_sessions, slots, host_sessions, device_sessions, device_bytes."""
        i = _lib.LbInfo()
        _lib.check(_lib.load().xsknf_gpu_lb_info(self.handle, ctypes.byref(i)), "xsknf_gpu_lb_info")
        return {k: int(getattr(i, k)) for k, _ in _lib.LbInfo._fields_}

    def sessions_put(self, keys, values) -> None:
        """xsknf_gpu_lb_sessions_put: KEY_DTYPE / VALUE_DTYPE records into both
        session tables, in order.  Only with no batch in flight."""
        k, v = _records(keys, 16, "keys"), _records(values, 16, "values")
        if k.size != v.size:
            raise ValueError("one value per key")
        _lib.check(_lib.load().xsknf_gpu_lb_sessions_put(self.handle, k.ctypes.data if k.size else None,
                                                         v.ctypes.data if v.size else None, k.size),
                   "xsknf_gpu_lb_sessions_put")

    def sessions_dump(self, which: int = HOST_TABLE):
        """xsknf_gpu_lb_sessions_dump: (keys, values) of the host or the device
        table, ascending by key.  Waits for the device."""
        lib = _lib.load()
        n = ctypes.c_uint32(0)
        rc = lib.xsknf_gpu_lb_sessions_dump(self.handle, which, None, None, 0, ctypes.byref(n))
        if rc not in (0, -errno.ENOSPC):
            _lib.check(rc, "xsknf_gpu_lb_sessions_dump")
        k, v = np.zeros(int(n.value), dtype=KEY_DTYPE), np.zeros(int(n.value), dtype=VALUE_DTYPE)
        if k.size:
            _lib.check(lib.xsknf_gpu_lb_sessions_dump(self.handle, which, k.ctypes.data, v.ctypes.data, k.size,
                                                      ctypes.byref(n)), "xsknf_gpu_lb_sessions_dump")
        return k, v

    def _device_result(self, stream):
        """(result tensor, stream handle) of a device removal: two int64 words
        on the current device, and `stream` (a torch stream, a raw handle, or
        None for the current stream)."""
        import torch

        res = torch.empty(_lib.LB_REMOVE_RESULT, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        if stream is None:
            stream = torch.cuda.current_stream()
        return res, int(getattr(stream, "cuda_stream", stream))

    def sessions_remove(self, keys, *, pair: bool = False, which: int = DEVICE_TABLE, stream=None):
        """xsknf_gpu_lb_sessions_remove (which == DEVICE_TABLE) or _remove_host:
        the listed KEY_DTYPE records leave one session table, with `pair` also
        each one's partner -- the other half of its flow -- where the table
        holds it as such.  Returns the two result words (REMOVED, COMPACTED):
        for the host table a uint64 array; for the device table an int64
        device tensor that is written on `stream` (default: the current
        stream of the current device, which must be the object's) -- nothing
        waits for it."""
        k = _records(keys, 16, "keys")
        flags = _lib.LB_REMOVE_PAIR if pair else 0
        kp = k.ctypes.data if k.size else None
        if which == HOST_TABLE:
            res = np.zeros(_lib.LB_REMOVE_RESULT, dtype=np.uint64)
            _lib.check(_lib.load().xsknf_gpu_lb_sessions_remove_host(self.handle, kp, k.size, flags, res.ctypes.data),
                       "xsknf_gpu_lb_sessions_remove_host")
            return res
        if which != DEVICE_TABLE:
            raise ValueError("which must be HOST_TABLE or DEVICE_TABLE")
        res, s = self._device_result(stream)
        _lib.check(_lib.load().xsknf_gpu_lb_sessions_remove(self.handle, kp, k.size, flags, res.data_ptr(),
                                                            ctypes.c_void_p(s or None)), "xsknf_gpu_lb_sessions_remove")
        return res

    def drain_backend(self, addr: int, port: int, proto: int, *, which: int = DEVICE_TABLE, stream=None):
        """xsknf_gpu_lb_drain_backend / _drain_backend_host: both halves of
        every flow of backend (addr, port, proto) leave one session table.
        Returns the result words as `sessions_remove` does."""
        if which == HOST_TABLE:
            res = np.zeros(_lib.LB_REMOVE_RESULT, dtype=np.uint64)
            _lib.check(_lib.load().xsknf_gpu_lb_drain_backend_host(self.handle, addr, port, proto, res.ctypes.data),
                       "xsknf_gpu_lb_drain_backend_host")
            return res
        if which != DEVICE_TABLE:
            raise ValueError("which must be HOST_TABLE or DEVICE_TABLE")
        res, s = self._device_result(stream)
        _lib.check(_lib.load().xsknf_gpu_lb_drain_backend(self.handle, addr, port, proto, res.data_ptr(),
                                                          ctypes.c_void_p(s or None)), "xsknf_gpu_lb_drain_backend")
        return res

    def _has_device_half(self) -> bool:
        if self._device_half is None:
            self._device_half = self.info["device_bytes"] != 0
        return self._device_half

    def backends_update(self, add=None, remove=None, *, ops=None, stream=None) -> None:
        """xsknf_gpu_lb_backends_update: edit the services and backends of the
        live object.  Either `ops`, BACKEND_OP_DTYPE records applied in order,
        or BACKEND_DTYPE records to `remove` and to `add`, the removals first.
        The host copy is new when the call returns; the device copy follows on
        `stream` (default: the current stream of the current device, which
        must be the object's), and nothing waits for it.  A host-only object
        ignores `stream`."""
        if ops is not None:
            if add is not None or remove is not None:
                raise ValueError("give ops, or add and remove, not both")
            o = _records(ops, 28, "ops")
        else:
            parts = []
            for recs, op in ((remove, BACKEND_REMOVE), (add, BACKEND_ADD)):
                if recs is None:
                    continue
                r = _records(recs, 24, "backends")
                part = np.zeros(r.size, dtype=BACKEND_OP_DTYPE)
                part["backend"] = r.view(BACKEND_DTYPE)
                part["op"] = op
                parts.append(part)
            o = np.concatenate(parts) if parts else np.zeros(0, dtype=BACKEND_OP_DTYPE)
        s = 0
        if o.size and self._has_device_half():
            import torch

            s = int(getattr(stream, "cuda_stream", stream)) if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().xsknf_gpu_lb_backends_update(self.handle, o.ctypes.data if o.size else None, o.size,
                                                            ctypes.c_void_p(s or None)), "xsknf_gpu_lb_backends_update")

    def backends_dump(self, which: int = HOST_TABLE) -> np.ndarray:
        """xsknf_gpu_lb_backends_dump: the BACKEND_DTYPE records of the host or
        the device copy, services ascending, a service's backends by number.
        The device form waits for the device."""
        lib = _lib.load()
        n = ctypes.c_uint32(0)
        rc = lib.xsknf_gpu_lb_backends_dump(self.handle, which, None, 0, ctypes.byref(n))
        if rc not in (0, -errno.ENOSPC):
            _lib.check(rc, "xsknf_gpu_lb_backends_dump")
        r = np.zeros(int(n.value), dtype=BACKEND_DTYPE)
        if r.size:
            _lib.check(lib.xsknf_gpu_lb_backends_dump(self.handle, which, r.ctypes.data, r.size, ctypes.byref(n)),
                       "xsknf_gpu_lb_backends_dump")
        return r

    def drain_backends(self, ids, *, which: int = DEVICE_TABLE, stream=None):
        """xsknf_gpu_lb_drain_backends / _drain_backends_host: both halves of
        every flow of every listed backend (BACKEND_ID_DTYPE records) leave one
        session table, in one pass over it.  Returns the result words as
        `drain_backend` does.  To take backends out of service, call
        `backends_update(remove=...)` first and this on the same stream."""
        i = _records(ids, 8, "ids")
        ip = i.ctypes.data if i.size else None
        if which == HOST_TABLE:
            res = np.zeros(_lib.LB_REMOVE_RESULT, dtype=np.uint64)
            _lib.check(_lib.load().xsknf_gpu_lb_drain_backends_host(self.handle, ip, i.size, res.ctypes.data),
                       "xsknf_gpu_lb_drain_backends_host")
            return res
        if which != DEVICE_TABLE:
            raise ValueError("which must be HOST_TABLE or DEVICE_TABLE")
        res, s = self._device_result(stream)
        _lib.check(_lib.load().xsknf_gpu_lb_drain_backends(self.handle, ip, i.size, res.data_ptr(),
                                                           ctypes.c_void_p(s or None)), "xsknf_gpu_lb_drain_backends")
        return res

    def aging_enable(self) -> None:
        """xsknf_gpu_lb_aging_enable: a last-seen stamp per session and a clock
        per table, from now on (rule 11).  Only with no batch in flight; a
        second call changes nothing."""
        _lib.check(_lib.load().xsknf_gpu_lb_aging_enable(self.handle), "xsknf_gpu_lb_aging_enable")

    def clock(self, now: int, *, which: int = DEVICE_TABLE, stream=None) -> None:
        """xsknf_gpu_lb_clock: one table's clock becomes `now` (uint32, the
        caller's unit); the device table's on `stream` (default: the current
        stream), in order with the batches there, waiting for nothing."""
        s = 0
        if which == DEVICE_TABLE and self._has_device_half():
            import torch

            s = int(getattr(stream, "cuda_stream", stream)) if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().xsknf_gpu_lb_clock(self.handle, which, now & 0xffffffff, ctypes.c_void_p(s or None)),
                   "xsknf_gpu_lb_clock")

    def expire(self, max_idle: int, *, which: int = DEVICE_TABLE, stream=None):
        """xsknf_gpu_lb_sessions_expire / _expire_host: every flow whose
        sessions have all been idle for more than `max_idle` ticks of the
        table's clock leaves one session table.  Returns the result words as
        `sessions_remove` does."""
        if which == HOST_TABLE:
            res = np.zeros(_lib.LB_REMOVE_RESULT, dtype=np.uint64)
            _lib.check(_lib.load().xsknf_gpu_lb_sessions_expire_host(self.handle, max_idle, res.ctypes.data),
                       "xsknf_gpu_lb_sessions_expire_host")
            return res
        if which != DEVICE_TABLE:
            raise ValueError("which must be HOST_TABLE or DEVICE_TABLE")
        if not self._has_device_half():   # (no tensor to make: the call itself says -EINVAL or -ENODEV)
            _lib.check(_lib.load().xsknf_gpu_lb_sessions_expire(self.handle, max_idle, None, None),
                       "xsknf_gpu_lb_sessions_expire")
        res, s = self._device_result(stream)
        _lib.check(_lib.load().xsknf_gpu_lb_sessions_expire(self.handle, max_idle, res.data_ptr(),
                                                            ctypes.c_void_p(s or None)), "xsknf_gpu_lb_sessions_expire")
        return res

    def sessions_ages(self, which: int = HOST_TABLE):
        """xsknf_gpu_lb_sessions_ages: (keys, ages uint32, clock) of the host or
        the device table, ascending by key as `sessions_dump`; an age is the
        table's clock minus the session's stamp.  Waits for the device."""
        lib = _lib.load()
        n, clock = ctypes.c_uint32(0), ctypes.c_uint32(0)
        rc = lib.xsknf_gpu_lb_sessions_ages(self.handle, which, None, None, 0, ctypes.byref(n), ctypes.byref(clock))
        if rc not in (0, -errno.ENOSPC):
            _lib.check(rc, "xsknf_gpu_lb_sessions_ages")
        k, a = np.zeros(int(n.value), dtype=KEY_DTYPE), np.zeros(int(n.value), dtype=np.uint32)
        if k.size:
            _lib.check(lib.xsknf_gpu_lb_sessions_ages(self.handle, which, k.ctypes.data, a.ctypes.data, k.size,
                                                      ctypes.byref(n), ctypes.byref(clock)), "xsknf_gpu_lb_sessions_ages")
        return k, a, int(clock.value)

    def sessions_clear(self, which: int, *, stream=None) -> None:
        """xsknf_gpu_lb_sessions_clear: every session of one table; the device
        table's on `stream` (default: the current stream), waiting for nothing."""
        s = 0
        if which == DEVICE_TABLE:
            import torch

            s = int(getattr(stream, "cuda_stream", stream)) if stream is not None else torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().xsknf_gpu_lb_sessions_clear(self.handle, which, ctypes.c_void_p(s or None)),
                   "xsknf_gpu_lb_sessions_clear")

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, 0
            _lib.check(_lib.load().xsknf_gpu_lb_destroy(h), "xsknf_gpu_lb_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


def lb_workspace(n: int) -> int:
    """xsknf_gpu_lb_workspace: the bytes of device workspace a batch of n frames needs."""
    b = ctypes.c_uint64(0)
    _lib.check(_lib.load().xsknf_gpu_lb_workspace(n, ctypes.byref(b)), "xsknf_gpu_lb_workspace")
    return int(b.value)


def lb_host(umem, descs, lb: LoadBalancer, ingress_ifindex: int = 0, num_interfaces: int = 1):
    """xsknf_gpu_lb_host on numpy arrays: `umem` (uint8, contiguous, writable)
    is rewritten IN PLACE over the host session table.  Returns (verdicts int32,
    stats uint64[8])."""
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
    _lib.check(_lib.load().xsknf_gpu_lb_host(up if n else None, umem.size, d.ctypes.data if n else None, n,
                                             ingress_ifindex, num_interfaces, lb.handle,
                                             v.ctypes.data if n else None, st.ctypes.data), "xsknf_gpu_lb_host")
    return v, st


def lb_batch_ptr(umem_ptr: int, umem_size: int, descs_ptr: int, n: int, ingress_ifindex: int, num_interfaces: int,
                 lb: LoadBalancer, verdicts_ptr: int, workspace_ptr: int, workspace_bytes: int, stats_ptr: int,
                 stream: int = 0) -> None:
    """Raw-pointer form of xsknf_gpu_lb_batch (device pointers; 0 = NULL), on
    the current device: only enqueues on `stream`."""
    _lib.check(_lib.load().xsknf_gpu_lb_batch(
        ctypes.c_void_p(umem_ptr or None), umem_size, ctypes.c_void_p(descs_ptr or None), n, ingress_ifindex,
        num_interfaces, lb.handle, ctypes.c_void_p(verdicts_ptr or None), ctypes.c_void_p(workspace_ptr or None),
        workspace_bytes, ctypes.c_void_p(stats_ptr or None), ctypes.c_void_p(stream or None)), "xsknf_gpu_lb_batch")


def lb_batch(umem, descs, lb: LoadBalancer, ingress_ifindex: int = 0, num_interfaces: int = 1, *, workspace=None,
             device=None):
    """xsknf_gpu_lb_batch on torch tensors, on the current stream of their
    device (the one `lb` was made on): `umem` a contiguous uint8 device tensor,
    rewritten IN PLACE; `descs` (n, 2) int64 / (n, 16) uint8, contiguous;
    `workspace` a uint8 device tensor of at least lb_workspace(n) bytes
    (default: a new one).  Returns (verdicts int32[n], stats int64[8]) as device
    tensors; nothing waits for the stream."""
    import torch

    if not umem.is_cuda or not descs.is_cuda:
        raise ValueError("umem and descs must be device tensors (lb_host is the CPU form)")
    if umem.dtype != torch.uint8 or not umem.is_contiguous():
        raise ValueError("umem must be a contiguous uint8 tensor")
    if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
        raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
    n = descs.numel() * descs.element_size() // 16
    dev = umem.device if device is None else torch.device(device)
    if umem.device != dev or descs.device != dev:
        raise ValueError("umem and descs must lie on the load balancer's device")
    need = lb_workspace(n)
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        elif (workspace.device != dev or workspace.dtype != torch.uint8 or not workspace.is_contiguous()
              or workspace.numel() < need):
            raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on the device")
        v = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.zeros(_lib.LB_STATS, dtype=torch.int64, device=dev)
        lb_batch_ptr(umem.data_ptr() if n else 0, umem.numel(), descs.data_ptr() if n else 0, n, ingress_ifindex,
                     num_interfaces, lb, v.data_ptr() if n else 0, workspace.data_ptr() if n else 0,
                     workspace.numel(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return v, st
