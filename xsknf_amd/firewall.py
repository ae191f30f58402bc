"""The firewall NF: a 5-tuple ACL lookup to one verdict per frame.

The reference's second NF with the per-frame callback
(examples/firewall/firewall_user.c:128-186): parse Ethernet / IPv4 / TCP or UDP,
look the 13-byte 5-tuple up in an exact-match ACL and return the rule's action
(-1 drops, anything else names a tx interface, 0 where no rule matches).  The
rules per frame are in include/xsknf_gpu.h ("the firewall NF").

`Acl` holds the table (xsknf_gpu_acl_*: xsknf_amd/csrc/acl.cpp), on the host and
on the device that was current when it was made; `Acl.update` puts, replaces
and deletes rules of the live table, on the device in stream order
(xsknf_gpu_acl_update); `Acl.counters_enable` gives every rule packet and byte
counters, one set for the host calls and one for the device calls, which
`Acl.counters` reads and `Acl.counters_clear` zeroes
(xsknf_gpu_acl_counters_*).  `firewall_batch` gives the
verdicts on the device for a UMEM and descriptors that lie there
(xsknf_gpu_firewall_batch; xsknf_amd/csrc/firewall_device.hip), `firewall_host`
on one CPU thread (xsknf_gpu_firewall_host: the model the device is held to).
The verdicts are what route.route_batch consumes; the UMEM is only read.
"""
from __future__ import annotations

import ctypes
import errno
import os

import numpy as np

from . import _lib

MAX_RULES = _lib.ACL_MAX_RULES
MAX_SLOTS = _lib.ACL_MAX_SLOTS
# struct xsknf_gpu_acl_rule: addresses and ports in network order, i.e. the
# frame's own bytes read as little-endian numbers
RULE_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("sport", "<u2"), ("dport", "<u2"), ("proto", "u1"),
                       ("pad", "u1", (3,)), ("action", "<i4")])
assert RULE_DTYPE.itemsize == 20
# struct xsknf_gpu_acl_op: a rule and what to do with it
PUT = _lib.ACL_PUT
DELETE = _lib.ACL_DELETE
OP_DTYPE = np.dtype([("rule", RULE_DTYPE), ("op", "<u4")])
assert OP_DTYPE.itemsize == 24
HOST_TABLE = _lib.ACL_HOST_TABLE
DEVICE_TABLE = _lib.ACL_DEVICE_TABLE
# struct xsknf_gpu_acl_counter: one rule's hits
COUNTER_DTYPE = np.dtype([("packets", "<u8"), ("bytes", "<u8")])
TOTALS = _lib.ACL_TOTALS    # frames, hits, misses, decided before the lookup


def make_ops(rules, op) -> np.ndarray:
    """OP_DTYPE records: every rule of `rules` with the same op."""
    r = np.ascontiguousarray(rules)
    if r.dtype.itemsize != 20 or r.ndim != 1:
        raise ValueError("rules must be a 1-d array of 20-byte struct xsknf_gpu_acl_rule records")
    ops = np.zeros(r.shape[0], dtype=OP_DTYPE)
    ops["rule"] = r.view(RULE_DTYPE)
    ops["op"] = op
    return ops


def parse_acl(path) -> np.ndarray:
    """xsknf_gpu_acl_parse: the reference's ACL text as RULE_DTYPE records (no GPU)."""
    lib = _lib.load()
    p = os.fsencode(path)
    n = ctypes.c_uint32(0)
    rc = lib.xsknf_gpu_acl_parse(p, None, 0, ctypes.byref(n))
    if rc not in (0, -errno.ENOSPC):
        _lib.check(rc, f"xsknf_gpu_acl_parse({path!r})")
    rules = np.zeros(int(n.value), dtype=RULE_DTYPE)
    if rules.size:
        _lib.check(lib.xsknf_gpu_acl_parse(p, rules.ctypes.data, rules.size, ctypes.byref(n)),
                   f"xsknf_gpu_acl_parse({path!r})")
    return rules


class Acl:
    """struct xsknf_gpu_acl: the rules as an open-addressing table, on the host
    and (where the process sees one) on the current device."""

    def __init__(self, handle: int):
        self._h = handle

    @classmethod
    def from_rules(cls, rules, slots: int = 0, *, device=None) -> "Acl":
        """rules: RULE_DTYPE records (any 20-byte records of that layout); the
        last rule of a key wins.  slots: 0 for the default, or a power of two
        greater than the number of distinct keys.  device: make it current for
        the upload (default: the current device)."""
        r = np.ascontiguousarray(rules)
        if r.dtype.itemsize != 20 or r.ndim != 1:
            raise ValueError("rules must be a 1-d array of 20-byte struct xsknf_gpu_acl_rule records")
        h = ctypes.c_void_p()

        def create():
            _lib.check(_lib.load().xsknf_gpu_acl_create(ctypes.byref(h), r.ctypes.data if r.size else None, r.size,
                                                        slots), "xsknf_gpu_acl_create")
        if device is None:
            create()
        else:
            import torch
            with torch.cuda.device(device):
                create()
        return cls(h.value)

    @classmethod
    def from_file(cls, path, slots: int = 0, *, device=None) -> "Acl":
        return cls.from_rules(parse_acl(path), slots, device=device)

    @property
    def handle(self) -> int:
        if not self._h:
            raise ValueError("the ACL is closed")
        return self._h

    @property
    def info(self) -> dict:
        """rules (live keys), slots, max_probe, tombstones, device_bytes."""
        i = _lib.AclInfo()
        _lib.check(_lib.load().xsknf_gpu_acl_info(self.handle, ctypes.byref(i)), "xsknf_gpu_acl_info")
        return {"rules": int(i.rules), "slots": int(i.slots), "max_probe": int(i.max_probe),
                "tombstones": int(i.tombstones), "device_bytes": int(i.device_bytes)}

    def update(self, puts=None, deletes=None, *, ops=None, stream=None) -> None:
        """xsknf_gpu_acl_update: `deletes` (RULE_DTYPE records whose keys go; the
        actions are ignored) and then `puts` (rules stored, or whose action
        replaces the key's), or `ops`, OP_DTYPE records applied in their order.
        The host table changes before the call returns; the device table on
        `stream`: a torch stream or a hipStream_t as an int, by default the
        current torch stream of the current device (the NULL stream for an ACL
        without a device table).  Only enqueues; a refused update
        (XsknfGpuError: -ENOSPC, -EINVAL) leaves both tables as they were."""
        if ops is not None:
            if puts is not None or deletes is not None:
                raise ValueError("give puts / deletes or ops, not both")
            o = np.ascontiguousarray(ops)
            if o.dtype.itemsize != 24 or o.ndim != 1:
                raise ValueError("ops must be a 1-d array of 24-byte struct xsknf_gpu_acl_op records")
        else:
            parts = [make_ops(deletes, DELETE)] if deletes is not None else []
            if puts is not None:
                parts.append(make_ops(puts, PUT))
            o = np.concatenate(parts) if parts else np.zeros(0, dtype=OP_DTYPE)
        if stream is None:
            s = 0
            if o.size and self.info["device_bytes"]:
                import torch
                s = torch.cuda.current_stream().cuda_stream
        else:
            s = int(getattr(stream, "cuda_stream", stream))
        _lib.check(_lib.load().xsknf_gpu_acl_update(self.handle, o.ctypes.data if o.size else None, o.size,
                                                    ctypes.c_void_p(s or None)), "xsknf_gpu_acl_update")

    def dump(self, device: bool = False) -> np.ndarray:
        """xsknf_gpu_acl_dump: the live rules of the host table or (waiting for
        the device) the device table as RULE_DTYPE records, ascending by
        (saddr, daddr, sport | dport << 16, proto)."""
        lib = _lib.load()
        which = DEVICE_TABLE if device else HOST_TABLE
        n = ctypes.c_uint32(0)
        rc = lib.xsknf_gpu_acl_dump(self.handle, which, None, 0, ctypes.byref(n))
        if rc not in (0, -errno.ENOSPC):
            _lib.check(rc, "xsknf_gpu_acl_dump")
        rules = np.zeros(int(n.value), dtype=RULE_DTYPE)
        if rules.size:
            _lib.check(lib.xsknf_gpu_acl_dump(self.handle, which, rules.ctypes.data, rules.size, ctypes.byref(n)),
                       "xsknf_gpu_acl_dump")
        return rules

    def counters_enable(self) -> None:
        """xsknf_gpu_acl_counters_enable: per-rule packet and byte counters and
        four totals from now on, one set on the host and one on the device
        (with no batch and no update in flight; idempotent)."""
        _lib.check(_lib.load().xsknf_gpu_acl_counters_enable(self.handle), "xsknf_gpu_acl_counters_enable")

    def counters(self, device: bool = False):
        """xsknf_gpu_acl_counters_dump: (rules, counters, totals) of the host set
        or (waiting for the device) the device set -- RULE_DTYPE records in
        dump()'s order, COUNTER_DTYPE records that belong to them one by one,
        and TOTALS uint64: frames, hits, misses, decided before the lookup."""
        lib = _lib.load()
        which = DEVICE_TABLE if device else HOST_TABLE
        n = ctypes.c_uint32(0)
        rc = lib.xsknf_gpu_acl_counters_dump(self.handle, which, None, None, 0, ctypes.byref(n), None)
        if rc not in (0, -errno.ENOSPC):
            _lib.check(rc, "xsknf_gpu_acl_counters_dump")
        rules = np.zeros(int(n.value), dtype=RULE_DTYPE)
        ctr = np.zeros(int(n.value), dtype=COUNTER_DTYPE)
        totals = np.zeros(TOTALS, dtype=np.uint64)
        _lib.check(lib.xsknf_gpu_acl_counters_dump(self.handle, which, rules.ctypes.data if rules.size else None,
                                                   ctr.ctypes.data if rules.size else None, rules.size, ctypes.byref(n),
                                                   totals.ctypes.data), "xsknf_gpu_acl_counters_dump")
        return rules, ctr, totals

    def counters_clear(self, device: bool = False, stream=None) -> None:
        """xsknf_gpu_acl_counters_clear: zero the host set at once, or the device
        set in the order of `stream` (as in update(): by default the current
        torch stream of the current device)."""
        s = 0
        if device:
            if stream is None:
                import torch
                s = torch.cuda.current_stream().cuda_stream
            else:
                s = int(getattr(stream, "cuda_stream", stream))
        _lib.check(_lib.load().xsknf_gpu_acl_counters_clear(self.handle, DEVICE_TABLE if device else HOST_TABLE,
                                                            ctypes.c_void_p(s or None)), "xsknf_gpu_acl_counters_clear")

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, 0
            _lib.check(_lib.load().xsknf_gpu_acl_destroy(h), "xsknf_gpu_acl_destroy")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


def firewall_host(umem, descs, acl: Acl) -> np.ndarray:
    """xsknf_gpu_firewall_host on numpy arrays (a uint8 UMEM, 16-byte descriptor
    records): one int32 verdict per descriptor."""
    u = np.ascontiguousarray(umem)
    if u.dtype != np.uint8:
        raise ValueError("umem must be uint8")
    d = np.ascontiguousarray(descs)
    if d.dtype.itemsize != 16:
        raise ValueError("descriptors must be struct xdp_desc records (16 bytes)")
    n = int(d.shape[0])
    v = np.zeros(n, dtype=np.int32)
    if n:
        # (an empty UMEM still needs an address: every descriptor is then outside it)
        up = u.ctypes.data if u.size else v.ctypes.data
        _lib.check(_lib.load().xsknf_gpu_firewall_host(up, u.size, d.ctypes.data, n, acl.handle, v.ctypes.data),
                   "xsknf_gpu_firewall_host")
    return v


def firewall_batch_ptr(umem_ptr: int, umem_size: int, descs_ptr: int, n: int, acl: Acl, verdicts_ptr: int,
                       stream: int = 0) -> None:
    """Raw-pointer form of xsknf_gpu_firewall_batch (device pointers; 0 = NULL),
    on the current device: only enqueues on `stream`."""
    _lib.check(_lib.load().xsknf_gpu_firewall_batch(
        ctypes.c_void_p(umem_ptr or None), umem_size, ctypes.c_void_p(descs_ptr or None), n, acl.handle,
        ctypes.c_void_p(verdicts_ptr or None), ctypes.c_void_p(stream or None)), "xsknf_gpu_firewall_batch")


def firewall_batch(umem, descs, acl: Acl, *, device=None):
    """xsknf_gpu_firewall_batch on torch tensors, on the current stream of their
    device (the one `acl` was made on): `umem` a contiguous uint8 device tensor,
    `descs` (n, 2) int64 / (n, 16) uint8, contiguous.  Returns the verdicts as an
    int32 device tensor of n entries; nothing waits for the stream."""
    import torch

    if not umem.is_cuda or not descs.is_cuda:
        raise ValueError("umem and descs must be device tensors (firewall_host is the CPU form)")
    if umem.dtype != torch.uint8 or not umem.is_contiguous():
        raise ValueError("umem must be a contiguous uint8 tensor")
    if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
        raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
    n = descs.numel() * descs.element_size() // 16
    dev = umem.device if device is None else torch.device(device)
    if umem.device != dev or descs.device != dev:
        raise ValueError("umem and descs must lie on the firewall's device")
    with torch.cuda.device(dev):
        v = torch.empty(n, dtype=torch.int32, device=dev)
        firewall_batch_ptr(umem.data_ptr() if n else 0, umem.numel(), descs.data_ptr() if n else 0, n, acl,
                           v.data_ptr() if n else 0, torch.cuda.current_stream(dev).cuda_stream)
    return v
