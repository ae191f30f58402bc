"""Host-side mirror of the reference checksummer NF over the gfx950 batch path.

Reference: examples/checksummer/checksummer_user.c
  * enum action {REDIRECT, DROP}                        :15-18
  * opt_action / opt_csum_iterations                    :24-25
  * xsknf_packet_processor(pkt, len, ingress_ifindex)   :30-112 (per frame)
  * parse_command_line(), getopt "qxai:c:"              :139-175
(The library options, src/xsknf.c:777-874, are parsed by the runtime's own C
xsknf_parse_args(): runtime.parse_args() binds it; there is one parser.)

The per-frame callback becomes `Checksummer.process_batch()`: one call per rx
batch, device-resident UMEM + descriptors, verdicts with the callback's meaning
(-1 drop, else tx interface).  Everything runs in libxsknf_gpu.so; there is no
CPU fallback (a missing library raises at construction).
"""
from __future__ import annotations

import ctypes
import getopt
import sys
from dataclasses import dataclass
from typing import List, Optional

from . import _lib

ACTION_REDIRECT = _lib.ACTION_REDIRECT
ACTION_DROP = _lib.ACTION_DROP

_APP_USAGE = (
    "usage: %s [xsknf library options] -- [checksummer options]\n"
    "checksummer options:\n"
    "  -c, --action=REDIRECT|DROP   send each checksummed frame on (default) or drop it\n"
    "  -i, --csum-iterations=N      sum the UDP payload N times (default 1)\n"
    "  -q, --quiet                  no per-second statistics\n"
    "  -x, --extra-stats            also the ring counters\n"
    "  -a, --app-stats              also the syscall counters\n")


def _usage_exit(prog: str) -> None:
    sys.stderr.write(_APP_USAGE % prog)
    sys.exit(1)   # EXIT_FAILURE, as usage() does at checksummer_user.c:136


@dataclass
class ChecksummerOptions:
    """The checksummer app globals (checksummer_user.c:20-25)."""
    action: int = ACTION_REDIRECT
    csum_iterations: int = 1
    quiet: bool = False
    extra_stats: bool = False
    app_stats: bool = False


def _atoi(s: str) -> int:
    """C atoi(): leading whitespace, optional sign, digits; 0 if none."""
    s = s.lstrip()
    i, sign = 0, 1
    if i < len(s) and s[i] in "+-":
        sign = -1 if s[i] == "-" else 1
        i += 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    v = int(s[i:j]) if j > i else 0
    v *= sign
    return ((v + 2**31) % 2**32) - 2**31


def parse_command_line(argv: List[str], prog: str = "checksummer") -> ChecksummerOptions:
    """Mirror of parse_command_line() (checksummer_user.c:139-175).

    `argv` are the APP options (after `--`).  An invalid action prints what
    was wrong plus the option summary and exits with status 1, like the
    reference.  The reference declares --csum-iterations as no_argument
    (:116) so only `-i N` works there; here the long form requires an argument
    rather than crashing on atoi(NULL)."""
    o = ChecksummerOptions()
    try:
        opts, _ = getopt.getopt(argv, "qxai:c:",
                                ["action=", "csum-iterations=", "quiet", "extra-stats", "app-stats"])
    except getopt.GetoptError:
        _usage_exit(prog)
    for k, v in opts:
        if k in ("-c", "--action"):
            if v == "REDIRECT":
                o.action = ACTION_REDIRECT
            elif v == "DROP":
                o.action = ACTION_DROP
            else:
                sys.stderr.write(f"checksummer: action '{v}' is neither REDIRECT nor DROP\n")
                _usage_exit(prog)
        elif k in ("-i", "--csum-iterations"):
            o.csum_iterations = _atoi(v)
        elif k in ("-q", "--quiet"):
            o.quiet = True
        elif k in ("-x", "--extra-stats"):
            o.extra_stats = True
        elif k in ("-a", "--app-stats"):
            o.app_stats = True
    return o


class Checksummer:
    """The checksummer NF bound to the gfx950 batch kernel.

    `process_batch` replaces the per-frame loop of process_batch_1if
    (src/xsknf.c:654-672): for every descriptor it performs exactly
    xsknf_packet_processor(umem + addr, len, ingress) -- the UDP check is
    rewritten in place in `umem` and the verdict stored in `verdicts`."""

    def __init__(self, options: Optional[ChecksummerOptions] = None, num_interfaces: int = 1,
                 frame_len_hint: int = 0, frame_len_mean: int = 0):
        self.options = options or ChecksummerOptions()
        self.num_interfaces = int(num_interfaces)
        self.frame_len_hint = int(frame_len_hint)     # longest frame (0 = unknown)
        self.frame_len_mean = int(frame_len_mean)     # mean length (0 = unknown): for the launch shape choice
        self._lib = _lib.load()

    def csum_opts(self) -> _lib.CsumOpts:
        return _lib.CsumOpts(int(self.options.csum_iterations), int(self.options.action),
                             self.num_interfaces, 0)

    def process_batch_ptr(self, umem_ptr: int, umem_size: int, descs_ptr: int, n: int,
                          verdicts_ptr: int, ingress_ifindex: int = 0, stream: int = 0,
                          frame_len_hint: Optional[int] = None) -> None:
        """Raw-pointer form (device pointers), asynchronous on `stream`.  The
        options and `ingress_ifindex` are this launch's arguments: launches in
        flight on other streams, from Checksummers with other options, keep theirs."""
        hint = self.frame_len_hint if frame_len_hint is None else int(frame_len_hint)
        opts = self.csum_opts()
        rc = self._lib.xsknf_gpu_checksum_batch_lens(
            ctypes.c_void_p(umem_ptr), umem_size, ctypes.c_void_p(descs_ptr), n,
            ingress_ifindex, ctypes.byref(opts), ctypes.c_void_p(verdicts_ptr), hint, self.frame_len_mean,
            ctypes.c_void_p(stream or None))
        _lib.check(rc, "xsknf_gpu_checksum_batch_lens")

    def launch_cfg(self, frame_len_hint: Optional[int] = None) -> "_lib.LaunchCfg":
        """The launch shape process_batch uses (xsknf_gpu_launch_cfg_for_lens)."""
        hint = self.frame_len_hint if frame_len_hint is None else int(frame_len_hint)
        cfg = _lib.LaunchCfg()
        _lib.check(self._lib.xsknf_gpu_launch_cfg_for_lens(hint, self.frame_len_mean, ctypes.byref(cfg)),
                   "xsknf_gpu_launch_cfg_for_lens")
        return cfg

    def process_batch(self, umem, descs, ingress_ifindex: int = 0, verdicts=None,
                      frame_len_hint: Optional[int] = None, stream=None):
        """Torch-tensor form: `umem` uint8 and `descs` (n,2) int64 / (n,16) uint8
        tensors on the same GPU.  Returns the int32 verdict tensor."""
        import torch

        if not umem.is_cuda or not descs.is_cuda:
            raise ValueError("umem and descs must be device tensors (no CPU path)")
        if umem.dtype != torch.uint8 or not umem.is_contiguous():
            raise ValueError("umem must be a contiguous uint8 tensor")
        if not descs.is_contiguous() or descs.numel() * descs.element_size() % 16:
            raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
        n = descs.numel() * descs.element_size() // 16
        if verdicts is None:
            verdicts = torch.empty(n, dtype=torch.int32, device=umem.device)
        elif verdicts.dtype != torch.int32 or verdicts.numel() < n or not verdicts.is_contiguous():
            raise ValueError("verdicts must be a contiguous int32 tensor with >= n entries")
        if stream is None:
            stream = torch.cuda.current_stream(umem.device)
        with torch.cuda.device(umem.device):
            self.process_batch_ptr(umem.data_ptr(), umem.numel(), descs.data_ptr(), n,
                                   verdicts.data_ptr(), ingress_ifindex, stream.cuda_stream,
                                   frame_len_hint)
        return verdicts

    def route(self, descs, verdicts, order: bool = False):
        """The other half of the batch loop (src/xsknf.c:503-522, :654-672), on
        the device: the batch's frames filed by the verdicts process_batch left,
        one tx list per interface of this object and the fill list of the drops
        (route.route_batch: tx_descs, fill_addrs, order or None, counts)."""
        from . import route as _route

        return _route.route_batch(descs, verdicts, self.num_interfaces, order=order)

    def forward(self, rx_umem, tx_umems, tx_descs, counts, *, n=None):
        """The copy that ends the batch loop (src/xsknf.c:563-571), on the
        device: every frame of route()'s tx lists whose interface has a UMEM of
        its own (tx_umems[i], a uint8 device tensor; None: it shares rx_umem) is
        copied there at the same offset (route.forward_frames: the stats)."""
        from . import route as _route

        if len(tx_umems) != self.num_interfaces:
            raise ValueError("one UMEM (or None) per interface")
        return _route.forward_frames(rx_umem, tx_umems, tx_descs, counts, n=n)


class HostPath:
    """The batch hook with the UMEM in host memory (include/xsknf_gpu.h
    xsknf_gpu_ctx_*): what an AF_XDP worker (src/xsknf.c:716-742) holds to run
    its per-frame loop (:654-672) on the GPU.  `umem` is a host numpy uint8
    array (the worker's mmap), pinned while registered; `process_batch` takes
    host descriptors (DESC_DTYPE) and returns host int32 verdicts, with the check
    bytes rewritten in `umem`.  path: "zerocopy", "staged" or "resident" (zero-copy,
    every batch through the resident kernel's ring: no launch per batch).

    The options and the ingress interface belong to a BATCH, not to the
    context: `process_batch` and `submit` hand the C call its `opts` and
    `ingress_ifindex` arguments per call, and batches in flight together may
    each carry their own (a worker with two interfaces alternates ingress batch
    by batch, src/xsknf.c:716-742).  `opts` (a `_lib.CsumOpts`: iterations,
    action, num_interfaces) defaults to the Checksummer's own."""

    PATHS = {"zerocopy": _lib.PATH_ZEROCOPY, "staged": _lib.PATH_STAGED, "resident": _lib.PATH_RESIDENT}

    def __init__(self, checksummer: Checksummer, umem, *, path: str = "zerocopy",
                 max_batch: int = 1 << 20, device: int = 0):
        import numpy as np

        if umem.dtype != np.uint8 or not umem.flags.c_contiguous:
            raise ValueError("umem must be a contiguous uint8 numpy array")
        self.cs = checksummer
        self.umem = umem
        self.max_batch = int(max_batch)
        self._pending = []   # (ticket, descs, verdicts) submitted and not yet waited for
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        _lib.check(self._lib.xsknf_gpu_ctx_create(ctypes.byref(self._ctx), device, self.PATHS[path],
                                                  self.max_batch, checksummer.frame_len_hint),
                   "xsknf_gpu_ctx_create")
        try:
            _lib.check(self._lib.xsknf_gpu_ctx_register_umem(self._ctx, umem.ctypes.data, umem.nbytes),
                       "xsknf_gpu_ctx_register_umem")
        except Exception:
            self.close()
            raise

    def process_batch(self, descs, ingress_ifindex: int = 0, verdicts=None,
                      opts: Optional[_lib.CsumOpts] = None):
        """One batch, waited for.  `ingress_ifindex` and `opts` are this batch's
        own (opts None: the Checksummer's)."""
        import numpy as np

        if descs.dtype.itemsize != 16 or not descs.flags.c_contiguous:
            raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
        n = int(descs.shape[0])
        if verdicts is None:
            verdicts = np.empty(n, dtype=np.int32)
        elif verdicts.dtype != np.int32 or verdicts.shape[0] < n or not verdicts.flags.c_contiguous:
            raise ValueError("verdicts must be a contiguous int32 array with >= n entries")
        if opts is None:
            opts = self.cs.csum_opts()
        _lib.check(self._lib.xsknf_gpu_ctx_process_batch(self._ctx, descs.ctypes.data, n,
                                                         ingress_ifindex, ctypes.byref(opts),
                                                         verdicts.ctypes.data),
                   "xsknf_gpu_ctx_process_batch")
        return verdicts

    def submit(self, descs, verdicts, ingress_ifindex: int = 0,
               opts: Optional[_lib.CsumOpts] = None) -> int:
        """Enqueue a batch (a launched context keeps five pieces in flight, a
        resident one eight; a submit past that waits for the oldest); returns its ticket.  The
        verdicts array and the batch's frames belong to the context until
        wait(ticket).  `ingress_ifindex` and `opts` are this batch's own (opts
        None: the Checksummer's); the batches in flight need not share them."""
        if descs.dtype.itemsize != 16 or not descs.flags.c_contiguous:
            raise ValueError("descs must be a contiguous array of 16-byte xdp_desc")
        n = int(descs.shape[0])
        if verdicts.dtype.itemsize != 4 or verdicts.dtype.kind != "i" or verdicts.shape[0] < n \
                or not verdicts.flags.c_contiguous:
            raise ValueError("verdicts must be a contiguous int32 array with >= n entries")
        if opts is None:
            opts = self.cs.csum_opts()
        t = ctypes.c_uint64()
        _lib.check(self._lib.xsknf_gpu_ctx_submit(self._ctx, descs.ctypes.data, n, ingress_ifindex,
                                                  ctypes.byref(opts), verdicts.ctypes.data, ctypes.byref(t)),
                   "xsknf_gpu_ctx_submit")
        self._pending.append((t.value, descs, verdicts))   # keep the arrays alive until waited for
        return t.value

    def wait(self, ticket: int) -> None:
        _lib.check(self._lib.xsknf_gpu_ctx_wait(self._ctx, ticket), "xsknf_gpu_ctx_wait")
        self._pending = [p for p in self._pending if p[0] > ticket]

    def stats(self) -> dict:
        st = _lib.CtxStats()
        _lib.check(self._lib.xsknf_gpu_ctx_get_stats(self._ctx, ctypes.byref(st)), "xsknf_gpu_ctx_get_stats")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def close(self):
        if self._ctx:
            self._lib.xsknf_gpu_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
