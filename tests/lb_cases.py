"""Frames, services and the model for the load balancer NF's tests
(tests/test_lb.py, tests/test_gpu_lb.py).

The model is written from the rules in include/xsknf_gpu.h ("the load balancer
NF") with Python dicts as the maps: sessions {13 key bytes -> (dir, addr, port,
mac, ifindex)}, services {7 key bytes -> [backends]}.  It walks a batch in index
order, reads and writes a bytearray in the order of the reference's lines
521-550, and shares no code with xsknf_amd/csrc; jhash is restated here from its
public description (Bob Jenkins' lookup3 as the Linux kernel shapes it).
"""
import os
import re

import numpy as np

from tests import firewall_cases as FC
from xsknf_amd import frames, lb

ROOT = FC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "lb_golden.npz")
M32 = 0xffffffff


def code_constant(pattern, name="kernel_lb.h"):
    """A number the kernel's source states, by pattern."""
    src = open(os.path.join(ROOT, "xsknf_amd", "csrc", name)).read()
    return int(re.search(pattern, src).group(1))


# ---- the model ---------------------------------------------------------------

def _rol(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def jhash(key: bytes, initval: int = 0) -> int:
    """The kernel's jhash over `key` (any length)."""
    a = b = c = (0xdeadbeef + len(key) + initval) & M32
    k = key
    while len(k) > 12:
        a = (a + int.from_bytes(k[0:4], "little")) & M32
        b = (b + int.from_bytes(k[4:8], "little")) & M32
        c = (c + int.from_bytes(k[8:12], "little")) & M32
        a = (a - c) & M32; a ^= _rol(c, 4); c = (c + b) & M32
        b = (b - a) & M32; b ^= _rol(a, 6); a = (a + c) & M32
        c = (c - b) & M32; c ^= _rol(b, 8); b = (b + a) & M32
        a = (a - c) & M32; a ^= _rol(c, 16); c = (c + b) & M32
        b = (b - a) & M32; b ^= _rol(a, 19); a = (a + c) & M32
        c = (c - b) & M32; c ^= _rol(b, 4); b = (b + a) & M32
        k = k[12:]
    if not k:
        return c
    k = k + bytes(12 - len(k))
    a = (a + int.from_bytes(k[0:4], "little")) & M32
    b = (b + int.from_bytes(k[4:8], "little")) & M32
    c = (c + int.from_bytes(k[8:12], "little")) & M32
    c ^= b; c = (c - _rol(b, 14)) & M32
    a ^= c; a = (a - _rol(c, 11)) & M32
    b ^= a; b = (b - _rol(a, 25)) & M32
    c ^= b; c = (c - _rol(b, 16)) & M32
    a ^= c; a = (a - _rol(c, 4)) & M32
    b ^= a; b = (b - _rol(a, 14)) & M32
    c ^= b; c = (c - _rol(b, 24)) & M32
    return c


def _add(csum, addend):
    csum = (csum + addend) & M32
    return (csum + (1 if csum < addend else 0)) & M32


def _fold(csum):
    csum = (csum & 0xffff) + (csum >> 16)
    csum = (csum & 0xffff) + (csum >> 16)
    return ~csum & 0xffff


def _u16(f, i):
    return f[i] | f[i + 1] << 8


def _u32(f, i):
    return int.from_bytes(f[i:i + 4], "little")


def _update(f, nxt, proto, rep):
    """Lines 521-550 on the bytearray f, in their order."""
    direction, addr, port, mac, ifindex = rep
    apos, ppos = (30, nxt + 2) if direction == lb.TO_BACKEND else (26, nxt)
    old_addr = _u32(f, apos)
    f[apos:apos + 4] = addr.to_bytes(4, "little")
    old_port = _u16(f, ppos)
    f[ppos:ppos + 2] = port.to_bytes(2, "little")
    f[6:12] = f[0:6]
    f[0:6] = mac
    csum = ~_u16(f, 24) & M32
    csum = _add(csum, ~old_addr & M32)
    csum = _add(csum, addr)
    f[24:26] = _fold(csum).to_bytes(2, "little")
    cpos = nxt + (16 if proto == 6 else 6)
    csum = ~_u16(f, cpos) & M32
    csum = _add(csum, ~old_addr & M32)
    csum = _add(csum, addr)
    csum = _add(csum, ~old_port & M32)   # the complement of the PROMOTED port
    csum = _add(csum, port)
    f[cpos:cpos + 2] = _fold(csum).to_bytes(2, "little")
    return ifindex


class Model:
    """The loop with dicts.  sessions keeps insertion state across batches."""

    def __init__(self, backends, max_sessions):
        self.services = {}
        for r in backends:
            k = int(r["vaddr"]).to_bytes(4, "little") + int(r["vport"]).to_bytes(2, "little") + bytes([int(r["proto"])])
            self.services.setdefault(k, []).append((int(r["addr"]), int(r["port"]), bytes(r["mac"]), int(r["ifindex"])))
        self.sessions = {}
        self.max_sessions = max_sessions
        self.backend_choices = []   # (sid, index) of every new flow, in order

    def put(self, key: bytes, rep) -> bool:
        if key not in self.sessions and len(self.sessions) >= self.max_sessions:
            return False
        self.sessions[key] = rep
        return True

    def sessions_put(self, keys, values):
        for k, v in zip(keys, values):
            assert self.put(key_bytes(k), (int(v["dir"]), int(v["addr"]), int(v["port"]), bytes(v["mac"]),
                                           int(v["ifindex"])))

    def batch(self, umem, descs, ingress, nif):
        """Rewrites umem (numpy uint8) in place; returns (verdicts, stats)."""
        size = int(umem.size)
        st = dict.fromkeys(lb.LB_STATS, 0)
        st["frames"] = descs.shape[0]
        out = np.empty(descs.shape[0], dtype=np.int32)
        pas = (ingress + 1) % nif if nif > 1 else -1
        for i, (addr, ln) in enumerate(zip(descs["addr"].tolist(), descs["len"].tolist())):
            off = (addr & ((1 << 48) - 1)) + (addr >> 48)
            if not (off <= size and ln <= size - off):
                out[i] = -1
                st["dropped"] += 1
                continue
            f = bytearray(umem[off:off + ln].tobytes())
            v, key = FC.frame_key(f)
            if key is None:
                out[i] = pas if v == 0 else -1
                st["passed" if v == 0 else "dropped"] += 1
                continue
            nxt, proto = 14 + 4 * (f[14] & 15), f[23]
            rep = self.sessions.get(key)
            if rep is None:
                backs = self.services.get(key[4:8] + key[10:12] + key[12:13])
                if backs is None:
                    out[i] = pas
                    st["passed"] += 1
                    continue
                idx = jhash(key) % len(backs)
                self.backend_choices.append((key, idx))
                baddr, bport, bmac, bif = backs[idx]
                rep = (lb.TO_BACKEND, baddr, bport, bmac, bif)
                before = len(self.sessions)
                if not self.put(key, rep):
                    st["inserts_failed"] += 1
                else:
                    bkey = (baddr.to_bytes(4, "little") + key[0:4] + bport.to_bytes(2, "little") + key[8:10] +
                            key[12:13])
                    brep = (lb.TO_CLIENT, _u32(key, 4), _u16(key, 10), bytes(f[6:12]), ingress & 0xffff)
                    if not self.put(bkey, brep):
                        st["inserts_failed"] += 1
                st["sessions_created"] += len(self.sessions) - before
            out[i] = _update(f, nxt, proto, rep)
            st["rewritten"] += 1
            umem[off:off + ln] = np.frombuffer(bytes(f), dtype=np.uint8)
        return out, np.array([st[k] for k in lb.LB_STATS], dtype=np.uint64)

    def dump(self):
        """(keys, values) ascending as xsknf_gpu_lb_sessions_dump orders them."""
        items = sorted(self.sessions.items(), key=lambda kv: (_u32(kv[0], 0), _u32(kv[0], 4), _u32(kv[0], 8), kv[0][12]))
        k = np.zeros(len(items), dtype=lb.KEY_DTYPE)
        v = np.zeros(len(items), dtype=lb.VALUE_DTYPE)
        for i, (kb, rep) in enumerate(items):
            k[i] = (_u32(kb, 0), _u32(kb, 4), _u16(kb, 8), _u16(kb, 10), kb[12], (0, 0, 0))
            v[i] = (rep[1], rep[2], rep[4], tuple(rep[3]), rep[0], 0)
        return k, v


def key_bytes(k) -> bytes:
    return (int(k["saddr"]).to_bytes(4, "little") + int(k["daddr"]).to_bytes(4, "little") +
            int(k["sport"]).to_bytes(2, "little") + int(k["dport"]).to_bytes(2, "little") + bytes([int(k["proto"])]))


# ---- services, sessions and frames ---------------------------------------------

def make_backends(rng, services=6, per=(1, 7), ifaces=4):
    """`services` services (TCP and UDP alternating) with per[0]..per[1]-1
    backends each, the records of different services interleaved."""
    recs = []
    for s in range(services):
        vaddr, vport, proto = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 16)), 6 if s % 2 else 17
        for _ in range(int(rng.integers(per[0], per[1]))):
            recs.append((vaddr, vport, proto, 0, int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 16)),
                         tuple(rng.integers(0, 256, 6).tolist()), int(rng.integers(0, ifaces)), (0, 0)))
    order = rng.permutation(len(recs))
    return np.array([recs[i] for i in order], dtype=lb.BACKEND_DTYPE)


def session(saddr, daddr, sport, dport, proto, direction, addr, port, mac, ifindex):
    k = np.zeros(1, dtype=lb.KEY_DTYPE)
    v = np.zeros(1, dtype=lb.VALUE_DTYPE)
    k[0] = (saddr, daddr, sport, dport, proto, (0, 0, 0))
    v[0] = (addr, port, ifindex, tuple(mac), direction, 0)
    return k[0], v[0]


def frame(rng, sid, length=None, ihl=5, smac=None, zero_check=False):
    """A frame carrying sid = (saddr, daddr, sport, dport, proto) in the places
    the parse reads them for this ihl (for ihl < 5 they overlap: the later
    field wins and the frame's key is whatever then lies there)."""
    saddr, daddr, sport, dport, proto = sid
    nxt = 14 + 4 * ihl
    need = max(34, nxt + (20 if proto == 6 else 8))
    length = need + int(rng.integers(0, 30)) if length is None else length
    f = bytearray(FC.make_frame(rng, length, ihl, proto, True))
    if length >= 34:
        f[26:30] = saddr.to_bytes(4, "little")
        f[30:34] = daddr.to_bytes(4, "little")
    if length >= nxt + 4:
        f[nxt:nxt + 2] = sport.to_bytes(2, "little")
        f[nxt + 2:nxt + 4] = dport.to_bytes(2, "little")
    if length > 14:
        f[14] = (f[14] & 0xf0) | ihl
    if length > 23:
        f[23] = proto
    if smac is not None:
        f[6:12] = bytes(smac)
    if zero_check and proto == 17 and length >= nxt + 8:
        f[nxt + 6:nxt + 8] = b"\0\0"
    return bytes(f)


def frame_sid(f: bytes):
    """The sid the parse reads from f, or None."""
    v, key = FC.frame_key(f)
    return key


def sessions_for(frames_list, rng, every=2, ifaces=4):
    """Pre-populated sessions for every `every`-th candidate frame, directions
    alternating: (keys, values)."""
    ks, vs, seen, j = [], [], set(), 0
    for f in frames_list:
        key = frame_sid(f)
        if key is None or key in seen:
            continue
        seen.add(key)
        j += 1
        if j % every:
            continue
        k, v = session(_u32(key, 0), _u32(key, 4), _u16(key, 8), _u16(key, 10), key[12], (j // every) % 2,
                       int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), rng.integers(0, 256, 6).tolist(),
                       int(rng.integers(0, ifaces)))
        ks.append(k)
        vs.append(v)
    return np.array(ks, dtype=lb.KEY_DTYPE), np.array(vs, dtype=lb.VALUE_DTYPE)


def sweep_frames(rng, phases=range(16)):
    """Every branch x ihl 0..15 x TCP / UDP / other x all start phases: the
    firewall's decision sweep (lengths around every rule's edge) plus, per ihl
    and protocol, well-formed frames that reach the session lookup."""
    fl, ph = FC.decision_frames(rng, phases=phases)
    for ihl in range(16):
        for proto in (6, 17):
            for p in phases:
                sid = (int(rng.integers(1 << 32)), int(rng.integers(1 << 32)), int(rng.integers(1 << 16)),
                       int(rng.integers(1 << 16)), proto)
                fl.append(frame(rng, sid, ihl=ihl, zero_check=bool(p % 4 == 0)))
                ph.append(p)
    return fl, ph


def service_sid(rng, backends, svc_index=None, sport=None):
    """A fresh client sid towards one of the services in `backends`."""
    r = backends[int(rng.integers(backends.shape[0])) if svc_index is None else svc_index]
    return (int(rng.integers(1, 1 << 32)), int(r["vaddr"]), int(rng.integers(1, 1 << 16)) if sport is None else sport,
            int(r["vport"]), int(r["proto"]))


def backend_for(backends, sid):
    """The record the model picks for a new flow sid."""
    mine = [r for r in backends if int(r["vaddr"]) == sid[1] and int(r["vport"]) == sid[3] and int(r["proto"]) == sid[4]]
    key = (sid[0].to_bytes(4, "little") + sid[1].to_bytes(4, "little") + sid[2].to_bytes(2, "little") +
           sid[3].to_bytes(2, "little") + bytes([sid[4]]))
    return mine[jhash(key) % len(mine)]


def backward_sid(backends, sid):
    b = backend_for(backends, sid)
    return (int(b["addr"]), sid[0], int(b["port"]), sid[2], sid[4])


def flows_batch(rng, backends, flows=300, filler=200):
    """`flows` new flows of 1-5 frames each (differing source MACs, mixed ihl >=
    5 and protocol by service) interleaved with their backward frames, placed
    both before and after the flow's first frame, and filler that passes."""
    items = []
    for _ in range(flows):
        sid = service_sid(rng, backends)
        bsid = backward_sid(backends, sid)
        for _ in range(int(rng.integers(1, 6))):
            items.append(frame(rng, sid, ihl=int(rng.choice([5, 5, 6, 15])), zero_check=bool(rng.integers(4) == 0)))
        for _ in range(int(rng.integers(0, 4))):
            items.append(frame(rng, bsid, ihl=int(rng.choice([5, 7]))))
    for _ in range(filler):
        items.append(FC.make_frame(rng, int(rng.integers(0, 120)), 5, int(rng.choice([6, 17, 1])), bool(rng.integers(4))))
    order = rng.permutation(len(items))
    return [items[i] for i in order]


def pack_packed(frame_list, rng, phases=None):
    """Back to back with ZERO gap (a phase, where given, is reached by padding
    before the frame only when asked): each frame's last bytes and the next
    frame's MACs share words; the last frame ends on the UMEM's last byte."""
    return FC.pack_unaligned(frame_list, rng, phases, max_gap=0, tail=0)


def fixed_batch(rng, n, backends, length=64, flows=4000):
    """n 64-byte frames (ihl 5) in 64-byte slots: about a third each of frames of
    up to `flows` new flows towards the services, their backward traffic, and
    random filler."""
    fr = rng.integers(0, 256, (n, length), dtype=np.uint8)
    sids = [service_sid(rng, backends) for _ in range(max(1, min(flows, n // 9)))]
    both = np.array([[s, backward_sid(backends, s)] for s in sids], dtype=np.uint64)   # (flows, 2, 5)
    c = rng.integers(3, size=n)
    pick = both[rng.integers(len(sids), size=n), np.minimum(c, 1)]
    live = c < 2
    hdr = np.zeros((n, length), dtype=np.uint8)
    hdr[:, 12], hdr[:, 14] = 8, 0x45
    hdr[:, 23] = pick[:, 4]
    hdr[:, 26:30] = pick[:, 0].astype("<u4").view(np.uint8).reshape(n, 4)
    hdr[:, 30:34] = pick[:, 1].astype("<u4").view(np.uint8).reshape(n, 4)
    hdr[:, 34:36] = pick[:, 2].astype("<u2").view(np.uint8).reshape(n, 2)
    hdr[:, 36:38] = pick[:, 3].astype("<u2").view(np.uint8).reshape(n, 2)
    for lo, hi in ((12, 15), (23, 24), (26, 38)):
        fr[live, lo:hi] = hdr[live, lo:hi]
    descs = np.zeros(n, dtype=frames.DESC_DTYPE)
    descs["addr"] = np.arange(n, dtype=np.uint64) * length
    descs["len"] = length
    return fr.reshape(-1).copy(), descs


# ---- the three causes of the ordered path --------------------------------------

def _rec(vaddr, vport, proto, addr, port, mac, ifindex):
    return (vaddr, vport, proto, 0, addr, port, tuple(mac), ifindex, (0, 0))


def ordered_cause(rng, which, salt=0):
    """(backends, pre-populated (keys, values), frames) of a small batch whose
    result depends on the loop's order in exactly one way:
    "existing_b"  a new flow's backward key is already a stored session (which
                  an earlier frame of the batch uses and a later one finds replaced);
    "shared_b"    two flows (one client address and port, two services whose only
                  backends are the same address and port) store one backward key;
    "vip_client"  a service address acts as a client: its flow's backward key is
                  the forward key of a second flow.
    salt moves every address, so that several causes fit one set of services."""
    macs = rng.integers(0, 256, (8, 6)).tolist()
    v1, v2 = (0x0a00000a + salt, 0x5000, 17), (0x0b00000b + salt, 0x5100, 17)
    a1, p1 = 0xc0a80101 + salt, 0x901f
    recs = [_rec(*v1, a1, p1, macs[0], 1), _rec(*v2, a1 if which == "shared_b" else 0xc0a80202 + salt, p1, macs[1], 2)]
    backends = np.array(recs, dtype=lb.BACKEND_DTYPE)
    ks, vs, fl = [], [], []
    client = (0x01020304 + salt, 0x3930)
    if which == "existing_b":
        sid = (client[0], v1[0], client[1], v1[1], 17)
        bsid = (a1, client[0], p1, client[1], 17)
        k, v = session(*bsid, lb.TO_CLIENT, 0x09090909, 0x0707, macs[2], 3)
        ks, vs = [k], [v]
        fl = [frame(rng, bsid), frame(rng, sid, smac=macs[3]), frame(rng, bsid), frame(rng, sid, smac=macs[4])]
    elif which == "shared_b":
        s1 = (client[0], v1[0], client[1], v1[1], 17)
        s2 = (client[0], v2[0], client[1], v2[1], 17)
        bsid = (a1, client[0], p1, client[1], 17)
        fl = [frame(rng, bsid), frame(rng, s1, smac=macs[3]), frame(rng, bsid), frame(rng, s2, smac=macs[4]),
              frame(rng, bsid), frame(rng, s1, smac=macs[5])]
    else:
        s1 = (v2[0], v1[0], v2[1], v1[1], 17)     # the "client" is service 2's address and port
        s2 = (a1, v2[0], p1, v2[1], 17)           # == the backward key of s1, and it hits service 2
        fl = [frame(rng, s2, smac=macs[3]), frame(rng, s1, smac=macs[4]), frame(rng, s2, smac=macs[5]),
              frame(rng, s1, smac=macs[6])]
        if rng.integers(2):
            fl = fl[1:] + fl[:1]
    filler = [FC.make_frame(rng, 60, 5, 1, True) for _ in range(3)]
    return backends, (np.array(ks, dtype=lb.KEY_DTYPE), np.array(vs, dtype=lb.VALUE_DTYPE)), filler[:1] + fl + filler[1:]
