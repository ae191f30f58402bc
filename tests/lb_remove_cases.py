"""The model and the helpers of the session removal tests (tests/test_lb_remove.py,
tests/test_gpu_lb_remove.py): xsknf_gpu_lb_sessions_remove, _drain_backend and
_sessions_clear of include/xsknf_gpu.h.

The reference has no removal, so the model is the set semantics the header
states, over the dict of tests/lb_cases.py's Model: every decision is taken on a
copy of the table as it stood before the call, never on what the call has
already removed.  It also counts tombstones as the header says -- a removal
that leaves more than slots / 4 of them rebuilds -- so that the COMPACTED word
is checked exactly.  It shares no code with xsknf_amd/csrc.
"""
import numpy as np

from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from xsknf_amd import frames, lb

REMOVED, COMPACTED = 0, 1
HIT_IFACE = 1   # the ifindex of the sessions these tests store: not PASS (3), not the ingress (2)


def partner(key: bytes, rep) -> bytes:
    """The key of the other half of the flow of session key -> rep."""
    direction, addr, port = rep[0], rep[1].to_bytes(4, "little"), rep[2].to_bytes(2, "little")
    if direction == lb.TO_BACKEND:
        return addr + key[0:4] + port + key[8:10] + key[12:13]
    return key[4:8] + addr + key[10:12] + port + key[12:13]


class Model(LC.Model):
    """LC.Model with the removals and the tombstone count of a table of `slots` slots."""

    def __init__(self, backends, max_sessions, slots):
        super().__init__(backends, max_sessions)
        self.slots, self.tombstones = slots, 0

    def _settle(self, gone):
        for k in gone:
            del self.sessions[k]
        self.tombstones += len(gone)
        compacted = int(self.tombstones > self.slots // 4)
        if compacted:
            self.tombstones = 0
        return np.array([len(gone), compacted], dtype=np.uint64)

    def remove(self, keys, pair=False):
        """keys: KEY_DTYPE records.  Returns the expected result words."""
        before = dict(self.sessions)
        listed = {LC.key_bytes(k) for k in keys if int(k["proto"]) in (6, 17)}
        held = {k for k in listed if k in before}
        gone = set(held)
        if pair:
            for k in held:
                pk = partner(k, before[k])
                prep = before.get(pk)
                if prep is not None and prep[0] != before[k][0] and partner(pk, prep) == k:
                    gone.add(pk)
        return self._settle(gone)

    def drain(self, addr, port, proto):
        gone = set()
        for k, rep in self.sessions.items():
            if k[12] != proto:
                continue
            if rep[0] == lb.TO_BACKEND:
                hit = rep[1] == addr and rep[2] == port
            else:
                hit = LC._u32(k, 0) == addr and LC._u16(k, 8) == port
            if hit:
                gone.add(k)
        return self._settle(gone)

    def clear(self):
        self.sessions.clear()
        self.tombstones = 0


# ---- keys and frames ---------------------------------------------------------------

def sid_of(key):
    """(a, b, c, p) key words -> sid."""
    return (key[0], key[1], key[2] & 0xffff, key[2] >> 16, key[3])


def key_records(sids):
    """KEY_DTYPE records of sids (saddr, daddr, sport, dport, proto)."""
    k = np.zeros(len(sids), dtype=lb.KEY_DTYPE)
    for i, s in enumerate(sids):
        k[i] = (s[0], s[1], s[2], s[3], s[4], (0, 0, 0))
    return k


def stored(sids, direction=lb.TO_BACKEND):
    """Sessions for sids that lead nowhere in particular: (keys, values) whose
    verdict is HIT_IFACE and whose partner key no test stores."""
    pairs = [LC.session(*s, direction, 0x0d0d0d00 + i, 0x7000 + i, (1, 2, 3, 4, 5, 6), HIT_IFACE)
             for i, s in enumerate(sids)]
    return CC.sessions(pairs)


def frames_of(sids, seed=7):
    """One 64-byte frame per sid, in order: (umem, descs)."""
    b = CC.Batch(max(len(sids), 1), seed)
    for i, s in enumerate(sids):
        b.put(i, s, ("x", s))
    return b.arrays()


def fast_frames(sids, seed=8):
    """frames_of for thousands of sids (ihl 5, 64 bytes, random payload), built as arrays."""
    n = len(sids)
    s = np.array(sids, dtype=np.uint64).reshape(n, 5)
    fr = np.random.default_rng(seed).integers(0, 256, (n, 64), dtype=np.uint8)
    fr[:, 12], fr[:, 13], fr[:, 14] = 8, 0, 0x45
    fr[:, 23] = s[:, 4]
    fr[:, 26:30] = s[:, 0].astype("<u4").view(np.uint8).reshape(n, 4)
    fr[:, 30:34] = s[:, 1].astype("<u4").view(np.uint8).reshape(n, 4)
    fr[:, 34:36] = s[:, 2].astype("<u2").view(np.uint8).reshape(n, 2)
    fr[:, 36:38] = s[:, 3].astype("<u2").view(np.uint8).reshape(n, 2)
    descs = np.zeros(n, dtype=frames.DESC_DTYPE)
    descs["addr"] = np.arange(n, dtype=np.uint64) * 64
    descs["len"] = 64
    return fr.reshape(-1).copy(), descs


def chain_service(backends=1):
    """The service that chain_keys' sids address, with `backends` backends."""
    return np.array([(0x0b0b0b0b, 0x3500, 6, 0, 0xc0a80a01 + i, 0x1f90 + i, (2, 4, 6, 8, 10, 12 + i), HIT_IFACE, (0, 0))
                     for i in range(backends)], dtype=lb.BACKEND_DTYPE)


def new_flows(bk, count, seed):
    """`count` distinct client sids towards bk's first service."""
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < count:
        s = LC.service_sid(rng, bk, svc_index=0)
        out[(s[0], s[2])] = s
    return list(out.values())


def same_dump(L, M, which):
    k, v = L.sessions_dump(which)
    mk, mv = M.dump()
    return k.tobytes() == mk.tobytes() and v.tobytes() == mv.tobytes()


def chain_keys(kind):
    """Twelve keys of one probe chain of a 64-slot table: "home" all hash to one
    slot; "wrap" home in slots 62, 63, 0, 1, so the chain passes the table's end."""
    if kind == "home":
        home, keys = CC.same_home_keys(64, 12)
        assert {h & 63 for h in CC.hash_keys(keys)} == {home}
    else:
        keys = [CC.fwd_key(s) for s in CC.sids_towards(0x0b0b0b0b, 0x3500, 6, 64, 4, 12)]
        assert CC.chain_of(keys, 64).wraps >= 1
    assert CC.chain_of(keys, 64).longest >= 8
    return [sid_of(k) for k in keys]
