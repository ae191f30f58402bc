"""The model and the helpers of the live services' tests (tests/test_lb_backends.py,
tests/test_gpu_lb_backends.py): xsknf_gpu_lb_backends_update, _backends_dump and
_drain_backends of include/xsknf_gpu.h.

The reference loads its services once and has neither call, so the model is the
rules the header states: tests/lb_cases.py's Model, whose services are an ordered
{service: [backends]}, edited op by op; and the list drain as the union of
tests/lb_remove_cases.py's drain predicate over the listed backends, taken on the
table as it stood before the call.  It shares no code with xsknf_amd/csrc.
"""
import numpy as np

from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from xsknf_amd import lb

ADD, REMOVE = 0, 1
I, NIF = CC.INGRESS, CC.NIF
H, D = lb.HOST_TABLE, lb.DEVICE_TABLE


def rec(vaddr, vport, proto, addr, port, mac=(2, 4, 6, 8, 10, 12), ifindex=1):
    """One BACKEND_DTYPE record as a tuple."""
    return (vaddr, vport, proto, 0, addr, port, tuple(mac), ifindex, (0, 0))


def records(recs):
    return np.array(list(recs), dtype=lb.BACKEND_DTYPE)


def op_records(ops):
    """BACKEND_OP_DTYPE records of (op, record tuple) pairs."""
    o = np.zeros(len(ops), dtype=lb.BACKEND_OP_DTYPE)
    for i, (op, r) in enumerate(ops):
        o[i] = (r, op)
    return o


def id_records(ids):
    """BACKEND_ID_DTYPE records of (addr, port, proto) triples."""
    o = np.zeros(len(ids), dtype=lb.BACKEND_ID_DTYPE)
    for i, t in enumerate(ids):
        o[i] = (t[0], t[1], t[2], 0)
    return o


def svc_key(r) -> bytes:
    return int(r["vaddr"]).to_bytes(4, "little") + int(r["vport"]).to_bytes(2, "little") + bytes([int(r["proto"])])


class Model(RC.Model):
    """RC.Model whose services change: `services` is LC.Model's dict {7 key bytes
    -> [(addr, port, mac, ifindex)]}, a list's index being the backend number."""

    def update(self, ops):
        """ops: BACKEND_OP_DTYPE records, applied in index order."""
        for o in ops:
            r = o["backend"]
            k, addr, port = svc_key(r), int(r["addr"]), int(r["port"])
            backs = self.services.get(k)
            if int(o["op"]) == REMOVE:
                if backs is None:
                    continue
                backs[:] = [b for b in backs if (b[0], b[1]) != (addr, port)]
                if not backs:
                    del self.services[k]
                continue
            new = (addr, port, bytes(r["mac"]), int(r["ifindex"]))
            if backs is None:
                self.services[k] = [new]
            elif any((b[0], b[1]) == (addr, port) for b in backs):
                backs[:] = [new if (b[0], b[1]) == (addr, port) else b for b in backs]
            else:
                backs.append(new)

    def _records(self, keys):
        out = []
        for k in keys:
            for addr, port, mac, ifindex in self.services[k]:
                out.append(rec(LC._u32(k, 0), LC._u16(k, 4), k[6], addr, port, mac, ifindex))
        return np.array(out, dtype=lb.BACKEND_DTYPE) if out else np.zeros(0, dtype=lb.BACKEND_DTYPE)

    def record_list(self):
        """The edited list: what xsknf_gpu_lb_create makes the same object from."""
        return self._records(self.services)

    def backends_dump(self):
        """As xsknf_gpu_lb_backends_dump orders them."""
        return self._records(sorted(self.services, key=lambda k: (LC._u32(k, 0), LC._u16(k, 4) | k[6] << 16)))

    def drain_list(self, ids):
        """ids: BACKEND_ID_DTYPE records.  The expected result words."""
        gone = set()
        for t in ids:
            addr, port, proto = int(t["addr"]), int(t["port"]), int(t["proto"])
            for k, rep in self.sessions.items():   # (nothing is removed before every backend has looked)
                if k[12] != proto:
                    continue
                if rep[0] == lb.TO_BACKEND:
                    hit = rep[1] == addr and rep[2] == port
                else:
                    hit = LC._u32(k, 0) == addr and LC._u16(k, 8) == port
                if hit:
                    gone.add(k)
        return self._settle(gone)


def same_backends(L, M, which=H):
    got, want = L.backends_dump(which), M.backends_dump()
    return got.tobytes() == want.tobytes()


def flows_to(vaddr, vport, proto, count, seed):
    """`count` distinct client sids towards one service."""
    rng = np.random.default_rng(seed)
    out = {}
    while len(out) < count:
        s = (int(rng.integers(1, 1 << 32)), vaddr, int(rng.integers(1, 1 << 16)), vport, proto)
        out[(s[0], s[2])] = s
    return list(out.values())


def choice(sid, count):
    """The backend number rule 9 gives sid in a service of `count` backends."""
    return LC.jhash(CC.sid_bytes(sid)) % count


def colliding_services(count, vport=0x5000, proto=6, seed=31):
    """`count` service addresses whose {vaddr, vport | proto << 16} all home in
    one slot of the 2048-slot service table (acl_hash restated in
    tests/lb_collide_cases.py)."""
    rng = np.random.default_rng(seed)
    vaddr = np.unique(rng.integers(1, 1 << 32, 1 << 16, dtype=np.uint64))
    home = CC.acl_hash(vaddr, vport | proto << 16, 0, 0) & np.uint32(2047)
    best = int(np.bincount(home, minlength=2048).argmax())
    got = vaddr[home == best][:count].tolist()
    assert len(got) == count
    return [int(v) for v in got]


def backend_ids(recs):
    """The distinct (addr, port, proto) of BACKEND_DTYPE records or record tuples."""
    r = records(recs) if not isinstance(recs, np.ndarray) else recs
    return list(dict.fromkeys((int(x["addr"]), int(x["port"]), int(x["proto"])) for x in r))
