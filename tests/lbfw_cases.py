"""The model and the helpers for the lbfw NF's tests (tests/test_lbfw.py,
tests/test_gpu_lbfw.py): the load balancer's dict model (tests/lb_cases.py) plus
the two things include/xsknf_gpu.h ("the lbfw NF") adds -- lbfw's PASS value and
the ACL gate, a Python dict {13 key bytes -> action} as in
tests/firewall_cases.py.  It shares no code with xsknf_amd/csrc.
"""
import os

import numpy as np

from tests import firewall_cases as FC
from tests import lb_cases as LC
from xsknf_amd import lb, lbfw

ROOT = FC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "lbfw_golden.npz")
GATED = lbfw.LBFW_STATS.index("acl_decided")
ORDERED = lbfw.LBFW_STATS.index("ordered_batches")


class Model(LC.Model):
    """LC.Model's loop with PASS = (ingress + 1) % nif and, between the key and
    the session lookup, the gate: a key the ACL dict holds returns its action
    with nothing read or written any further."""

    def batch(self, umem, descs, ingress, nif, acl=None):
        """Rewrites umem (numpy uint8) in place; acl: {key bytes: action} or
        None.  Returns (verdicts, stats)."""
        assert nif > 0
        size = int(umem.size)
        st = dict.fromkeys(lbfw.LBFW_STATS, 0)
        st["frames"] = descs.shape[0]
        out = np.empty(descs.shape[0], dtype=np.int32)
        pas = (ingress + 1) % nif
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
            if acl is not None and key in acl:
                out[i] = acl[key]
                st["acl_decided"] += 1
                continue
            nxt, proto = 14 + 4 * (f[14] & 15), f[23]
            rep = self.sessions.get(key)
            if rep is None:
                backs = self.services.get(key[4:8] + key[10:12] + key[12:13])
                if backs is None:
                    out[i] = pas
                    st["passed"] += 1
                    continue
                idx = LC.jhash(key) % len(backs)
                self.backend_choices.append((key, idx))
                baddr, bport, bmac, bif = backs[idx]
                rep = (lb.TO_BACKEND, baddr, bport, bmac, bif)
                before = len(self.sessions)
                if not self.put(key, rep):
                    st["inserts_failed"] += 1
                else:
                    bkey = (baddr.to_bytes(4, "little") + key[0:4] + bport.to_bytes(2, "little") + key[8:10] +
                            key[12:13])
                    brep = (lb.TO_CLIENT, LC._u32(key, 4), LC._u16(key, 10), bytes(f[6:12]), ingress & 0xffff)
                    if not self.put(bkey, brep):
                        st["inserts_failed"] += 1
                st["sessions_created"] += len(self.sessions) - before
            out[i] = LC._update(f, nxt, proto, rep)
            st["rewritten"] += 1
            umem[off:off + ln] = np.frombuffer(bytes(f), dtype=np.uint8)
        return out, np.array([st[k] for k in lbfw.LBFW_STATS], dtype=np.uint64)


def sid_key(sid) -> bytes:
    """The 13 key bytes of sid = (saddr, daddr, sport, dport, proto)."""
    return (sid[0].to_bytes(4, "little") + sid[1].to_bytes(4, "little") + sid[2].to_bytes(2, "little") +
            sid[3].to_bytes(2, "little") + bytes([sid[4]]))


def flip(key: bytes, bit: int) -> bytes:
    """key with one of its first 96 bits (the addresses and ports) flipped."""
    return (int.from_bytes(key, "little") ^ (1 << bit)).to_bytes(13, "little")


def rules(keys, actions):
    """RULE_DTYPE records and the model's dict for the same rules."""
    r = FC.rules_from_keys(list(keys), list(actions))
    return r, FC.acl_dict(r)


def frame_keys(frame_list):
    """The distinct sids the parse reads from the frames, in order."""
    seen, out = set(), []
    for f in frame_list:
        k = LC.frame_sid(f)
        if k is not None and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def identity(st) -> bool:
    """[0] = [1] + [2] + [3] + [7]."""
    return int(st[0]) == int(st[1]) + int(st[2]) + int(st[3]) + int(st[GATED])


def golden_sessions(raw):
    """An (n, 31) dump of the reference's pool (struct session_id, struct
    replace_info) as (keys, values) in xsknf_gpu_lb_sessions_dump's order."""
    fk, fv = raw[:, :13], raw[:, 13:]
    k = np.zeros(fk.shape[0], dtype=lb.KEY_DTYPE)
    v = np.zeros(fk.shape[0], dtype=lb.VALUE_DTYPE)
    k.view(np.uint8).reshape(-1, 16)[:, :13] = fk
    r = v.view(np.uint8).reshape(-1, 16)
    r[:, 0:4] = fv[:, 4:8]      # addr
    r[:, 4:6] = fv[:, 8:10]     # port
    r[:, 6:8] = fv[:, 16:18]    # ifindex
    r[:, 8:14] = fv[:, 10:16]   # mac
    r[:, 14] = fv[:, 0]         # dir (an int of 0 or 1)
    assert not fv[:, 1:4].any()
    order = sorted(range(k.shape[0]), key=lambda i: (int(k[i]["saddr"]), int(k[i]["daddr"]),
                                                     int(k[i]["sport"]) | int(k[i]["dport"]) << 16, int(k[i]["proto"])))
    return k[order], v[order]


def run_golden(g, mode, call, dump):
    """The fixture's batches of `mode` ("afxdp": with the ACL, "combined":
    without) through call(b, umem, descs, ingress, nif) -> (umem after,
    verdicts); after every batch dump() -> (keys, values) must equal the
    reference's sessions."""
    for b in range(int(g["batches"])):
        umem = g[f"umem{b}"].copy()
        ingress, nif = (int(x) for x in g[f"params{b}"])
        after, verdicts = call(b, umem, g[f"descs{b}"], ingress, nif)
        want = g[f"{mode}_verdicts{b}"]
        bad = np.nonzero(verdicts != want)[0]
        assert bad.size == 0, f"{mode} batch {b}: verdicts differ at {bad[:8]}: {verdicts[bad[:8]]} != {want[bad[:8]]}"
        bad = np.nonzero(after != g[f"{mode}_after{b}"])[0]
        assert bad.size == 0, f"{mode} batch {b}: {bad.size} UMEM bytes differ, first at {bad[:8]}"
        k, v = dump()
        wk, wv = golden_sessions(g[f"{mode}_sessions{b}"])
        assert k.tobytes() == wk.tobytes() and v.tobytes() == wv.tobytes(), f"{mode} batch {b}: the sessions differ"
