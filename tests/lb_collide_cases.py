"""Keys chosen by their home slot, for the load balancer's collision tests
(tests/test_lb_collide.py, tests/test_gpu_lb_collide.py).

Every other test gives the session table and the staging table random keys:
chains of one to three slots that almost never reach the table's last slot.
Here the keys are searched for: client (saddr, sport) pairs towards one service
with one backend whose forward key S = {saddr, vaddr, sport | vport << 16,
proto}, whose backward key B = {baddr, saddr, bport | sport << 16, proto}, or
both, hash into a window of w home slots that straddles a table's end (homes
M - w/2 .. M - 1, 0 .. w/2 - 1).  A window of a table of M slots is also a
window of every smaller power-of-two table, so one set of flows clusters in
the batch's staging table and in the session table at once.

acl_hash is restated here from acl_table.h's description (xor the word in,
multiply by an odd constant, xor-shift the high bits down; four rounds) and
shares no code with xsknf_amd/csrc; tests/test_lb_collide.py anchors it to the
library.  Chain is plain linear probing in Python: the tests assert their own
premises (probe lengths, wraps) with it.
"""
import functools

import numpy as np

from tests import firewall_cases as FC
from tests import lb_cases as LC
from xsknf_amd import frames, lb

DRAWS = 1 << 22
U32 = np.uint32


# ---- the hash and the chain model ------------------------------------------------

def acl_hash(a, b, c, p) -> np.ndarray:
    """acl_table.h's hash over arrays of key words (uint32 arithmetic, wrapping)."""
    a, b, c, p = (np.atleast_1d(np.asarray(x, dtype=np.uint64)).astype(U32) for x in (a, b, c, p))
    h = a * U32(0x9E3779B1)
    h ^= h >> U32(15)
    h = (h ^ b) * U32(0x85EBCA77)
    h ^= h >> U32(13)
    h = (h ^ c) * U32(0xC2B2AE3D)
    h ^= h >> U32(16)
    h = (h ^ p) * U32(0x27D4EB2F)
    h ^= h >> U32(15)
    return h


def hash_keys(keys) -> list:
    """acl_hash of (a, b, c, p) tuples."""
    if not len(keys):
        return []
    k = np.array(keys, dtype=np.uint64)
    return acl_hash(k[:, 0], k[:, 1], k[:, 2], k[:, 3]).tolist()


def in_window(h, M, w):
    home = np.asarray(h) & (M - 1)
    return (home >= M - w // 2) | (home < w // 2)


class Chain:
    """Open addressing with linear probing over M slots, as lb_table.h and the
    staging table do it: a probe starts at hash & (M - 1) and walks up one slot
    at a time, wrapping.  The home slot counts as probe 1."""

    def __init__(self, M):
        assert M & (M - 1) == 0
        self.M, self.slots = M, {}
        self.longest, self.wraps = 0, 0

    def _walk(self, key):
        s = hash_keys([key])[0] & (self.M - 1)
        probes, wrapped = 1, False
        while s in self.slots and self.slots[s] != key:
            assert probes < self.M, "the table is full"
            wrapped |= s == self.M - 1
            s = (s + 1) & (self.M - 1)
            probes += 1
        return s, probes, wrapped

    def _note(self, probes, wrapped):
        self.longest = max(self.longest, probes)
        self.wraps += wrapped
        return probes, wrapped

    def put(self, key):
        """Insert (a stored key is found): (probes, passed slot M-1 to slot 0)."""
        s, probes, wrapped = self._walk(key)
        self.slots[s] = key
        return self._note(probes, wrapped)

    def find(self, key):
        """Look up: (probes until the key or the first empty slot, wrapped, found)."""
        s, probes, wrapped = self._walk(key)
        return self._note(probes, wrapped) + (s in self.slots,)


def chain_of(keys, M):
    """A Chain of M slots with `keys` inserted in order."""
    c = Chain(M)
    for k in keys:
        c.put(k)
    return c


def stage_slots(n):
    """The batch's staging table (lb_device.hip): the power of two >= 4 n, at least 64."""
    s = 64
    while s < 4 * n:
        s *= 2
    return s


# ---- one service, one backend, and the flow search -------------------------------

def one_backend(proto=17, salt=0):
    """One service with one backend: a flow's backward key is a function of its sid alone."""
    return np.array([(0x0a00000a + salt, 0x5000 + salt, proto, 0, 0xc0a80101 + salt, 0x901f + salt,
                      (2, 4, 6, 8, 10, 12), 1, (0, 0))], dtype=lb.BACKEND_DTYPE)


def fwd_key(sid):
    return (sid[0], sid[1], sid[2] | sid[3] << 16, sid[4])


def bwd_sid(bk, sid):
    r = bk[0]
    return (int(r["addr"]), sid[0], int(r["port"]), sid[2], sid[4])


def bwd_key(bk, sid):
    return fwd_key(bwd_sid(bk, sid))


@functools.lru_cache(maxsize=None)
def _draw(seed):
    """DRAWS client (saddr, sport) pairs, in the order they were drawn."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 1 << 32, DRAWS, dtype=np.uint64), rng.integers(1, 1 << 16, DRAWS, dtype=np.uint64)


def _pick(seed, mask, count, skip):
    """The distinct clients `mask` selects, in drawing order: `count` of them after the first `skip`."""
    saddr, sport = _draw(seed)
    idx = np.nonzero(mask)[0]
    _, first = np.unique(saddr[idx] << np.uint64(16) | sport[idx], return_index=True)
    idx = idx[np.sort(first)][skip:skip + count]
    assert idx.size == count, f"the search gives {idx.size} clients where {skip} + {count} were asked for"
    return list(zip(saddr[idx].tolist(), sport[idx].tolist()))


@functools.lru_cache(maxsize=None)
def _hashes(seed, daddr, dport, proto, baddr, bport):
    """acl_hash of the forward key towards (daddr, dport) and of the backward
    key from (baddr, bport), for every drawn client."""
    saddr, sport = _draw(seed)
    hs = acl_hash(saddr, daddr, sport | np.uint64(dport << 16), proto)
    hb = acl_hash(baddr, saddr, np.uint64(bport) | sport << np.uint64(16), proto)
    return hs, hb


def flows(bk, M, w, group, count, skip=0, seed=2026):
    """`count` client sids towards bk's service, after the first `skip`, whose
    "s": forward key homes in the window of w slots across the end of a table of
          M slots and whose backward key does not;
    "b": backward key does and whose forward key does not;
    "both": keys both do (only a small M gives any)."""
    r = bk[0]
    dst = (int(r["vaddr"]), int(r["vport"]), int(r["proto"]))
    hs, hb = _hashes(seed, *dst, int(r["addr"]), int(r["port"]))
    ws, wb = in_window(hs, M, w), in_window(hb, M, w)
    pick = {"s": ws & ~wb, "b": wb & ~ws, "both": ws & wb}[group]
    return [(a, dst[0], p, dst[1], dst[2]) for a, p in _pick(seed, pick, count, skip)]


def sids_towards(daddr, dport, proto, M, w, count, skip=0, seed=2026):
    """`count` sids towards any (daddr, dport) whose own key homes in the window."""
    hs, _ = _hashes(seed, daddr, dport, proto, 0, 0)
    return [(a, daddr, p, dport, proto) for a, p in _pick(seed, in_window(hs, M, w), count, skip)]


def same_home_keys(M, count, seed=2027):
    """(home, `count` keys (a, b, c, p) that all hash to that one slot of a table of M slots)."""
    daddr, dport, proto = 0x0b0b0b0b, 0x3500, 6
    hs, _ = _hashes(seed, daddr, dport, proto, 0, 0)
    home = hs & U32(M - 1)
    best = int(np.bincount(home, minlength=M).argmax())
    return best, [fwd_key((a, daddr, p, dport, proto)) for a, p in _pick(seed, home == best, count, 0)]


# ---- batches of 64-byte frames ---------------------------------------------------

NO_SERVICE = (0x0c0c0c0c, 0x1f90)   # an address and port that no service of these tests has
PASS_IFACE, INGRESS, NIF = 3, 2, 4  # the batches run with ingress 2 of 4 interfaces: PASS is 3 for both NFs


def session_of(bk, sid, direction, mac=(9, 8, 7, 6, 5, 4), ifindex=3):
    """A stored session for key sid: towards bk's backend, or towards a client."""
    r = bk[0]
    if direction == lb.TO_BACKEND:
        return LC.session(*sid, lb.TO_BACKEND, int(r["addr"]), int(r["port"]), r["mac"].tolist(), int(r["ifindex"]))
    return LC.session(*sid, lb.TO_CLIENT, int(r["vaddr"]), int(r["vport"]), list(mac), ifindex)


def sessions(pairs):
    ks, vs = [p[0] for p in pairs], [p[1] for p in pairs]
    return np.array(ks, dtype=lb.KEY_DTYPE), np.array(vs, dtype=lb.VALUE_DTYPE)


class Batch:
    """n 64-byte frames in 64-byte slots, filler (not IPv4: it passes) until a
    frame is put.  what[i] names frame i: ("f", flow) a frame of a client sid
    towards the service, ("b", flow) its backward traffic, ("x", sid) any other
    candidate, None the filler."""

    def __init__(self, n, seed):
        self.rng = np.random.default_rng(seed)
        self.n = n
        self.fr = self.rng.integers(0, 256, (n, 64), dtype=np.uint8)
        self.fr[:, 12] = 0x86
        self.what = [None] * n
        self.mac = [None] * n

    def put(self, i, sid, tag):
        assert self.what[i] is None
        mac = self.rng.integers(0, 256, 6).tolist()
        self.fr[i] = np.frombuffer(LC.frame(self.rng, sid, length=64, smac=mac), dtype=np.uint8)
        self.what[i], self.mac[i] = tag, mac

    def free(self):
        return [i for i, t in enumerate(self.what) if t is None]

    def scatter(self, items):
        """items (sid, tag) onto free indices in a random order."""
        free = self.free()
        assert len(items) <= len(free)
        at = self.rng.permutation(len(free))[:len(items)]
        for (sid, tag), j in zip(items, at.tolist()):
            self.put(free[j], sid, tag)

    def reversed(self):
        other = Batch.__new__(Batch)
        other.rng, other.n = self.rng, self.n
        other.fr, other.what, other.mac = self.fr[::-1].copy(), self.what[::-1], self.mac[::-1]
        return other

    def arrays(self):
        descs = np.zeros(self.n, dtype=frames.DESC_DTYPE)
        descs["addr"] = np.arange(self.n, dtype=np.uint64) * 64
        descs["len"] = 64
        return self.fr.reshape(-1).copy(), descs

    def creators(self):
        """{flow sid: the lowest index of its forward frames}."""
        out = {}
        for i, t in enumerate(self.what):
            if t is not None and t[0] == "f":
                out.setdefault(t[1], i)
        return out

    def staged_keys(self, bk):
        """The distinct keys lb_propose stages, in the loop's order (given that
        no session exists yet for any flow of the batch)."""
        keys = []
        for sid in self.creators():
            keys += [fwd_key(sid), bwd_key(bk, sid)]
        return keys

    def expected_verdicts(self, bk, known=()):
        """{index: verdict} of the flows' frames on a table that holds the keys
        `known` and no other key of the batch: forward frames go to the
        backend's interface, backward frames pass ahead of their flow's creator
        and return through the ingress interface after it."""
        first = self.creators()
        out = {}
        for i, t in enumerate(self.what):
            if t is None or t[0] == "x":
                continue
            if t[0] == "f":
                out[i] = int(bk[0]["ifindex"])
            else:
                out[i] = INGRESS if (t[1] in known or (t[1] in first and first[t[1]] < i)) else PASS_IFACE
        return out


def small_case(variant):
    """3a: eight flows whose 16 keys all home in slots 62, 63, 0, 1 of the
    smallest staging table (64 slots for n <= 16) and of a session table of 64
    slots.  16 frames hold either two frames of every flow ("two_frames") or,
    "backward", two frames of four flows, one of the other four, and four
    backward frames, two ahead of their flow's first frame and two after it."""
    bk = one_backend(17)
    fl = flows(bk, 64, 4, "both", 8)
    b = Batch(16, 301)
    if variant == "two_frames":
        order = b.rng.permutation(16).tolist()
        for j, i in enumerate(order):
            b.put(i, fl[j % 8], ("f", fl[j % 8]))
    else:
        # index:  0   1   2   3   4   5   6   7   8   9   10  11  12  13  14  15
        plan = ["b0", "f1", "f0", "b1", "f2", "b3", "f4", "f0", "f3", "f5", "b2", "f1", "f6", "f2", "f7", "f3"]
        for i, p in enumerate(plan):
            sid = fl[int(p[1])]
            if p[0] == "f":
                b.put(i, sid, ("f", sid))
            else:
                b.put(i, bwd_sid(bk, sid), ("b", sid))
    return bk, b


def grid_case(T, reverse=False):
    """3b: n = 16 T frames, sixteen blocks.  256 flows whose forward key and 256
    whose backward key home in a window of 16 slots across the end of the
    staging table (and so of the session table of 8192 slots); two to three
    frames per flow in different blocks, the lowest of them in block flow % 15;
    for every other flow a backward frame ahead of the creator where an index
    is free and one after it.  reverse: the same frames in the opposite order."""
    bk = one_backend(6)
    n = 16 * T
    M = stage_slots(n)
    fl = flows(bk, M, 16, "s", 256) + flows(bk, M, 16, "b", 256)
    b = Batch(n, 302)
    rng = b.rng
    room = [rng.permutation(T).tolist() for _ in range(16)]
    for j, sid in enumerate(fl):
        first = j % 15
        later = rng.permutation(np.arange(first + 1, 16))[:1 + j % 2].tolist()
        for blk in [first] + later:
            b.put(blk * T + room[blk].pop(), sid, ("f", sid))
    first = b.creators()
    used = np.array([t is not None for t in b.what])
    for j, sid in enumerate(fl):
        if j % 2:
            continue
        c = first[sid]
        for cand in (np.nonzero(~used[:c])[0], c + 1 + np.nonzero(~used[c + 1:])[0]):
            if cand.size:
                i = int(cand[rng.integers(cand.size)])
                b.put(i, bwd_sid(bk, sid), ("b", sid))
                used[i] = True
    return bk, (b.reversed() if reverse else b), fl


def deep_case():
    """3c: a session table of 1024 slots (max_sessions 512) with 300 stored
    sessions, 150 towards the backend and 150 towards clients, homed in a window
    of 16 slots across its end.  A frame for each; 150 near misses of the same
    homes towards no service; 150 frames of 100 new flows towards the service
    (500 sessions afterwards), whose forward keys join the cluster."""
    bk = one_backend(6, salt=1)
    M, w = 1024, 16
    fs, fb = flows(bk, M, w, "s", 250), flows(bk, M, w, "b", 300)
    pre = []
    for i in range(150):
        pre += [session_of(bk, fs[i], lb.TO_BACKEND), session_of(bk, bwd_sid(bk, fb[i]), lb.TO_CLIENT, ifindex=i % NIF)]
    stored = [fs[i] for i in range(150)] + [bwd_sid(bk, fb[i]) for i in range(150)]
    absent = [bwd_sid(bk, s) for s in fb[150:300]]
    new = fs[150:250]
    items = [(s, ("x", s)) for s in stored + absent]
    items += [(s, ("f", s)) for s in new] + [(s, ("f", s)) for s in new[::2]]
    b = Batch(640, 303)
    b.scatter(items)
    return bk, sessions(pre), b, stored, absent, new


def capacity_case():
    """3d: max_sessions 256 in 512 slots.  56 stored sessions and 100 new flows
    of one to four frames, every key of them homed in one window of 16 slots
    across the end of the staging table of n = 512 frames (2048 slots): 56 + 2 *
    100 == 256.  `extra` is the exact-fit batch with one frame of one further
    flow; `gated` the exact-fit batch with 20 further flows of one to three
    frames, which the ACL `rules` holds."""
    bk = one_backend(17, salt=2)
    n = 512
    M, w = stage_slots(n), 16
    fs, fb = flows(bk, M, w, "s", 28 + 50 + 1 + 20), flows(bk, M, w, "b", 28 + 50)
    pre, stored = [], []
    for i in range(28):
        pre += [session_of(bk, fs[i], lb.TO_BACKEND), session_of(bk, bwd_sid(bk, fb[i]), lb.TO_CLIENT, ifindex=i % NIF)]
        stored += [fs[i], bwd_sid(bk, fb[i])]
    new = fs[28:78] + fb[28:78]
    items = [(s, ("x", s)) for s in stored]
    for j, s in enumerate(new):
        items += [(s, ("f", s))] * (1 + j % 4)
        if j % 3 == 0:
            items.append((bwd_sid(bk, s), ("b", s)))
    exact = Batch(n, 304)
    exact.scatter(items)
    extra, gated = Batch(n, 304), Batch(n, 304)
    for other in (extra, gated):
        other.scatter(items)
        assert other.what == exact.what and np.array_equal(other.fr, exact.fr)
    extra.scatter([(fs[78], ("f", fs[78]))])
    held = fs[79:99]
    gitems = []
    for j, s in enumerate(held):
        gitems += [(s, ("f", s))] * (1 + j % 3)
    gated.scatter(gitems)
    rules = FC.rules_from_keys([sid_bytes(s) for s in held], [FC.ACTIONS[j % len(FC.ACTIONS)] for j in range(20)])
    return {"bk": bk, "pre": sessions(pre), "stored": stored, "new": new, "exact": exact, "extra": extra,
            "gated": gated, "gated_frames": len(gitems), "rules": rules, "max_sessions": 256, "slots": 512}


def sid_bytes(sid) -> bytes:
    """The 13 key bytes of sid = (saddr, daddr, sport, dport, proto)."""
    return (sid[0].to_bytes(4, "little") + sid[1].to_bytes(4, "little") + sid[2].to_bytes(2, "little") +
            sid[3].to_bytes(2, "little") + bytes([sid[4]]))


def acl_cluster_case():
    """3e: an ACL of 1024 slots whose 600 rules (300 towards the service, 300
    towards an address without one; every action of firewall_cases.ACTIONS, 0
    among them) home in a window of 16 slots across its end.  A frame for every
    rule; near misses of the same homes that the ACL does not hold: 60 with a
    stored session, 120 new flows towards the service (180 frames), 100 towards
    no service."""
    bk = one_backend(6, salt=3)
    r = bk[0]
    M, w = 1024, 16
    to_svc = sids_towards(int(r["vaddr"]), int(r["vport"]), 6, M, w, 300 + 30 + 120)
    to_none = sids_towards(*NO_SERVICE, 6, M, w, 300 + 30 + 100)
    ruled = [s for pair in zip(to_svc[:300], to_none[:300]) for s in pair]
    rules = FC.rules_from_keys([sid_bytes(s) for s in ruled], [FC.ACTIONS[j % len(FC.ACTIONS)] for j in range(600)])
    stored = to_svc[300:330] + to_none[300:330]
    pre = [session_of(bk, s, lb.TO_BACKEND if j < 30 else lb.TO_CLIENT) for j, s in enumerate(stored)]
    new, nowhere = to_svc[330:450], to_none[330:430]
    items = [(s, ("x", s)) for s in ruled + stored + nowhere]
    items += [(s, ("f", s)) for s in new] + [(s, ("f", s)) for s in new[::2]]
    b = Batch(1024, 305)
    b.scatter(items)
    return bk, rules, ruled, sessions(pre), b, new
