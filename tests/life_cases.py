"""Scripts and the combined model for the long-run tests (tests/test_life.py,
tests/test_gpu_life.py): about 200 operations on ONE LoadBalancer and ONE Acl
object -- batches of the load balancer, of lbfw with and without the gate and of
the firewall, ACL updates, session removals, drains, clears and puts -- over a
small fixed universe of keys, so that the same keys are stored, removed and
created again many times on tables that carry tombstones.

The model is composed from the other *_cases modules and restates none of their
rules: tests/lb_remove_cases.Model holds the sessions, the removals and the
session table's tombstone count, tests/lbfw_cases.Model.batch is lbfw's loop,
the ACL is a dict kept by tests/acl_update_cases.apply, the firewall's verdicts
are tests/firewall_cases.model's.  Two things no earlier model needed are stated
here, from include/xsknf_gpu.h and the comment at the head of kernel_lb.h:
  - where an ACL update's keys come to lie (AclSlots: the first tombstone of the
    probe sequence; the rebuild in ascending slot order), which is what
    info["tombstones"] and the size of an update's records depend on;
  - when a device batch stands down to its ordered path (stand_down), which the
    batch reports in its ordered_batches word and the host forms never do.
It shares no code with xsknf_amd/csrc.  A script is generated together with the
model's run over it: every op carries what the model expects after it (`want`),
and coverage() counts, from the model alone, what the script exercises.
"""
import collections
import functools
import types

import numpy as np

from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lb_remove_cases as RC
from tests import lbfw_cases as WC
from xsknf_amd import firewall, frames, lb

ORDERED = WC.ORDERED
CREATED, FAILED = lb.LB_STATS.index("sessions_created"), lb.LB_STATS.index("inserts_failed")
BATCHES = ("lb_batch", "lbfw_batch")
REMOVALS = ("sessions_remove", "drain_backend")

Shape = collections.namedtuple("Shape", "name seed n_ops slots max_sessions acl_slots clients strangers acl_keys "
                                        "acl_initial max_frames max_flows max_remove max_update puts clear weights")
# the weights: lb_batch, lbfw_batch behind the ACL, lbfw_batch without, firewall_batch, acl_update,
# sessions_remove, drain_backend
SHAPES = {
    # chains wrap, both tombstone bounds are reached, the session table is full again and again
    "small": Shape("small", 9101, 200, 256, 128, 64, 200, 24, 44, 20, 300, 18, 64, 40, (66, 133), (100,),
                   (22, 18, 7, 6, 14, 24, 9)),
    # key lists and update records on both sides of a stage's first 4096 bytes
    "wide": Shape("wide", 9202, 200, 4096, 2048, 1024, 700, 40, 640, 300, 300, 90, 600, 400, (66, 133), (100,),
                  (24, 16, 6, 5, 14, 27, 8)),
}
KINDS = ("lb_batch", "lbfw_batch", "lbfw_batch_open", "firewall_batch", "acl_update", "sessions_remove",
         "drain_backend")


def stage_first_bytes(name):
    """The capacity of the first stage a removal (lb_remove_device.hip) or an
    update (acl_update_device.hip) makes."""
    return LC.code_constant(r"size_t cap = (\d+);   // powers of two", name)


@functools.lru_cache(maxsize=None)
def session_tombstone_share():
    """A removal that leaves more than slots / this many tombstones rebuilds (lb_table.h)."""
    return LC.code_constant(r"constexpr uint32_t kTombstoneShare = (\d+);", "lb_table.h")


def update_record_bytes():
    return FC.code_constant(r"sizeof\(AclUpdateRec\) == (\d+)", "acl_table.h")


# ---- the model -----------------------------------------------------------------------

class Sessions(RC.Model):
    """The session table: RC.Model (LC.Model.batch is the load balancer's loop)
    with lbfw's loop beside it, on the same dict."""
    lbfw_batch = WC.Model.batch


class AclSlots:
    """Where the ACL's keys lie (include/xsknf_gpu.h, xsknf_gpu_acl_update's
    "How"): what the tombstone count, the rebuilds and the number of changed
    slots follow from.  The rules themselves are the dict's (UC.apply)."""
    TOMB = "tombstone"

    def __init__(self, slots, rules):
        self.n, self.slot, self.at, self.tombstones = slots, [None] * slots, {}, 0
        for r in rules:
            k = FC.rule_key(r)
            if k[12] in (6, 17) and k not in self.at:
                self._store(k, self._empty_from(k))

    def _store(self, k, s):
        self.slot[s], self.at[k] = k, s

    def _empty_from(self, k):
        s = UC.home(k, self.n)
        while self.slot[s] is not None:
            s = (s + 1) & (self.n - 1)
        return s

    def _place(self, k):
        """The first tombstone on the way to the empty slot that ends k's probe, or that slot."""
        s, tomb = UC.home(k, self.n), None
        while self.slot[s] is not None:
            if self.slot[s] is self.TOMB and tomb is None:
                tomb = s
            s = (s + 1) & (self.n - 1)
        return s if tomb is None else tomb

    def update(self, ops):
        """(rebuilt, changed slots) of one accepted call: the last op of a key
        stands for it, the deletes go first, the puts follow in op order."""
        last = {}
        for i, o in enumerate(ops):
            k = FC.rule_key(o["rule"])
            if k[12] in (6, 17):
                last[k] = (i, int(o["op"]))
        dels = [k for k, (_, op) in last.items() if op == UC.DELETE and k in self.at]
        puts = [k for _, k in sorted((i, k) for k, (i, op) in last.items() if op == UC.PUT)]
        after = len(self.at) - len(dels) + sum(1 for k in puts if k not in self.at)
        assert after < self.n, "the generator made an update that must be refused"
        if not dels and not puts:
            return False, 0
        tombs = self.tombstones + len(dels)
        rebuilt = tombs > self.n // UC.tombstone_share() or after + tombs > self.n - 1
        dirty = set()
        for k in dels:
            s = self.at.pop(k)
            self.slot[s] = self.TOMB
            dirty.add(s)
        self.tombstones = tombs
        if rebuilt:
            live = [e for e in self.slot if e is not None and e is not self.TOMB]
            self.slot, self.at, self.tombstones = [None] * self.n, {}, 0
            for k in live:
                self._store(k, self._empty_from(k))
        for k in puts:
            if k not in self.at:
                s = self._place(k)
                self.tombstones -= self.slot[s] is self.TOMB
                self._store(k, s)
            dirty.add(self.at[k])
        return rebuilt, len(dirty)


def stand_down(M, umem, descs, acl):
    """Why a device batch leaves its parallel path, on the tables as they stand
    before it (kernel_lb.h): "capacity" -- the sessions plus the distinct keys
    the batch proposes pass max_sessions; "flag" -- a proposed backward key is a
    stored session already, or one key is proposed by two flows or as both a
    forward and a backward key; "both"; or None.  A frame proposes where it is
    a candidate the gate lets through whose key is no session and whose
    destination is a service."""
    size, buf = int(umem.size), umem.tobytes()
    proposed, flag = {}, False
    for addr, ln in zip(descs["addr"].tolist(), descs["len"].tolist()):
        off = (addr & ((1 << 48) - 1)) + (addr >> 48)
        if not (off <= size and ln <= size - off):
            continue
        key = FC.frame_key(buf[off:off + ln])[1]
        if key is None or (acl is not None and key in acl) or key in M.sessions:
            continue
        backs = M.services.get(key[4:8] + key[10:12] + key[12:13])
        if backs is None:
            continue
        baddr, bport = backs[LC.jhash(key) % len(backs)][:2]
        bkey = baddr.to_bytes(4, "little") + key[0:4] + bport.to_bytes(2, "little") + key[8:10] + key[12:13]
        flag |= bkey in M.sessions
        proposed.setdefault(key, set()).add((key, 0))
        proposed.setdefault(bkey, set()).add((key, 1))
    flag |= any(len(who) > 1 for who in proposed.values())
    capacity = len(M.sessions) + len(proposed) > M.max_sessions
    return "both" if flag and capacity else "flag" if flag else "capacity" if capacity else None


class World:
    """Everything the script's objects hold, and apply(op): the model's run of one op."""

    def __init__(self, shape, backends, rules, sessions=Sessions):
        self.shape = shape
        self.M = sessions(backends, shape.max_sessions, shape.slots)
        self.acl = FC.acl_dict(rules)
        self.slots = AclSlots(shape.acl_slots, rules)
        self._dump = self.M.dump()
        self._rules = UC.sorted_rules(self.acl)

    def apply(self, op):
        M = self.M
        before = dict(M.sessions)
        w = types.SimpleNamespace(tomb_before=M.tombstones, acl_tomb_before=self.slots.tombstones)
        if op.kind in BATCHES:
            acl = self.acl if op.kind == "lbfw_batch" and op.gate else None
            w.cause = stand_down(M, op.umem, op.descs, acl)
            w.umem = op.umem.copy()
            if op.kind == "lb_batch":
                w.verdicts, w.stats = M.batch(w.umem, op.descs, op.ingress, op.nif)
            else:
                w.verdicts, w.stats = M.lbfw_batch(w.umem, op.descs, op.ingress, op.nif, acl)
            w.host_stats = w.stats.copy()          # the host forms never stand down
            w.stats[ORDERED] = int(w.cause is not None)
            w.created = set(M.sessions) - set(before)
        elif op.kind == "firewall_batch":
            w.verdicts = FC.model(op.umem, op.descs, self.acl)
        elif op.kind == "acl_update":
            self.acl = UC.apply(self.acl, op.ops)
            w.rebuilt, w.records = self.slots.update(op.ops)
            assert set(self.slots.at) == set(self.acl)
            w.stage_bytes = 20 * self.shape.acl_slots if w.rebuilt else update_record_bytes() * w.records
            self._rules = UC.sorted_rules(self.acl)
        elif op.kind == "sessions_remove":
            w.result = M.remove(op.keys, op.pair)
        elif op.kind == "drain_backend":
            w.result = M.drain(op.addr, op.port, op.proto)
        elif op.kind == "sessions_clear":
            M.clear()
        elif op.kind == "sessions_put":
            M.sessions_put(op.keys, op.values)
        else:
            self.other(op, w)
        if op.kind in REMOVALS:
            w.removed = set(before) - set(M.sessions)
        if M.sessions != before:
            self._dump = M.dump()
        w.sessions = tuple(a.tobytes() for a in self._dump)
        w.n_sessions, w.tombstones = len(M.sessions), M.tombstones
        w.acl_rules, w.acl_tombstones = self._rules, self.slots.tombstones
        op.want = w
        return w

    def other(self, op, w):
        """The op kinds of a later generation of scripts (tests/churn_cases.py)."""
        raise ValueError(op.kind)


# ---- the universe and the generator --------------------------------------------------

def sid_of_key(k: bytes):
    return (LC._u32(k, 0), LC._u32(k, 4), LC._u16(k, 8), LC._u16(k, 10), k[12])


def key_records(keys) -> np.ndarray:
    """KEY_DTYPE records of 13-byte keys."""
    k = np.zeros(len(keys), dtype=lb.KEY_DTYPE)
    if len(keys):
        k.view(np.uint8).reshape(-1, 16)[:, :13] = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 13)
    return k


def _universe(shape, rng):
    """2 UDP services and a TCP one with 1, 2 and 3 backends (their records
    interleaved), the clients, their backward sids, strangers towards no
    service, and the keys the ACL's updates draw from: client, backward and
    stranger keys and keys that no frame of a flow carries."""
    svcs = [(0x0a00000a, 0x5000, 17, 1), (0x0b00000b, 0x5100, 6, 2), (0x0c00000c, 0x5200, 17, 3)]
    recs = []
    for vaddr, vport, proto, count in svcs:
        for j in range(count):
            recs.append((vaddr, vport, proto, 0, 0xc0a80100 + (vaddr & 0xff) * 16 + j, 0x901f + j,
                         tuple(rng.integers(0, 256, 6).tolist()), 1 + (len(recs) % 3), (0, 0)))
    backends = np.array([recs[i] for i in (0, 3, 1, 4, 2, 5)], dtype=lb.BACKEND_DTYPE)
    clients = {}
    while len(clients) < shape.clients:
        s = LC.service_sid(rng, backends)
        clients[s] = None
    clients = list(clients)
    backs = [LC.backward_sid(backends, s) for s in clients]
    strangers = [(int(rng.integers(1, 1 << 32)), 0x0d0d0d0d, int(rng.integers(1, 1 << 16)), 0x5300, 6 + 11 * (i & 1))
                 for i in range(shape.strangers)]
    a = shape.acl_keys // 3
    acl_keys = ([WC.sid_key(s) for s in clients[:a]] + [WC.sid_key(s) for s in backs[a:a + a // 3]] +
                [WC.sid_key(s) for s in strangers[:shape.strangers // 2]])
    while len(acl_keys) < shape.acl_keys:
        acl_keys.append(UC.random_key(rng))
    assert len(set(acl_keys)) == shape.acl_keys
    return types.SimpleNamespace(backends=backends, clients=clients, backs=backs, strangers=strangers, acl_keys=acl_keys)


def _outside(descs, umem, rng):
    """A few descriptors outside the UMEM (FC.with_outside's kinds) among the others."""
    size = int(umem.size)
    bad = [(size - 10, 11), (size, 1), (1 << 47, 64), (size - 1, 0xffffffff), (((1 << 48) - 1) | (0xffff << 48), 64),
           (0, size + 1)]
    out = [tuple(d) for d in descs]
    for _ in range(int(rng.integers(0, 4))):
        b = bad[int(rng.integers(len(bad)))]
        out.insert(int(rng.integers(len(out) + 1)), (b[0], b[1], 7))
    return np.array(out, dtype=frames.DESC_DTYPE)


def _batch(shape, U, world, rng, lookups_only=False):
    """30 .. max_frames frames (across the 256-lane tile): frames of a handful
    of flows, forward and backward in one batch, mixed ihl (0 and 3: the key is
    what then lies where the parse reads it), TCP and UDP; frames whose keys the
    ACL may hold; strangers; frames the parse decides.  Packed with no gap, or
    with small ones."""
    n = int(rng.integers(30, shape.max_frames + 1))
    items = []
    flows = int(rng.integers(2, shape.max_flows + 1))
    # half of the batches stay inside a window of the clients, so that flows return as hits
    span = len(U.clients) if rng.integers(2) else min(len(U.clients), 3 * flows)
    lo = int(rng.integers(0, len(U.clients) - span + 1))
    for c in (lo + rng.permutation(span)[:flows]).tolist():
        if lookups_only and rng.integers(2):
            continue
        for _ in range(int(rng.integers(1, 4))):
            items.append(LC.frame(rng, U.clients[c], ihl=int(rng.choice([5, 5, 5, 6, 15, 0, 3])),
                                  zero_check=bool(rng.integers(4) == 0)))
        for _ in range(int(rng.integers(0, 3))):
            items.append(LC.frame(rng, U.backs[c], ihl=int(rng.choice([5, 7]))))
    for k in rng.permutation(len(U.acl_keys))[:int(rng.integers(2, 12))].tolist():
        items.append(LC.frame(rng, sid_of_key(U.acl_keys[k]), ihl=5))
    for s in rng.permutation(len(U.strangers))[:int(rng.integers(0, 5))].tolist():
        items.append(LC.frame(rng, U.strangers[s], ihl=int(rng.choice([5, 6]))))
    items = [items[i] for i in rng.permutation(len(items))][:n - 4]
    while len(items) < n:
        items.append(FC.make_frame(rng, int(rng.integers(0, 120)), 5, int(rng.choice([6, 17, 1])), bool(rng.integers(4))))
    items = [items[i] for i in rng.permutation(len(items))]
    umem, descs = FC.pack_unaligned(items, rng, max_gap=12) if rng.integers(4) == 0 else LC.pack_packed(items, rng)
    return umem, _outside(descs, umem, rng)


def _removal(shape, U, world, rng):
    """A key list of 1 .. max_remove records: stored keys, some beside their
    partners, duplicates, keys the table does not hold, records with a bad
    proto, pad bytes that must be ignored."""
    n = int(rng.integers(1, shape.max_remove + 1))
    if rng.integers(5) == 0:
        n = min(n, 4)
    live = list(world.M.sessions)
    # every other list, where the table allows it, stops exactly AT the bound:
    # slots / 4 tombstones stay and nothing is rebuilt; the next removal passes it
    short = shape.slots // session_tombstone_share() - world.M.tombstones
    if rng.integers(2) == 0 and 1 <= short <= min(len(live), shape.max_remove - 2):
        keys = [live[i] for i in rng.permutation(len(live))[:short].tolist()]
        keys += [keys[0], WC.sid_key(U.strangers[0])[:12] + bytes([1])]      # a duplicate, a bad proto
        return key_records([keys[i] for i in rng.permutation(len(keys))]), False
    keys = []
    if live:
        for i in rng.permutation(len(live))[:int(rng.integers(n // 3, n + 1))].tolist():
            keys.append(live[i])
            if rng.integers(4) == 0:
                keys.append(RC.partner(live[i], world.M.sessions[live[i]]))   # both halves of one flow
            if rng.integers(8) == 0:
                keys.append(live[i])                                           # a duplicate
    while len(keys) < n:
        pool = U.clients if rng.integers(2) else U.strangers
        keys.append(WC.sid_key(pool[int(rng.integers(len(pool)))]))           # mostly absent
    keys = [keys[i] for i in rng.permutation(len(keys))][:n]
    rec = key_records(keys)
    odd = rng.integers(0, 12, n) == 0
    rec["proto"][odd] = 1
    rec["pad"][rng.integers(0, 6, n) == 0] = (0xa5, 0x5a, 0xff)
    return rec, bool(rng.integers(2))


def _update(shape, U, world, rng):
    """1 .. max_update ops on the ACL universe: puts of new keys, replaces,
    deletes of stored and of absent keys, a key named twice, a bad proto."""
    n = int(rng.integers(1, shape.max_update + 1))
    share = (0.65, 0.25, 0.9)[int(rng.integers(3))]      # mixed, delete-heavy, put-heavy
    items = []
    for k in rng.integers(0, len(U.acl_keys), n).tolist():
        key = U.acl_keys[k]
        if rng.integers(40) == 0:
            key = key[:12] + bytes([1])
        items.append((UC.PUT if rng.random() < share else UC.DELETE, key, FC.ACTIONS[int(rng.integers(len(FC.ACTIONS)))]))
    return UC.ops_of(items)


def _put(shape, U, world, rng):
    """A few stranger sessions (towards no service, no partner) where there is
    room, and new values for stored ones."""
    room = shape.max_sessions - len(world.M.sessions)
    new = [s for s in U.strangers if WC.sid_key(s) not in world.M.sessions][:min(room, 6)]
    old = [sid_of_key(k) for k in list(world.M.sessions)[:3]]
    ks, vs = RC.stored(new + old, direction=int(rng.integers(2)))
    vs["port"] += int(rng.integers(1, 100))
    return ks, vs


def _generate(shape):
    rng = np.random.default_rng(shape.seed)
    U = _universe(shape, rng)
    rules = FC.rules_from_keys(U.acl_keys[:shape.acl_initial], [FC.ACTIONS[i % len(FC.ACTIONS)]
                                                                 for i in range(shape.acl_initial)])
    world = World(shape, U.backends, rules)
    weights = np.array(shape.weights, dtype=float)
    ops = []
    for i in range(shape.n_ops):
        kind = "sessions_put" if i in shape.puts else "sessions_clear" if i in shape.clear else \
            KINDS[int(rng.choice(len(KINDS), p=weights / weights.sum()))]
        op = types.SimpleNamespace(kind=kind, index=i)
        if kind in ("lb_batch", "lbfw_batch", "lbfw_batch_open"):
            op.kind, op.gate = ("lb_batch", False) if kind == "lb_batch" else ("lbfw_batch", kind == "lbfw_batch")
            op.umem, op.descs = _batch(shape, U, world, rng)
            op.nif = int(rng.choice([4, 4, 4, 2, 1]))
            op.ingress = int(rng.integers(op.nif))
        elif kind == "firewall_batch":
            op.umem, op.descs = _batch(shape, U, world, rng, lookups_only=True)
        elif kind == "acl_update":
            op.ops = _update(shape, U, world, rng)
        elif kind == "sessions_remove":
            op.keys, op.pair = _removal(shape, U, world, rng)
        elif kind == "drain_backend":
            r = U.backends[int(rng.integers(U.backends.shape[0]))]
            op.addr, op.port = int(r["addr"]), int(r["port"])
            op.proto = int(r["proto"]) if rng.integers(6) else 23 - int(r["proto"])
        elif kind == "sessions_put":
            op.keys, op.values = _put(shape, U, world, rng)
        world.apply(op)
        ops.append(op)
    return types.SimpleNamespace(shape=shape, name=shape.name, backends=U.backends, rules=rules, ops=ops)


@functools.lru_cache(maxsize=None)
def script(name):
    """The script of SHAPES[name] with the model's expectations: computed once
    per process and shared; the tests leave it unchanged."""
    return _generate(SHAPES[name])


def describe(op) -> str:
    what = {"lb_batch": lambda: f"{op.descs.shape[0]} frames, ingress {op.ingress} of {op.nif}",
            "lbfw_batch": lambda: f"{op.descs.shape[0]} frames, ingress {op.ingress} of {op.nif}, "
                                  f"{'behind the ACL' if op.gate else 'acl=None'}",
            "firewall_batch": lambda: f"{op.descs.shape[0]} frames",
            "acl_update": lambda: f"{op.ops.shape[0]} ops",
            "sessions_remove": lambda: f"{op.keys.shape[0]} keys, pair={op.pair}",
            "drain_backend": lambda: f"{op.addr:#x}:{op.port:#x} proto {op.proto}",
            "sessions_clear": lambda: "", "sessions_put": lambda: f"{op.keys.shape[0]} sessions"}[op.kind]()
    return f"op {op.index} {op.kind} ({what})"


# ---- what a script exercises, from the model alone --------------------------------------

def coverage(S) -> dict:
    c = collections.Counter()
    state = {}                      # key -> 1 created by a batch, 2 then removed, 3 then created again
    prev, cleared = None, False
    key_bytes = stage_first_bytes("lb_remove_device.hip")
    rec_bytes = stage_first_bytes("acl_update_device.hip")
    for op in S.ops:
        w = op.want
        if op.kind in REMOVALS:
            c["compactions"] += int(w.result[RC.COMPACTED])
            c["removals_that_stop_at_the_tombstone_bound"] += bool(
                int(w.result[RC.REMOVED]) and w.tombstones == S.shape.slots // session_tombstone_share())
            c["removals_after_the_clear"] += cleared
            for k in w.removed:
                if state.get(k) == 1:
                    state[k] = 2
            if op.kind == "sessions_remove":
                c["key_lists_within_the_first_stage" if 16 * op.keys.shape[0] <= key_bytes
                  else "key_lists_past_the_first_stage"] += 1
        elif op.kind in BATCHES:
            c["batches_after_the_clear"] += cleared
            if (w.created and prev is not None and prev.kind in REMOVALS and int(prev.want.result[RC.REMOVED])
                    and not int(prev.want.result[RC.COMPACTED]) and prev.want.tombstones):
                c["creating_batches_right_after_an_uncompacted_removal"] += 1
            if w.cause and w.tomb_before:
                c["capacity_stand_downs_over_tombstones"] += w.cause in ("capacity", "both")
                c["flag_stand_downs_over_tombstones"] += w.cause in ("flag", "both")
            c["stand_downs"] += w.cause is not None
            c["parallel_batches_that_create_over_tombstones"] += bool(not w.cause and w.created and w.tomb_before)
            c["inserts_failed"] += int(w.stats[FAILED])
            c["lbfw_batches_over_acl_tombstones"] += bool(op.kind == "lbfw_batch" and op.gate and w.acl_tomb_before)
            for k in w.created:
                state[k] = {None: 1, 1: 1, 2: 3, 3: 3}[state.get(k)]
        elif op.kind == "acl_update":
            c["acl_rebuilds"] += w.rebuilt
            if not w.rebuilt and w.records:
                c["record_updates_within_the_first_stage" if w.stage_bytes <= rec_bytes
                  else "record_updates_past_the_first_stage"] += 1
        elif op.kind == "sessions_clear":
            c["clears"] += 1
            cleared = True
        c["max_live_plus_tombstones"] = max(c["max_live_plus_tombstones"], w.n_sessions + w.tombstones)
        prev = op
    c["keys_created_again"] = sum(1 for v in state.values() if v == 3)
    return dict(c)


def coverage_gaps(S, cov) -> list:
    """The conditions a script must meet that `cov` does not."""
    need = {"compactions": 3, "creating_batches_right_after_an_uncompacted_removal": 1, "acl_rebuilds": 1,
            "lbfw_batches_over_acl_tombstones": 1, "flag_stand_downs_over_tombstones": 2, "keys_created_again": 20,
            "clears": 1, "batches_after_the_clear": 1, "removals_after_the_clear": 1}
    if S.name == "small":    # the wide table (2048 sessions, 1400 flow keys) never fills, and a list of 600
        need["capacity_stand_downs_over_tombstones"] = 2      # keys seldom ends on its 1024th tombstone
        need["removals_that_stop_at_the_tombstone_bound"] = 1
    if S.name == "wide":
        need.update({k: 1 for k in ("key_lists_within_the_first_stage", "key_lists_past_the_first_stage",
                                    "record_updates_within_the_first_stage", "record_updates_past_the_first_stage")})
    return [f"{k}: {cov.get(k, 0)} < {v}" for k, v in need.items() if cov.get(k, 0) < v]


# ---- one op through the host forms -------------------------------------------------------

def run_host(op, L, A):
    """The op on the host tables of L and A.  Returns what it gave: (verdicts,
    UMEM after, stats) of a batch, the verdicts of a firewall batch, the result
    words of a removal."""
    from xsknf_amd import lbfw

    H = lb.HOST_TABLE
    if op.kind == "lb_batch":
        u = op.umem.copy()
        v, st = lb.lb_host(u, op.descs, L, op.ingress, op.nif)
        return v, u, st
    if op.kind == "lbfw_batch":
        u = op.umem.copy()
        v, st = lbfw.lbfw_host(u, op.descs, A if op.gate else None, L, op.ingress, op.nif)
        return v, u, st
    if op.kind == "firewall_batch":
        return firewall.firewall_host(op.umem, op.descs, A)
    if op.kind == "acl_update":
        return A.update(ops=op.ops)
    if op.kind == "sessions_remove":
        return L.sessions_remove(op.keys, pair=op.pair, which=H)
    if op.kind == "drain_backend":
        return L.drain_backend(op.addr, op.port, op.proto, which=H)
    if op.kind == "sessions_clear":
        return L.sessions_clear(H)
    return L.sessions_put(op.keys, op.values)


def same_batch(op, verdicts, umem, stats, want_stats) -> str:
    """"" or what differs between a batch's outputs and the model's."""
    w = op.want
    bad = np.nonzero(verdicts != w.verdicts)[0]
    if bad.size:
        return f"{bad.size} verdicts differ, first at {bad[:8]}: {verdicts[bad[:8]]} != {w.verdicts[bad[:8]]}"
    bad = np.nonzero(umem != w.umem)[0]
    if bad.size:
        return f"{bad.size} UMEM bytes differ, first at {bad[:8]}"
    if [int(x) for x in stats] != [int(x) for x in want_stats]:
        return f"stats {[int(x) for x in stats]} != {[int(x) for x in want_stats]}"
    return ""


def same_tables(op, sessions, rules) -> str:
    """"" or what differs between the dumps (sessions: (keys, values)) and the model's."""
    w = op.want
    if (sessions[0].tobytes(), sessions[1].tobytes()) != w.sessions:
        return f"the session table is not the model's ({sessions[0].shape[0]} sessions, the model {w.n_sessions})"
    if rules.tobytes() != w.acl_rules.tobytes():
        return f"the ACL is not the model's ({rules.shape[0]} rules, the model {w.acl_rules.shape[0]})"
    return ""
