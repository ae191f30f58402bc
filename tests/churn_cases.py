"""The second generation of the long-run scripts (tests/test_churn.py,
tests/test_gpu_churn.py): about 240 operations on ONE LoadBalancer and ONE Acl,
the op kinds of tests/life_cases.py plus the three features that came after it --
the live backends (backends_update, drain_backends), and ageing (aging_enable,
clock, expire; sessions_ages is held to the model after every op).

Nothing is restated.  The session model is the ageing model and the live
services' model on one dict (tests/lb_age_cases.Model: the per-frame stamping
batch, expire, the stamps dropped by _settle; tests/lb_backends_cases.Model:
update, drain_list, backends_dump), the world around it is life_cases.World --
the ACL, its slots, the stand-down decision, which reads the services as they
stand -- and the generator reuses life_cases' _batch, _removal, _update and _put.
Before aging_enable the model's clock is 0 and so is every stamp, which is what
the header says an enable makes of the stored sessions.  It shares no code with
xsknf_amd/csrc.  Every op carries what the model expects after it (`want`), and
coverage() counts, from the model alone, what a script exercises.
"""
import collections
import copy
import functools
import types

import numpy as np

from tests import firewall_cases as FC
from tests import lb_age_cases as AC
from tests import lb_backends_cases as BC
from tests import lb_cases as LC
from tests import lb_remove_cases as RC
from tests import lbfw_cases as WC
from tests import life_cases as LF
from xsknf_amd import lb

M32 = AC.M32
BATCHES = LF.BATCHES
REMOVALS = LF.REMOVALS + ("expire", "drain_backends")       # every op that returns the two result words
SEGMENT_ENDS = ("sessions_put", "aging_enable")            # no stream argument: they wait for the device
MAX_PER_SERVICE = 12

Shape = collections.namedtuple("Shape", "name seed n_ops slots max_sessions acl_slots clients strangers acl_keys "
                                        "acl_initial max_frames max_flows max_remove max_update puts clear weights "
                                        "clock0 enable_from")
# the weights: lb_batch, lbfw_batch behind the ACL, lbfw_batch without, firewall_batch, acl_update,
# sessions_remove, drain_backend, clock, expire, backends_update, drain_backends
KINDS = LF.KINDS + ("clock", "expire", "backends_update", "drain_backends")
SHAPES = {
    # ageing from the start (enable_from None), a clock that wraps, a table that fills again and again
    "aged": Shape("aged", 9303, 240, 256, 128, 64, 200, 24, 44, 20, 300, 18, 64, 40, (84, 165), (124,),
                  (24, 20, 7, 4, 10, 9, 3, 14, 12, 10, 7), 0xffffff00, None),
    # ageing enabled in mid-script; key lists, update records and id lists on both sides of a stage's first 4096 bytes
    "churn": Shape("churn", 9409, 240, 4096, 2048, 1024, 700, 40, 640, 300, 300, 90, 600, 400, (130, 186), (150,),
                   (22, 18, 6, 4, 9, 9, 3, 14, 16, 10, 10), 1000, 64),
}


@functools.lru_cache(maxsize=None)
def lds_set_slots():
    """The largest id set lb_drain_list keeps in LDS: a list of half as many entries."""
    return LC.code_constant(r"constexpr uint32_t kLdsSetSlots = (\d+);", "kernel_lb_drain_list.h")


# ---- the model -----------------------------------------------------------------------

class Sessions(AC.Model, BC.Model):
    """One dict under both models: AC.Model's batch (the load balancer's loop,
    or with gate=True lbfw's, one frame at a time with the stamps), put, expire,
    _settle and clear; BC.Model's update, drain_list and backends_dump;
    RC.Model's remove and drain below them."""

    def lbfw_batch(self, umem, descs, ingress, nif, acl):
        return self.batch(umem, descs, ingress, nif, acl, gate=True)


def service_of(key: bytes) -> bytes:
    """The service key a frame with session key `key` addresses."""
    return key[4:8] + key[10:12] + key[12:13]


def frame_keys(op):
    """The session key of every frame of a batch the parse does not decide, in order."""
    size, buf, out = int(op.umem.size), op.umem.tobytes(), []
    for addr, ln in zip(op.descs["addr"].tolist(), op.descs["len"].tolist()):
        off = (addr & ((1 << 48) - 1)) + (addr >> 48)
        if off <= size and ln <= size - off:
            key = FC.frame_key(buf[off:off + ln])[1]
            if key is not None:
                out.append(key)
    return out


class World(LF.World):
    """life_cases.World over Sessions, with the new op kinds and, per op, what
    coverage() needs from the model as it stood around the op."""

    def __init__(self, shape, backends, rules):
        super().__init__(shape, backends, rules, sessions=Sessions)
        self.aging = False
        self.added, self.taken = set(), set()   # (service, addr, port) an update has added / taken away, ever
        self.chosen = {}                        # forward key -> ((addr, port), backends of its service) at its creation
        self._backends = self.M.backends_dump()
        self._order, self._order_of = [], None  # the stored keys in the dump's order, and the dump they were cut from

    def live(self):
        return {(s, b[0], b[1]) for s, backs in self.M.services.items() for b in backs}

    def apply(self, op):
        M = self.M
        before = dict(M.sessions)
        facts = types.SimpleNamespace()
        if op.kind in BATCHES:
            acl = self.acl if op.kind == "lbfw_batch" and op.gate else None
            keys = frame_keys(op)
            through = [k for k in keys if not (acl is not None and k in acl)]
            facts.hits = sum(1 for k in through if k in before)
            live = self.live()
            facts.orphan_hits = sum(1 for k in through if k in before and before[k][0] == lb.TO_BACKEND
                                    and (service_of(k), before[k][1], before[k][2]) in self.taken - live)
            gated_stored = {k for k in keys if acl is not None and k in acl and k in before}
            facts.services = {service_of(k) for k in keys}
        w = super().apply(op)
        w.aging = self.aging
        if op.kind in BATCHES:
            w.hits, w.orphan_hits, w.services = facts.hits, facts.orphan_hits, facts.services
            # a stored session whose frame the ACL decided: visible where the clock has left its stamp behind
            w.gated_stored = sum(1 for k in gated_stored if M.age(k) != 0) if self.aging else 0
            w.to_added = w.moved = 0
            for k in w.created:
                rep = M.sessions[k]
                if rep[0] != lb.TO_BACKEND:
                    continue
                s = service_of(k)
                w.to_added += (s, rep[1], rep[2]) in self.added
                was, now = self.chosen.get(k), ((rep[1], rep[2]), len(M.services[s]))
                w.moved += bool(was and was[0] != now[0] and now[1] < was[1])
                self.chosen[k] = now
        w.clock = M.clock
        if self._order_of is not self._dump:
            raw = self._dump[0].view(np.uint8).reshape(-1, 16)[:, :13].tobytes()
            self._order, self._order_of = [raw[i:i + 13] for i in range(0, len(raw), 13)], self._dump
        w.ages = np.array([M.age(k) for k in self._order], dtype=np.uint32).tobytes() if self.aging else None
        w.backends = self._backends.tobytes()
        w.n_services, w.n_backends = len(M.services), self._backends.shape[0]
        return w

    def other(self, op, w):
        M = self.M
        before = dict(M.sessions)
        if op.kind == "clock":
            w.wrapped = op.now < M.clock
            M.clock = op.now
        elif op.kind == "expire":
            w.idle = sum(1 for k in before if M.age(k) > op.max_idle)
            w.result = M.expire(op.max_idle)
            w.idle_kept = w.idle - int(w.result[RC.REMOVED])
        elif op.kind == "backends_update":
            was = self.live()
            M.update(op.ops)
            now = self.live()
            self.added |= now - was
            self.taken |= was - now
            w.services = {BC.svc_key(o["backend"]) for o in op.ops}
            self._backends = M.backends_dump()
        elif op.kind == "drain_backends":
            gone_backends = {(a, p, s[6]) for s, a, p in self.taken - self.live()}
            named = {(int(t["addr"]), int(t["port"]), int(t["proto"])) for t in op.ids} & gone_backends
            w.result = M.drain_list(op.ids)
            w.orphans_removed = sum(1 for k, rep in before.items() if k not in M.sessions and rep[0] == lb.TO_BACKEND
                                    and (rep[1], rep[2], k[12]) in named)
        elif op.kind == "aging_enable":
            assert M.clock == 0 and not any(M.stamps.values())
            self.aging = True
        else:
            raise ValueError(op.kind)
        if op.kind in REMOVALS:
            w.removed = set(before) - set(M.sessions)


# ---- the generator -------------------------------------------------------------------

class _Backs:
    """U.backs for life_cases._batch on services that move: the backward sid of
    client c as its stored session has it, else as a new flow would get it now."""

    def __init__(self, U, M):
        self.U, self.M = U, M

    def __getitem__(self, c):
        s = self.U.clients[c]
        k = WC.sid_key(s)
        rep = self.M.sessions.get(k)
        if rep is not None and rep[0] == lb.TO_BACKEND:
            return LF.sid_of_key(RC.partner(k, rep))
        backs = self.M.services.get(service_of(k))
        if not backs:
            return self.U.backs[c]
        addr, port = backs[LC.jhash(k) % len(backs)][:2]
        return (addr, s[0], port, s[2], s[4])


def _pool(svc, j):
    """Backend j of a service's pool of MAX_PER_SERVICE: life_cases._universe's numbering."""
    return 0xc0a80100 + (svc[0] & 0xff) * 16 + j, 0x901f + j


def _backend_ops(U, world, rng):
    """1 .. 8 ops: a last backend added, a mac or an ifindex replaced, the first,
    a middle or the last backend removed (the only one too: the service goes,
    and a later ADD brings it back), records that name nothing, add-then-remove."""
    have = {s: [b[:2] for b in world.M.services.get(s[0].to_bytes(4, "little") + s[1].to_bytes(2, "little") + bytes([s[2]]), [])]
            for s in U.svcs}
    n, out = int(rng.integers(1, 9)), []

    def record(s, addr, port):
        return BC.rec(s[0], s[1], s[2], addr, port, tuple(rng.integers(0, 256, 6).tolist()), int(rng.integers(1, 4)))

    while len(out) < n:
        s = U.svcs[int(rng.integers(len(U.svcs)))]
        cur = have[s]
        free = [_pool(s, j) for j in range(MAX_PER_SERVICE) if _pool(s, j) not in cur]
        r = int(rng.integers(10))
        if not cur or (len(cur) < 4 and r < 5) or (r < 3 and free):
            b = free[int(rng.integers(len(free)))]
            out.append((BC.ADD, record(s, *b)))
            cur.append(b)
        elif r < 4:
            out.append((BC.ADD, record(s, *cur[int(rng.integers(len(cur)))])))
        elif r < 7 or not free:
            b = cur[(0, len(cur) // 2, len(cur) - 1)[int(rng.integers(3))]]
            out.append((BC.REMOVE, record(s, *b)))
            cur.remove(b)
        elif r < 8:
            out.append((BC.REMOVE, record(s, *free[0]) if rng.integers(2) else BC.rec(0x0f00000f, s[1], s[2], 1, 1)))
        else:
            out += [(BC.ADD, record(s, *free[0])), (BC.REMOVE, record(s, *free[0]))]
    return BC.op_records(out[:8])


def _id_list(shape, U, world, rng):
    """0 .. 6 backends, live ones and ones an update has removed; sometimes one
    twice, sometimes one under the other protocol, sometimes padded with absent
    ids to half of kLdsSetSlots or to one more."""
    M = world.M
    live = [(a, p, s[6]) for s, a, p in world.live()]
    gone = [(a, p, s[6]) for s, a, p in world.taken - world.live()]
    pool = sorted(live) + 2 * sorted(gone)
    ids = [pool[i] for i in rng.permutation(len(pool))[:int(rng.integers(0, 7))].tolist()]
    # every other list, where the table allows it, passes the tombstone bound: the backends with the most flows
    per = collections.Counter((rep[1], rep[2], k[12]) for k, rep in M.sessions.items() if rep[0] == lb.TO_BACKEND)
    most = per.most_common(6)
    if rng.integers(2) and M.tombstones + 2 * sum(n for _, n in most) > shape.slots // LF.session_tombstone_share():
        ids = [b for b, _ in most]
    ids = list(dict.fromkeys(ids))
    if ids and rng.integers(4) == 0:
        ids.append(ids[0])
    if ids and rng.integers(4) == 0:
        ids.append(ids[-1][:2] + (23 - ids[-1][2],))
    pad = int(rng.integers(8))
    if pad < 2:
        ids += [(0x0e000001 + i, 0x1f90 + (i & 15), 6 + 11 * (i & 1)) for i in range(lds_set_slots() // 2 + pad - len(ids))]
    return BC.id_records([ids[i] for i in rng.permutation(len(ids))])


def _max_idle(shape, world, rng, after_batch):
    """Around the recent clock steps: a quantile of the stored ages, so that a
    fifth to a half of the sessions are idle; 0 right after a batch; 0xffffffff.
    Every other time, where the table allows it, the largest of a few quantiles
    at which the expire passes the tombstone bound (tried on a copy of the model)."""
    r = int(rng.integers(12))
    if r < 2:
        return M32
    if r < 4 and after_batch:
        return 0
    M = world.M
    ages = sorted(M.age(k) for k in M.sessions)
    if not ages:
        return int(rng.integers(0, 20))
    if rng.integers(2) and M.tombstones + len(ages) > shape.slots // LF.session_tombstone_share():
        for q in (0.5, 0.3, 0.1):
            trial = copy.deepcopy(M)
            if int(trial.expire(ages[int(q * len(ages))])[RC.COMPACTED]):
                return ages[int(q * len(ages))]
    return ages[min(int(rng.uniform(0.5, 0.8) * len(ages)), len(ages) - 1)]


def _generate(shape):
    rng = np.random.default_rng(shape.seed)
    U = LF._universe(shape, rng)
    U.svcs = list(dict.fromkeys((int(r["vaddr"]), int(r["vport"]), int(r["proto"])) for r in U.backends))
    rules = FC.rules_from_keys(U.acl_keys[:shape.acl_initial], [FC.ACTIONS[i % len(FC.ACTIONS)]
                                                                 for i in range(shape.acl_initial)])
    world = World(shape, U.backends, rules)
    now_U = types.SimpleNamespace(**vars(U))
    now_U.backs = _Backs(U, world.M)
    if shape.enable_from is None:
        world.aging = True
    weights = np.array(shape.weights, dtype=float)
    ops, prev = [], None
    for i in range(shape.n_ops):
        M = world.M
        if i in shape.puts:
            kind = "sessions_put"
        elif i in shape.clear:
            kind = "sessions_clear"
        elif world.aging and not any(o.kind == "clock" for o in ops):
            kind = "clock"                       # the clock's first value
        elif not world.aging and i >= shape.enable_from and M.tombstones and M.sessions:
            kind = "aging_enable"
        else:
            kind = KINDS[int(rng.choice(len(KINDS), p=weights / weights.sum()))]
            if kind in ("clock", "expire") and not world.aging:
                kind = "lb_batch"
        op = types.SimpleNamespace(kind=kind, index=i)
        if kind in ("lb_batch", "lbfw_batch", "lbfw_batch_open"):
            op.kind, op.gate = ("lb_batch", False) if kind == "lb_batch" else ("lbfw_batch", kind == "lbfw_batch")
            # one batch in three runs to max_frames, across the 256-lane tile; the others stay short
            few = shape if rng.integers(3) == 0 else shape._replace(max_frames=120)
            op.umem, op.descs = LF._batch(few, now_U, world, rng)
            op.nif = int(rng.choice([4, 4, 4, 2, 1]))
            op.ingress = int(rng.integers(op.nif))
        elif kind == "firewall_batch":
            op.umem, op.descs = LF._batch(shape, now_U, world, rng, lookups_only=True)
        elif kind == "acl_update":
            op.ops = LF._update(shape, U, world, rng)
        elif kind == "sessions_remove":
            op.keys, op.pair = LF._removal(shape, U, world, rng)
        elif kind == "drain_backend":
            live = sorted(world.live())
            s, addr, port = live[int(rng.integers(len(live)))] if live else (b"\0" * 6 + b"\x06", 1, 1)
            op.addr, op.port = addr, port
            op.proto = s[6] if rng.integers(6) else 23 - s[6]
        elif kind == "sessions_put":
            op.keys, op.values = LF._put(shape, U, world, rng)
        elif kind == "clock":
            first = not any(o.kind == "clock" for o in ops)
            op.now = shape.clock0 if first else (M.clock + int(rng.integers(1, 33))) & M32
        elif kind == "expire":
            op.max_idle = _max_idle(shape, world, rng, prev is not None and prev.kind in BATCHES)
        elif kind == "backends_update":
            op.ops = _backend_ops(U, world, rng)
        elif kind == "drain_backends":
            op.ids = _id_list(shape, U, world, rng)
        world.apply(op)
        ops.append(op)
        prev = op
    return types.SimpleNamespace(shape=shape, name=shape.name, backends=U.backends, rules=rules, ops=ops,
                                 enable_first=shape.enable_from is None)


@functools.lru_cache(maxsize=None)
def script(name):
    """The script of SHAPES[name] with the model's expectations: computed once
    per process and shared; the tests leave it unchanged."""
    return _generate(SHAPES[name])


def describe(op) -> str:
    what = {"clock": lambda: f"{op.now:#x}", "expire": lambda: f"max_idle {op.max_idle:#x}",
            "backends_update": lambda: f"{op.ops.shape[0]} ops", "drain_backends": lambda: f"{op.ids.shape[0]} ids",
            "aging_enable": lambda: ""}.get(op.kind)
    return f"op {op.index} {op.kind} ({what()})" if what else LF.describe(op)


def segments(S):
    """The script cut at its ops without a stream argument: [(ops, the op that ends them or None)]."""
    out, cur = [], []
    for op in S.ops:
        if op.kind in SEGMENT_ENDS:
            out.append((cur, op))
            cur = []
        else:
            cur.append(op)
    out.append((cur, None))
    return out


# ---- what a script exercises, from the model alone --------------------------------------

def coverage(S) -> dict:
    c = collections.Counter(LF.coverage(S))
    state = {}                      # key -> 1 created by a batch, 2 then expired, 3 then created again
    half = lds_set_slots() // 2
    for seg, _ in segments(S):
        for i, op in enumerate(seg):
            w = op.want
            if op.kind == "expire":
                n, compacted = int(w.result[RC.REMOVED]), int(w.result[RC.COMPACTED])
                c["expires_that_remove_and_do_not_compact"] += bool(n and not compacted)
                c["expires_that_compact"] += compacted
                c["idle_sessions_kept_by_their_partner"] += w.idle_kept
                c["expires_of_0_right_after_a_batch"] += bool(op.max_idle == 0 and i and seg[i - 1].kind in BATCHES)
                c["expires_of_0xffffffff"] += op.max_idle == M32
                for k in w.removed:
                    if state.get(k) == 1:
                        state[k] = 2
                # a clock, this expire, a creating batch, in that order within 4 ops of one segment
                for lo in range(max(0, i - 2), i):
                    window, at = seg[lo:lo + 4], i - lo
                    if (any(o.kind == "clock" for o in window[:at])
                            and any(o.kind in BATCHES and o.want.created for o in window[at + 1:])):
                        c["clock_expire_creating_batch_within_4_ops"] += 1
                        break
            elif op.kind in BATCHES:
                if w.aging and w.cause and w.hits:
                    c["aged_stand_downs_with_hits"] += 1
                    c["aged_stand_downs_with_hits_lb"] += op.kind == "lb_batch"
                    c["aged_stand_downs_with_hits_gated"] += bool(op.kind == "lbfw_batch" and op.gate)
                    c["stored_sessions_the_acl_decided_in_gated_stand_downs"] += w.gated_stored
                c["sessions_created_towards_an_added_backend"] += w.to_added
                c["hits_on_sessions_of_a_removed_backend"] += w.orphan_hits
                c["flows_moved_by_a_shorter_list"] += w.moved
                for k in w.created:
                    state[k] = {None: 1, 1: 1, 2: 3, 3: 3}[state.get(k)]
            elif op.kind == "drain_backends":
                c["list_drains_of_a_removed_backend_that_remove"] += bool(w.orphans_removed)
                c["list_drains_that_compact"] += int(w.result[RC.COMPACTED])
                c["lists_of_half_the_lds_set"] += op.ids.shape[0] == half
                c["lists_of_one_more_than_half_the_lds_set"] += op.ids.shape[0] == half + 1
            elif op.kind == "backends_update":
                c["updates"] += 1
                if (0 < i < len(seg) - 1 and seg[i - 1].kind in BATCHES and seg[i + 1].kind in BATCHES
                        and w.services & seg[i - 1].want.services & seg[i + 1].want.services):
                    c["updates_between_two_batches_of_their_service"] += 1
                if c["updates"] == 1:
                    c["first_update_with_batches_on_both_sides_of_its_segment"] = int(
                        any(o.kind in BATCHES for o in seg[:i]) and any(o.kind in BATCHES for o in seg[i + 1:]))
            elif op.kind == "clock":
                c["clock_wraps"] += w.wrapped
            c["max_tombstones"] = max(c["max_tombstones"], w.tombstones)
    for op in S.ops:
        if op.kind == "aging_enable":
            c["enables_after_a_removal_over_sessions_and_tombstones"] += bool(
                op.want.tomb_before and op.want.n_sessions
                and any(o.kind in REMOVALS and int(o.want.result[RC.REMOVED]) for o in S.ops[:op.index]))
    c["keys_created_expired_and_created_again"] = sum(1 for v in state.values() if v == 3)
    return dict(c)


def coverage_gaps(S, cov) -> list:
    """The conditions a script must meet that `cov` does not."""
    need = {"expires_that_remove_and_do_not_compact": 3, "expires_that_compact": 1,
            "idle_sessions_kept_by_their_partner": 10, "expires_of_0_right_after_a_batch": 1, "expires_of_0xffffffff": 1,
            "aged_stand_downs_with_hits": 3, "aged_stand_downs_with_hits_lb": 1, "aged_stand_downs_with_hits_gated": 1,
            "stored_sessions_the_acl_decided_in_gated_stand_downs": 1, "keys_created_expired_and_created_again": 20,
            "sessions_created_towards_an_added_backend": 20, "hits_on_sessions_of_a_removed_backend": 5,
            "flows_moved_by_a_shorter_list": 1, "list_drains_of_a_removed_backend_that_remove": 1,
            "list_drains_that_compact": 1, "clock_expire_creating_batch_within_4_ops": 1,
            "updates_between_two_batches_of_their_service": 1}
    if S.name == "aged":
        need["clock_wraps"] = 1
    if S.name == "churn":
        need.update({k: 1 for k in ("lists_of_half_the_lds_set", "lists_of_one_more_than_half_the_lds_set",
                                    "enables_after_a_removal_over_sessions_and_tombstones",
                                    "first_update_with_batches_on_both_sides_of_its_segment",
                                    "key_lists_within_the_first_stage", "key_lists_past_the_first_stage",
                                    "record_updates_within_the_first_stage", "record_updates_past_the_first_stage")})
    return [f"{k}: {cov.get(k, 0)} < {v}" for k, v in need.items() if cov.get(k, 0) < v]


# ---- one op through the host forms, and the tables against the model ------------------------

def run_host(op, L, A):
    """The op on the host tables of L and A: life_cases.run_host's returns, the
    result words of an expire and of a list drain."""
    H = lb.HOST_TABLE
    if op.kind == "clock":
        return L.clock(op.now, which=H)
    if op.kind == "expire":
        return L.expire(op.max_idle, which=H)
    if op.kind == "backends_update":
        return L.backends_update(ops=op.ops)
    if op.kind == "drain_backends":
        return L.drain_backends(op.ids, which=H)
    if op.kind == "aging_enable":
        return L.aging_enable()
    return LF.run_host(op, L, A)


def same_tables(op, L, A, which, acl_rules) -> str:
    """"" or what differs between the model after `op` and one side's tables:
    the session dump, the ages and the clock once ageing is on, the backends
    dump, and `acl_rules`, that side's ACL dump."""
    w = op.want
    bad = LF.same_tables(op, L.sessions_dump(which), acl_rules)
    if bad:
        return bad
    if w.aging:
        k, a, clock = L.sessions_ages(which)
        if clock != w.clock:
            return f"the clock is {clock:#x}, the model's {w.clock:#x}"
        if k.tobytes() != w.sessions[0]:
            return "the keys of sessions_ages are not the model's"
        want = np.frombuffer(w.ages, dtype=np.uint32)
        diff = np.nonzero(a != want)[0]
        if diff.size:
            return f"{diff.size} ages differ, first at {diff[:8]}: {a[diff[:8]]} != {want[diff[:8]]}"
    if L.backends_dump(which).tobytes() != w.backends:
        return "the backends dump is not the model's"
    return ""
