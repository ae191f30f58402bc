"""The model, the rig and the cases of the load balancer's ageing tests
(tests/test_lb_age.py on the host table, tests/test_gpu_lb_age.py on the device
table): xsknf_gpu_lb_aging_enable, _clock, _sessions_expire and _sessions_ages of
include/xsknf_gpu.h.

The model is tests/lb_remove_cases.py's Model plus a clock and a stamp per stored
key.  Rule 11: it walks a batch in index order, decides hit or create from the
frame as it lies before the rewrite, and stamps what the rule names with the
clock; `expire` decides every session on a copy of the table as it stood.  It
shares no code with xsknf_amd/csrc.

A Rig is one LoadBalancer with ageing, the model, and the tables under test: the
host table alone, or the device table and the host table side by side (every
step goes to both; after every step both sessions_ages dumps, both results and
the counts equal the model).  The cases are written once, against a Rig.
"""
import numpy as np

from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from tests import lbfw_cases as WC
from xsknf_amd import lb, lbfw

H, D = lb.HOST_TABLE, lb.DEVICE_TABLE
I, NIF = CC.INGRESS, CC.NIF
M32 = 0xffffffff
REWRITTEN, CREATED, FAILED, ORDERED = 1, 4, 5, 6
GATED = WC.GATED


class Model(RC.Model):
    """RC.Model with the table's clock and {key: stamp}."""

    def __init__(self, backends, max_sessions, slots):
        super().__init__(backends, max_sessions, slots)
        self.clock, self.stamps = 0, {}

    def put(self, key, rep):
        """Rule 9 and _sessions_put: a session stored or replaced is stamped; a refused one is not."""
        ok = super().put(key, rep)
        if ok:
            self.stamps[key] = self.clock
        return ok

    def batch(self, umem, descs, ingress, nif, acl=None, gate=False):
        """The loop one frame at a time.  Before a frame is rewritten: its key, and
        whether the table holds it (rule 7: stamped) -- unless the ACL decides
        the frame (rule 6a: nothing stamped).  gate: lbfw's PASS and gate."""
        size = int(umem.size)
        out, total = [], None
        for i in range(descs.shape[0]):
            addr, ln = int(descs["addr"][i]), int(descs["len"][i])
            off = (addr & ((1 << 48) - 1)) + (addr >> 48)
            hit = None
            if off <= size and ln <= size - off:
                _, key = FC.frame_key(umem[off:off + ln].tobytes())
                if key is not None and not (acl is not None and key in acl) and key in self.sessions:
                    hit = key
            if gate:
                v, st = WC.Model.batch(self, umem, descs[i:i + 1], ingress, nif, acl)
            else:
                v, st = LC.Model.batch(self, umem, descs[i:i + 1], ingress, nif)
            if hit is not None:
                self.stamps[hit] = self.clock
            out.append(v)
            total = st if total is None else total + st
        if total is None:
            total = np.zeros(len(lbfw.LBFW_STATS if gate else lb.LB_STATS), dtype=np.uint64)
        return (np.concatenate(out) if out else np.zeros(0, dtype=np.int32)), total

    def _settle(self, gone):
        for k in gone:
            del self.stamps[k]
        return super()._settle(gone)

    def clear(self):
        super().clear()
        self.stamps.clear()

    def age(self, key):
        return (self.clock - self.stamps[key]) & M32

    def expire(self, max_idle):
        """Idle, and the checked partner -- the table holds the partner key, in the
        opposite direction, with this key as its own partner -- idle too or absent."""
        before = dict(self.sessions)
        gone = set()
        for k, rep in before.items():
            if self.age(k) <= max_idle:
                continue
            pk = RC.partner(k, rep)
            prep = before.get(pk)
            checked = prep is not None and prep[0] != rep[0] and RC.partner(pk, prep) == k
            if checked and self.age(pk) <= max_idle:
                continue
            gone.add(k)
        return self._settle(gone)

    def ages(self):
        """(keys, ages) as xsknf_gpu_lb_sessions_ages orders them."""
        k, _ = self.dump()
        order = sorted(self.sessions, key=lambda kb: (LC._u32(kb, 0), LC._u32(kb, 4), LC._u32(kb, 8), kb[12]))
        return k, np.array([self.age(kb) for kb in order], dtype=np.uint32)


class Rig:
    """dev None: the host table (xsknf_gpu_lb_host, the _host forms).  dev a torch
    device: the device table and the host table; a batch then goes through
    check_batch of tests/test_gpu_lb.py (device == host byte for byte)."""

    def __init__(self, bk, max_sessions, slots, dev=None, enable=True):
        self.L = lb.LoadBalancer.from_backends(bk, max_sessions=max_sessions, slots=slots)
        self.M = Model(bk, max_sessions, slots)
        self.bk, self.dev = bk, dev
        self.tables = (H,) if dev is None else (D, H)
        if enable:
            self.L.aging_enable()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.L.close()

    def put(self, ks, vs):
        self.L.sessions_put(ks, vs)
        self.M.sessions_put(ks, vs)
        self.check()

    def clock(self, now):
        for t in self.tables:
            self.L.clock(now, which=t)
        self.M.clock = now & M32
        self.check()

    def _removal(self, call, want):
        """call(which) on every table under test; every result is the model's."""
        got = [call(t) for t in self.tables]
        if self.dev is not None:
            import torch

            torch.cuda.synchronize()
            got[0] = got[0].cpu().numpy()
        for g, t in zip(got, self.tables):
            assert g.tolist() == want.tolist(), f"table {t}: result {g.tolist()} != {want.tolist()}"
        self.check()
        return want.tolist()

    def expire(self, max_idle):
        return self._removal(lambda t: self.L.expire(max_idle, which=t), self.M.expire(max_idle))

    def remove(self, sids, pair=False):
        k = RC.key_records(sids)
        return self._removal(lambda t: self.L.sessions_remove(k, pair=pair, which=t), self.M.remove(k, pair))

    def drain(self, addr, port, proto):
        return self._removal(lambda t: self.L.drain_backend(addr, port, proto, which=t), self.M.drain(addr, port, proto))

    def batch(self, umem, descs, what="", ordered=0, acl=None, model=None):
        """One batch on every table under test and on the model: (verdicts,
        stats).  acl: (Acl, dict) runs the lbfw NF.  model: the indices of the
        frames the model walks (the others pass or drop by the parse alone,
        which touches no table)."""
        mu = umem.copy()
        gate = acl is not None
        A, adict = acl if gate else (None, None)
        if self.dev is None:
            hu = umem.copy()
            hv, hs = (lbfw.lbfw_host(hu, descs, A, self.L, I, NIF) if gate else lb.lb_host(hu, descs, self.L, I, NIF))
        elif gate:
            from tests.test_gpu_lbfw import check_batch as lbfw_check_batch

            hu, hv, hs = lbfw_check_batch(self.dev, A, self.L, umem, descs, I, NIF, what, ordered=ordered)
        else:
            from tests.test_gpu_lb import check_batch

            hu = None
            hv, hs = check_batch(self.dev, self.L, umem, descs, I, NIF, what, ordered=ordered)
        if model is None:
            mv, ms = self.M.batch(mu, descs, I, NIF, adict, gate)
            assert np.array_equal(hv, mv), f"{what}: the model's verdicts differ"
            assert np.array_equal(hs, ms), f"{what}: the model's counters differ: {hs} != {ms}"
            assert hu is None or np.array_equal(hu, mu), f"{what}: the model's frames differ"
        else:
            mv, ms = self.M.batch(mu, descs[model], I, NIF, adict, gate)
            assert np.array_equal(hv[model], mv) and np.array_equal(hs[1:], ms[1:] + np.array(
                [0, descs.shape[0] - len(model)] + [0] * (len(ms) - 3), dtype=np.uint64)), f"{what}: {hs} != {ms}"
        self.check(what)
        return hv, hs

    def check(self, what=""):
        if self.dev is not None:
            import torch

            torch.cuda.synchronize()
        mk, ma = self.M.ages()
        for t in self.tables:
            k, a, c = self.L.sessions_ages(t)
            assert c == self.M.clock, f"{what}: table {t}: clock {c} != {self.M.clock}"
            assert k.tobytes() == mk.tobytes(), f"{what}: table {t}: the keys are not the model's"
            bad = np.nonzero(a != ma)[0]
            assert bad.size == 0, f"{what}: table {t}: {bad.size} ages differ, first at {bad[:8]}: {a[bad[:8]]} != {ma[bad[:8]]}"
            assert RC.same_dump(self.L, self.M, t), f"{what}: table {t} is not the model's"
        i = self.L.info
        assert i["host_sessions"] == len(self.M.sessions)
        if self.dev is not None:
            assert i["device_sessions"] == len(self.M.sessions)

    def ages_of(self, sids):
        return [self.M.age(CC.sid_bytes(s)) for s in sids]


def flows_rig(make, n, seed, max_sessions=32, slots=64, proto=17):
    """A rig towards one backend and n client sids; nothing stored yet."""
    bk = CC.one_backend(proto)
    return make(bk, max_sessions, slots), bk, RC.new_flows(bk, n, seed=seed)


# ---- the cases: make(bk, max_sessions, slots, enable=True) -> Rig ------------------

def case_enable_on_a_filled_table(make):
    """1.  Sessions stored before ageing is enabled: all ages 0; clock 5: all 5;
    a second enable keeps the stamps."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 8, seed=31)
    with make(bk, 32, 64, enable=False) as R:
        ks, vs = CC.sessions([CC.session_of(bk, s, lb.TO_BACKEND) for s in sids])
        R.L.sessions_put(ks, vs)
        R.M.sessions_put(ks, vs)
        R.L.aging_enable()
        R.check("enable")
        assert R.ages_of(sids) == [0] * 8
        R.clock(5)
        assert R.ages_of(sids) == [5] * 8
        R.L.aging_enable()
        R.check("second enable")
        umem, descs = RC.frames_of(sids[:2])
        R.batch(umem, descs, "two hits at 5")
        R.clock(9)
        R.L.aging_enable()
        R.check("third enable")
        assert R.ages_of(sids) == [4, 4] + [9] * 6


def case_hits(make):
    """2.  Eight flows; at clock 10 a batch hits the forward halves of three:
    those three have age 0, their backward halves and the rest 10."""
    R, bk, sids = flows_rig(make, 8, seed=32)
    with R:
        R.batch(*RC.frames_of(sids), "fill at 0")
        R.clock(10)
        hv, hs = R.batch(*RC.frames_of([sids[1], sids[4], sids[6], sids[4]]), "three hits")
        assert int(hs[CREATED]) == 0 and int(hs[REWRITTEN]) == 4
        assert R.ages_of(sids) == [10, 0, 10, 10, 0, 10, 0, 10]
        assert R.ages_of([CC.bwd_sid(bk, s) for s in sids]) == [10] * 8


def case_new_flows(make):
    """3.  New flows at clock t: both halves age 0.  And a batch on the ordered
    path (a new flow's backward key is a stored session, which an earlier frame
    uses): the replaced backward session carries the new stamp."""
    R, bk, sids = flows_rig(make, 6, seed=33)
    with R:
        R.batch(*RC.frames_of(sids[:2]), "two flows at 0")
        R.clock(7)
        hv, hs = R.batch(*RC.frames_of(sids[2:4] + sids[:1]), "two new flows and a hit at 7")
        assert int(hs[CREATED]) == 4
        assert R.ages_of(sids[:4]) == [0, 7, 0, 0]
        assert R.ages_of([CC.bwd_sid(bk, s) for s in sids[:4]]) == [7, 7, 0, 0]
        back = CC.bwd_sid(bk, sids[4])
        R.put(*CC.sessions([CC.session_of(bk, back, lb.TO_CLIENT, mac=(1, 1, 1, 1, 1, 1), ifindex=2)]))
        R.clock(12)
        old = R.M.sessions[CC.sid_bytes(back)]
        hv, hs = R.batch(*RC.frames_of([back, sids[4], back]), "a stored backward key replaced", ordered=1)
        assert int(hs[CREATED]) == 1 and R.M.sessions[CC.sid_bytes(back)] != old
        assert R.ages_of([sids[4], back]) == [0, 0] and R.ages_of(sids[:1]) == [5]


def case_full_table(make):
    """4.  max_sessions 8, full.  New flows fail and stamp nothing; the clock
    advances, expire makes room, and the same batch creates its sessions."""
    R, bk, sids = flows_rig(make, 7, seed=34, max_sessions=8, slots=64)
    with R:
        R.batch(*RC.frames_of(sids[:4]), "fill")
        assert len(R.M.sessions) == 8
        R.clock(3)
        more = RC.frames_of([sids[4], sids[0], sids[5], sids[4]])
        hv, hs = R.batch(*more, "a full table", ordered=1)
        assert int(hs[FAILED]) == 3 and int(hs[CREATED]) == 0 and len(R.M.sessions) == 8
        assert R.ages_of(sids[:4]) == [0, 3, 3, 3]
        R.clock(20)
        hv, hs = R.batch(*RC.frames_of([sids[0]]), "keep one flow's forward half alive")
        assert R.expire(10) == [6, 0]
        assert set(R.M.sessions) == {CC.sid_bytes(sids[0]), CC.sid_bytes(CC.bwd_sid(bk, sids[0]))}
        hv, hs = R.batch(*more, "room again", ordered=0)
        assert int(hs[FAILED]) == 0 and int(hs[CREATED]) == 4 and len(R.M.sessions) == 6


def case_pair_rule(make):
    """5.  Forward-only traffic keeps both halves; both go once both are idle; an
    unpaired _sessions_put entry expires alone; a backward session that another
    flow replaced decides alone."""
    rng = np.random.default_rng(35)
    bk, _, fl = LC.ordered_cause(rng, "shared_b")
    keys = [LC.frame_sid(f) for f in fl]
    bsid, s1, s2 = keys[1], keys[2], keys[4]
    lone = (0x01010101, 0x02020202, 0x1111, 0x2222, 17)
    with make(bk, 32, 64) as R:
        umem, descs = LC.pack_packed(fl, rng)
        R.batch(umem, descs, "two flows, one backward key", ordered=1)
        assert RC.partner(bsid, R.M.sessions[bsid]) == s2 and len(R.M.sessions) == 3
        R.put(*CC.sessions([LC.session(*lone, lb.TO_BACKEND, 0x0d0d0d0d, 0x7000, (1, 2, 3, 4, 5, 6), RC.HIT_IFACE)]))
        R.clock(10)
        one = [f for f in fl if LC.frame_sid(f) == s2][:1]
        R.batch(*LC.pack_packed(one, rng), "forward-only traffic of the second flow")
        assert R.M.age(s2) == 0 and R.M.age(bsid) == 10 and R.M.age(s1) == 10
        # s1's partner key holds a session whose own partner is s2: s1 decides alone, and so does the lone entry
        assert R.expire(5) == [2, 0]
        assert set(R.M.sessions) == {s2, bsid}
        R.clock(14)
        assert R.expire(5) == [0, 0]          # the backward half is idle (14), the forward half is not (4): both stay
        R.clock(16)
        assert R.expire(5) == [2, 0] and not R.M.sessions


def case_bounds(make):
    """6.  max_idle 0 right after a batch spares what the batch touched;
    0xffffffff removes nothing; stamps at 0xfffffff0 and clock 0x10 read 0x20."""
    R, bk, sids = flows_rig(make, 6, seed=36)
    with R:
        R.clock(0xfffffff0)
        R.batch(*RC.frames_of(sids[:4]), "four flows just below the wrap")
        R.clock(0x10)
        assert R.ages_of(sids[:4]) == [0x20] * 4
        assert R.expire(0xffffffff) == [0, 0]
        assert R.expire(0x20) == [0, 0]
        hv, hs = R.batch(*RC.frames_of([sids[0], CC.bwd_sid(bk, sids[1]), sids[4]]), "a hit each way and a new flow")
        assert int(hs[CREATED]) == 2
        assert R.expire(0) == [4, 0]          # flows 2 and 3; 0 and 1 were touched on one side, 4 is new
        assert len(R.M.sessions) == 6
        assert R.expire(0x1f) == [0, 0]
        R.clock(0x11)
        assert R.expire(0) == [6, 0]


def case_rebuild(make, trigger):
    """7.  64 slots, 32 sessions; a removal buries 17, more than 64 / 4: COMPACTED
    and the survivors' ages unchanged; a later expire removes the model's set."""
    bk = RC.chain_service(backends=2)
    sids = RC.new_flows(bk, 16, seed=37)
    with make(bk, 32, 64) as R:
        for t, part in enumerate((sids[:5], sids[5:11], sids[11:])):
            R.clock(10 * t)
            R.batch(*RC.frames_of(part), f"flows at {10 * t}")
        assert len(R.M.sessions) == 32
        lone = (0x01010101, 0x02020202, 0x1111, 0x2222, 6)
        assert R.remove([sids[15]], pair=True) == [2, 0]
        R.clock(5)
        R.put(*CC.sessions([LC.session(*lone, lb.TO_BACKEND, 0x0d0d0d0d, 0x7000, (1, 2, 3, 4, 5, 6), RC.HIT_IFACE)]))
        R.clock(30)
        if trigger == "expire":
            assert R.expire(22) == [11, 0]    # the five flows of clock 0 (age 30) and the lone entry (25)
            assert R.expire(19) == [12, 1]    # the six of clock 10: 25 tombstones
        elif trigger == "remove":
            assert R.remove(sids[:8], pair=True) == [16, 1]
        else:
            per = [sum(1 for rep in R.M.sessions.values() if rep[0] == lb.TO_BACKEND and rep[1] == int(r["addr"]))
                   for r in bk]
            which = int(np.argmax(per))
            assert 2 * per[which] + 2 > 16
            assert R.drain(int(bk[which]["addr"]), int(bk[which]["port"]), 6) == [2 * per[which], 1]
        left = [s for s in sids if CC.sid_bytes(s) in R.M.sessions]
        assert left and set(R.ages_of(left)) <= {30, 20, 10}
        R.batch(*RC.frames_of(left[:2]), "hits after the rebuild")
        R.clock(41)
        got = R.expire(15)                    # the flows that were not hit: whatever the model says, at least two
        assert got[0] >= 4 and got[1] == 0 and all(CC.sid_bytes(s) in R.M.sessions for s in left[:2])
        R.clock(100)
        R.expire(0)
        assert not R.M.sessions


def case_lbfw(make, acl_of):
    """10.  The lbfw NF: a frame the ACL decides stamps nothing, hit or new flow;
    the others stamp as the load balancer's.  acl_of(rules) -> Acl."""
    R, bk, sids = flows_rig(make, 8, seed=38)
    with R:
        R.batch(*RC.frames_of(sids[:4]), "fill")
        R.clock(6)
        rules, adict = WC.rules([WC.sid_key(s) for s in (sids[1], sids[5], CC.bwd_sid(bk, sids[2]))], [0, -1, 2])
        with acl_of(rules) as A:
            batch = [sids[0], sids[1], sids[4], sids[5], CC.bwd_sid(bk, sids[2]), CC.bwd_sid(bk, sids[3])]
            hv, hs = R.batch(*RC.frames_of(batch), "lbfw", acl=(A, adict))
            assert int(hs[GATED]) == 3 and int(hs[CREATED]) == 2
        assert R.ages_of(sids[:5]) == [0, 6, 6, 6, 0] and CC.sid_bytes(sids[5]) not in R.M.sessions
        assert R.ages_of([CC.bwd_sid(bk, s) for s in sids[:5]]) == [6, 6, 6, 0, 0]
        assert R.expire(3) == [4, 0]


def case_mixed_run(make, seed, steps=60):
    """11.  `steps` steps drawn from batch, clock, expire, remove, drain, put on a
    table of at most 256 slots; after every step every table equals the model."""
    rng = np.random.default_rng(seed)
    slots = int(rng.choice([64, 128, 256]))
    bk = RC.chain_service(backends=3)
    pool = RC.new_flows(bk, 96, seed=seed + 1)
    lone = [(0x01010101 + i, 0x02020202, 0x1111, 0x2222, 6) for i in range(8)]
    now = int(rng.integers(0, 1 << 32))
    with make(bk, slots // 2, slots) as R:
        R.clock(now)
        for step in range(steps):
            op = rng.choice(["batch", "batch", "batch", "clock", "clock", "expire", "expire", "remove", "drain", "put"])
            what = f"seed {seed} step {step} {op}"
            if op == "batch":
                pick = [pool[j] for j in rng.integers(0, len(pool), int(rng.integers(1, 24)))]
                pick = [CC.bwd_sid(bk[k:k + 1], s) if rng.integers(4) == 0 else s
                        for s, k in zip(pick, rng.integers(0, 3, len(pick)))]
                umem, descs = RC.frames_of(pick, seed=step)
                R.batch(umem, descs, what, ordered=_stands_down(R, pick))
            elif op == "clock":
                now = (now + int(rng.integers(1, 12))) & M32
                R.clock(now)
            elif op == "expire":
                R.expire(int(rng.integers(0, 20)))
            elif op == "remove":
                R.remove([pool[j] for j in rng.integers(0, len(pool), 6)], pair=bool(rng.integers(2)))
            elif op == "drain":
                r = bk[int(rng.integers(3))]
                R.drain(int(r["addr"]), int(r["port"]), 6)
            else:
                free = slots // 2 - len(R.M.sessions)
                some = [s for s in (lone[j] for j in rng.integers(0, 8, 3)) if CC.sid_bytes(s) in R.M.sessions or free > 3]
                if some:
                    R.put(*RC.stored(some))


def _stands_down(R, pick):
    """Whether the batch of client flows and backward frames `pick` leaves the
    parallel path (kernel_lb.h): a new flow's backward key is a stored session
    (its forward half was removed alone), or sessions + new keys > max_sessions."""
    new, replaces = set(), False
    for s in pick:
        k = CC.sid_bytes(s)
        if k in R.M.sessions or k[4:8] + k[10:12] + k[12:13] not in R.M.services:
            continue
        back = CC.sid_bytes(CC.bwd_sid(R.bk[LC.jhash(k) % len(R.bk):][:1], s))
        replaces |= back in R.M.sessions
        new |= {k, back}
    return int(replaces or len(R.M.sessions) + len(new) > R.M.max_sessions)
