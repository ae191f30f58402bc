"""The services and backends of a live load balancer, and the list drain, on the
host copy and the host table (include/xsknf_gpu.h xsknf_gpu_lb_backends_update,
_backends_dump, _drain_backends_host; xsknf_amd/csrc/lb.cpp) against the model of
tests/lb_backends_cases.py.  After every update the dump is the model's, a batch
of new flows through xsknf_gpu_lb_host gives the model's frames, verdicts and
sessions, and an object created from the edited list gives the same."""
import ctypes
import errno

import numpy as np
import pytest

from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from tests import lb_backends_cases as BC
from xsknf_amd import _lib, lb

ADD, REMOVE, H, I, NIF = BC.ADD, BC.REMOVE, BC.H, BC.I, BC.NIF
REWRITTEN, PASSED, CREATED = 1, 2, 4
V1, V2 = (0x0a00000a, 0x5000, 6), (0x0b00000b, 0x5100, 17)


def b(svc, i, **kw):
    """Backend i of service svc: an address and a port of its own, interface 1 + i % 2."""
    kw.setdefault("ifindex", 1 + i % 2)
    kw.setdefault("mac", (2, 4, 6, 8, 10, 12 + i))
    return BC.rec(*svc, 0xc0a80a01 + i, 0x1f90 + i, **kw)


def update(L, M, ops):
    o = BC.op_records(ops)
    L.backends_update(ops=o)
    M.update(o)
    assert BC.same_backends(L, M), "the host copy is not the model's"
    i = L.info
    assert (i["services"], i["backends"]) == (len(M.services), sum(len(v) for v in M.services.values()))


def batch(L, M, sids, what):
    """One batch on the object, the model and an object made from the edited
    list with the object's sessions: all three agree, byte for byte."""
    umem, descs = RC.fast_frames(sids)
    ks, vs = L.sessions_dump(H)
    with lb.LoadBalancer.from_backends(M.record_list(), max_sessions=M.max_sessions, slots=M.slots) as F:
        F.sessions_put(ks, vs)
        fu = umem.copy()
        fv, fs = lb.lb_host(fu, descs, F, I, NIF)
        fk = F.sessions_dump(H)
    mu = umem.copy()
    mv, ms = M.batch(mu, descs, I, NIF)
    hv, hs = lb.lb_host(umem, descs, L, I, NIF)
    assert np.array_equal(hv, mv) and np.array_equal(hs, ms) and np.array_equal(umem, mu), f"{what}: not the model's"
    assert np.array_equal(hv, fv) and np.array_equal(hs, fs) and np.array_equal(umem, fu), f"{what}: not a fresh object's"
    assert RC.same_dump(L, M, H), f"{what}: the sessions are not the model's"
    k, v = L.sessions_dump(H)
    assert k.tobytes() == fk[0].tobytes() and v.tobytes() == fk[1].tobytes()
    return hv, hs


def make(recs, max_sessions=2048, slots=4096):
    r = BC.records(recs)
    return lb.LoadBalancer.from_backends(r, max_sessions=max_sessions, slots=slots), BC.Model(r, max_sessions, slots)


def test_add_to_a_new_service_as_last_backend_and_in_place():
    L, M = make([b(V1, 0), b(V1, 1)])
    with L:
        f1, f2 = BC.flows_to(*V1, 60, seed=1), BC.flows_to(*V2, 40, seed=2)
        hv, hs = batch(L, M, f1[:20] + f2[:10], "before")
        assert int(hs[PASSED]) == 10 and int(hs[CREATED]) == 40
        update(L, M, [(ADD, b(V2, 0))])                       # a new service
        hv, hs = batch(L, M, f2[10:20], "the new service")
        assert int(hs[REWRITTEN]) == 10 and int(hs[CREATED]) == 20
        update(L, M, [(ADD, b(V1, 2))])                       # the last backend of its service
        assert [x[0] for x in M.services[BC.svc_key(BC.records([b(V1, 0)])[0])]] == [0xc0a80a01, 0xc0a80a02, 0xc0a80a03]
        new = f1[20:50]
        assert {BC.choice(s, 3) for s in new} == {0, 1, 2}
        batch(L, M, new, "three backends")
        update(L, M, [(ADD, b(V1, 1, mac=(9, 9, 9, 9, 9, 9), ifindex=3))])   # mac and ifindex replaced, the number kept
        assert L.info["backends"] == 4
        mine = [s for s in f1[50:60] if BC.choice(s, 3) == 1]
        assert mine
        hv, hs = batch(L, M, mine, "the replaced record")
        assert (hv == 3).all()
        # the sessions stored before keep what they were stored with
        old = [s for s in f1[:20] if BC.choice(s, 2) == 1]
        hv, hs = batch(L, M, old, "old sessions")
        assert int(hs[CREATED]) == 0 and (hv == 2).all()


@pytest.mark.parametrize("where", [0, 2, 4])
def test_remove_renumbers_the_later_backends(where):
    """Five backends; the first, a middle or the last goes.  New flows pick
    among four by jhash % 4: some land on the record they would have had, some
    on another.  The removed backend's stored sessions still rewrite."""
    L, M = make([b(V1, i, ifindex=10 + i) for i in range(5)])
    with L:
        before = BC.flows_to(*V1, 50, seed=3)
        hv0, _ = batch(L, M, before, "five backends")
        update(L, M, [(REMOVE, b(V1, where, mac=(0,) * 6, ifindex=77))])   # mac and ifindex are ignored
        left = [i for i in range(5) if i != where]
        new = BC.flows_to(*V1, 200, seed=4)
        same = [s for s in new if left[BC.choice(s, 4)] == BC.choice(s, 5)]
        moved = [s for s in new if BC.choice(s, 5) != where and left[BC.choice(s, 4)] != BC.choice(s, 5)]
        assert len(same) >= 5 and len(moved) >= 5
        hv, hs = batch(L, M, new, "four backends")
        assert hv.tolist() == [10 + left[BC.choice(s, 4)] for s in new]
        hv1, hs1 = batch(L, M, before, "the flows from before")
        assert int(hs1[CREATED]) == 0 and np.array_equal(hv1, hv0) and (hv0 == 10 + where).any()


def test_remove_the_only_backend_and_absent_ones():
    L, M = make([b(V1, 0), b(V2, 0), b(V2, 1)])
    with L:
        update(L, M, [(REMOVE, b(V1, 3)), (REMOVE, BC.rec(0x0c0c0c0c, 1, 6, 1, 1))])   # absent backend, absent service
        assert L.info["services"] == 2 and L.info["backends"] == 3
        update(L, M, [(REMOVE, BC.rec(V1[0], V1[1], 17, 0xc0a80a01, 0x1f90))])          # the other protocol: absent
        assert L.info["backends"] == 3
        update(L, M, [(REMOVE, b(V1, 0))])
        assert L.info["services"] == 1
        hv, hs = batch(L, M, BC.flows_to(*V1, 10, seed=5) + BC.flows_to(*V2, 10, seed=6), "one service left")
        assert int(hs[PASSED]) == 10 and (hv[:10] == CC.PASS_IFACE).all() and int(hs[CREATED]) == 20
        update(L, M, [(REMOVE, b(V2, 0)), (REMOVE, b(V2, 1))])
        assert L.info["services"] == 0 and L.backends_dump().size == 0
        hv, hs = batch(L, M, BC.flows_to(*V2, 10, seed=7), "no service left")
        assert int(hs[PASSED]) == 10
        update(L, M, [(ADD, b(V1, 4))])                                                  # and back
        hv, hs = batch(L, M, BC.flows_to(*V1, 10, seed=8), "a service again")
        assert int(hs[REWRITTEN]) == 10


def test_duplicate_records_from_create():
    """{addr, port} twice in one service (numbers 0 and 2 of three): an ADD
    replaces both, a REMOVE takes both and the one between moves down."""
    L, M = make([b(V1, 0), b(V1, 1), b(V1, 0, ifindex=5)])
    with L:
        batch(L, M, BC.flows_to(*V1, 30, seed=9), "two of three are one backend")
        update(L, M, [(ADD, b(V1, 0, ifindex=9))])
        d = L.backends_dump()
        assert d["ifindex"].tolist() == [9, 2, 9] and L.info["backends"] == 3
        hv, hs = batch(L, M, BC.flows_to(*V1, 30, seed=10), "both replaced")
        assert set(hv.tolist()) == {9, 2}
        update(L, M, [(REMOVE, b(V1, 0))])
        assert L.backends_dump()["ifindex"].tolist() == [2]
        batch(L, M, BC.flows_to(*V1, 10, seed=11), "one left")


def test_add_and_remove_of_one_backend_in_one_call():
    L, M = make([b(V1, 0), b(V1, 1)])
    with L:
        update(L, M, [(ADD, b(V1, 2)), (REMOVE, b(V1, 2))])
        assert L.info["backends"] == 2
        update(L, M, [(REMOVE, b(V1, 0)), (ADD, b(V1, 0))])      # the reverse: it returns as the LAST backend
        assert L.backends_dump()["addr"].tolist() == [0xc0a80a02, 0xc0a80a01]
        batch(L, M, BC.flows_to(*V1, 40, seed=12), "the order changed")
        update(L, M, [(REMOVE, b(V2, 0)), (ADD, b(V2, 0)), (REMOVE, b(V1, 1)), (REMOVE, b(V1, 0)), (ADD, b(V1, 3))])
        assert L.info["services"] == 2 and L.backends_dump()["addr"].tolist() == [0xc0a80a04, 0xc0a80a01]
        batch(L, M, BC.flows_to(*V1, 10, seed=13) + BC.flows_to(*V2, 10, seed=14), "both services")
        L.backends_update(add=BC.records([b(V1, 0)]), remove=BC.records([b(V1, 3)]))   # the removals first
        M.update(BC.op_records([(REMOVE, b(V1, 3)), (ADD, b(V1, 0))]))
        assert BC.same_backends(L, M) and L.info["backends"] == 2


@pytest.mark.parametrize("gone", [(0, 1), (1, 0), (1, 2)])
def test_services_of_one_probe_chain(gone):
    """Four services whose slots collide in the 2048-slot table, made in chain
    order.  Two go, one update each; after each the rest are still found."""
    vaddrs = BC.colliding_services(4)
    svcs = [(v, 0x5000, 6) for v in vaddrs]
    homes = CC.acl_hash(np.array(vaddrs, dtype=np.uint64), 0x5000 | 6 << 16, 0, 0) & np.uint32(2047)
    assert len(set(homes.tolist())) == 1
    L, M = make([b(s, i) for i, s in enumerate(svcs)])
    with L:
        alive = list(range(4))
        for step, g in enumerate(gone):
            victim = alive.pop(g)
            update(L, M, [(REMOVE, b(svcs[victim], victim))])
            sids = [s for j in range(4) for s in BC.flows_to(*svcs[j], 6, seed=20 + 4 * step + j)]
            hv, hs = batch(L, M, sids, f"after service {victim} went")
            assert int(hs[REWRITTEN]) == 6 * len(alive) and int(hs[PASSED]) == 24 - 6 * len(alive)
        update(L, M, [(ADD, b(svcs[victim], 7))])
        hv, hs = batch(L, M, BC.flows_to(*svcs[victim], 6, seed=40), "it returns")
        assert int(hs[REWRITTEN]) == 6


def raw_update(L, ops, n=None, handle=True):
    o = BC.op_records(ops)
    return _lib.load().xsknf_gpu_lb_backends_update(L.handle if handle else None, o.ctypes.data if o.size else None,
                                                    o.size if n is None else n, None)


def test_einval_changes_nothing_and_n_zero():
    L, M = make([b(V1, 0), b(V2, 0)])
    with L:
        before = L.backends_dump().tobytes()
        bad_op = BC.op_records([(ADD, b(V1, 1)), (ADD, b(V1, 2))])
        bad_op["op"][1] = 2
        lib = _lib.load()
        assert lib.xsknf_gpu_lb_backends_update(L.handle, bad_op.ctypes.data, 2, None) == -errno.EINVAL
        assert raw_update(L, [(ADD, b(V1, 1))], handle=False) == -errno.EINVAL
        assert raw_update(L, [], n=3) == -errno.EINVAL                                      # NULL ops, n > 0
        assert raw_update(L, [(ADD, b(V1, 1)), (ADD, BC.rec(1, 2, 7, 3, 4))]) == -errno.EINVAL
        assert raw_update(L, [(REMOVE, b(V1, 0)), (REMOVE, BC.rec(1, 2, 1, 3, 4))]) == -errno.EINVAL
        assert L.backends_dump().tobytes() == before and BC.same_backends(L, M)
        assert raw_update(L, []) == 0 and L.backends_dump().tobytes() == before
        n = ctypes.c_uint32(0)
        r = np.zeros(2, dtype=lb.BACKEND_DTYPE)
        assert lib.xsknf_gpu_lb_backends_dump(L.handle, 2, r.ctypes.data, 2, ctypes.byref(n)) == -errno.EINVAL
        assert lib.xsknf_gpu_lb_backends_dump(L.handle, H, None, 2, ctypes.byref(n)) == -errno.EINVAL
        assert lib.xsknf_gpu_lb_backends_dump(L.handle, H, r.ctypes.data, 2, None) == -errno.EINVAL
        assert lib.xsknf_gpu_lb_backends_dump(L.handle, H, r.ctypes.data, 1, ctypes.byref(n)) == -errno.ENOSPC
        assert n.value == 2 and r[0].tobytes() == L.backends_dump()[0].tobytes() and r[1].tobytes() == bytes(24)


def test_enospc_at_the_service_and_the_record_maxima():
    svcs = BC.records([BC.rec(0x0a000000 + i, 80, 6, 1 + i, 9) for i in range(lb.MAX_SERVICES + 1)])
    with lb.LoadBalancer.from_backends(svcs[:lb.MAX_SERVICES - 1], max_sessions=16, slots=64) as L:
        L.backends_update(add=svcs[lb.MAX_SERVICES - 1:lb.MAX_SERVICES])                    # exactly 1024
        assert L.info["services"] == lb.MAX_SERVICES
        before = L.backends_dump().tobytes()
        with pytest.raises(_lib.XsknfGpuError, match="rc=-28"):
            L.backends_update(add=svcs[lb.MAX_SERVICES:])                                    # 1025
        assert L.backends_dump().tobytes() == before and L.info["services"] == lb.MAX_SERVICES
        L.backends_update(remove=svcs[:1], add=svcs[lb.MAX_SERVICES:])                       # one out, one in
        d = L.backends_dump()
        assert L.info["services"] == lb.MAX_SERVICES and d.tobytes() == svcs[1:].tobytes()
        # every service is still found: one flow each
        sids = [(0x01010101 + i, int(r["vaddr"]), 1000, 80, 6) for i, r in enumerate(svcs[1:201])]
        v, st = lb.lb_host(*RC.fast_frames(sids), L, I, NIF)
        assert int(st[REWRITTEN]) == 200
    many = np.zeros(lb.MAX_BACKENDS + 1, dtype=lb.BACKEND_DTYPE)
    many["vaddr"], many["vport"], many["proto"], many["port"] = 0x0a000001, 80, 6, 9
    many["addr"] = np.arange(1, lb.MAX_BACKENDS + 2)
    with lb.LoadBalancer.from_backends(many[:lb.MAX_BACKENDS - 1], max_sessions=16, slots=64) as L:
        L.backends_update(add=many[lb.MAX_BACKENDS - 1:lb.MAX_BACKENDS])                     # exactly 131072
        assert L.info["backends"] == lb.MAX_BACKENDS
        before = L.backends_dump().tobytes()
        assert before == many[:lb.MAX_BACKENDS].tobytes()
        with pytest.raises(_lib.XsknfGpuError, match="rc=-28"):
            L.backends_update(add=many[lb.MAX_BACKENDS:])                                    # 131073
        assert L.backends_dump().tobytes() == before and L.info["backends"] == lb.MAX_BACKENDS
        L.backends_update(remove=many[5:6], add=many[lb.MAX_BACKENDS:])
        assert L.backends_dump().tobytes() == np.concatenate([many[:5], many[6:]]).tobytes()


# ---- the list drain on the host table ---------------------------------------------

def drain(L, M, ids):
    i = BC.id_records(ids)
    got, want = L.drain_backends(i, which=H), M.drain_list(i)
    assert got.tolist() == want.tolist(), f"{got.tolist()} != {want.tolist()}"
    assert RC.same_dump(L, M, H), "the host table is not the model's"
    return want.tolist()


def drain_case():
    """Eighty backends in two services that share addresses: V1's backend i and
    V2's backend i are one address with different ports, and V2 is UDP with,
    for i < 8, V1's very {addr, port}."""
    recs = [b(V1, i) for i in range(40)]
    recs += [BC.rec(*V2, 0xc0a80a01 + i, 0x1f90 + i if i < 8 else 0x2f90 + i) for i in range(40)]
    return recs


@pytest.mark.parametrize("n", [0, 1, 2, 70])
def test_host_list_drain(n):
    recs = drain_case()
    L, M = make(recs)
    with L:
        sids = BC.flows_to(*V1, 300, seed=50) + BC.flows_to(*V2, 300, seed=51)
        batch(L, M, sids, "fill")
        lone = RC.stored([(7, 8, 9, 10, 6), (11, 12, 13, 14, 17)])   # unpaired entries towards no backend of the list
        stray = CC.sessions([LC.session(21, 22, 23, 24, 6, lb.TO_BACKEND, 0xc0a80a01, 0x1f90, (1,) * 6, 1),
                             LC.session(0xc0a80a01, 26, 0x1f90, 28, 17, lb.TO_CLIENT, 5, 6, (1,) * 6, 1)])
        for ks, vs in (lone, stray):                                  # and two that name backend 0 without a partner
            L.sessions_put(ks, vs)
            M.sessions_put(ks, vs)
        ids = BC.backend_ids(recs)
        assert len(ids) == 80
        if n == 2:
            listed = [ids[0], ids[0]]                                 # a duplicate counts once
        else:
            listed = (ids[:35] + ids[40:75])[:n]
        count = len(M.sessions)
        got = drain(L, M, listed)
        if n == 0:
            assert got == [0, 0] and len(M.sessions) == count
        else:
            assert got[0] > 0 and got[0] == count - len(M.sessions)
            assert CC.sid_bytes((21, 22, 23, 24, 6)) not in M.sessions                       # TCP backend 0 is listed
            assert (CC.sid_bytes((0xc0a80a01, 26, 0x1f90, 28, 17)) in M.sessions) == (n < 70)   # the UDP one only at 70
        assert CC.sid_bytes((7, 8, 9, 10, 6)) in M.sessions
        hv, hs = batch(L, M, sids, "after the drain")
        assert int(hs[CREATED]) == got[0] - (2 if n == 70 else 1 if n else 0)


def test_host_list_drain_crosses_the_tombstone_bound():
    """slots 256: 60 flows are 120 sessions.  A first drain leaves 40 tombstones
    (no rebuild), the second passes 64 and rebuilds."""
    recs = [b(V1, i) for i in range(6)]
    L, M = make(recs, max_sessions=128, slots=256)
    with L:
        sids = BC.flows_to(*V1, 60, seed=52)
        per = [sum(1 for s in sids if BC.choice(s, 6) == i) for i in range(6)]
        batch(L, M, sids, "fill")
        ids = BC.backend_ids(recs)
        order = sorted(range(6), key=lambda i: per[i])
        first, k = [], 0
        while 2 * sum(per[i] for i in first + [order[k]]) <= 64:
            first.append(order[k])
            k += 1
        rest = [i for i in range(6) if i not in first]
        assert first and 2 * sum(per) > 64
        assert drain(L, M, [ids[i] for i in first]) == [2 * sum(per[i] for i in first), 0]
        assert drain(L, M, [ids[i] for i in rest]) == [2 * sum(per[i] for i in rest), 1]
        assert not M.sessions and M.tombstones == 0
        batch(L, M, sids, "again")


def test_list_drain_errors():
    L, M = make([b(V1, 0)])
    with L:
        lib = _lib.load()
        ids = BC.id_records([(1, 2, 6), (1, 2, 7)])
        res = np.full(2, 9, dtype=np.uint64)
        assert lib.xsknf_gpu_lb_drain_backends_host(L.handle, ids.ctypes.data, 2, res.ctypes.data) == -errno.EINVAL
        assert lib.xsknf_gpu_lb_drain_backends_host(None, ids.ctypes.data, 1, res.ctypes.data) == -errno.EINVAL
        assert lib.xsknf_gpu_lb_drain_backends_host(L.handle, None, 1, res.ctypes.data) == -errno.EINVAL
        big = np.zeros(lb.MAX_BACKENDS + 1, dtype=lb.BACKEND_ID_DTYPE)
        big["proto"] = 6
        assert lib.xsknf_gpu_lb_drain_backends_host(L.handle, big.ctypes.data, big.size, res.ctypes.data) == -errno.EINVAL
        assert res.tolist() == [9, 9]
        assert lib.xsknf_gpu_lb_drain_backends_host(L.handle, big.ctypes.data, lb.MAX_BACKENDS, res.ctypes.data) == 0
        assert res.tolist() == [0, 0]
        assert lib.xsknf_gpu_lb_drain_backends_host(L.handle, None, 0, None) == 0
        ids["pad"] = 0xff                                             # pad is ignored
        ks, vs = CC.sessions([LC.session(21, 22, 23, 24, 6, lb.TO_BACKEND, 1, 2, (1,) * 6, 1)])
        L.sessions_put(ks, vs)
        assert L.drain_backends(ids[:1], which=H).tolist() == [1, 0]
