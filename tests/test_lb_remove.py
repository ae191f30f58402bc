"""Removing sessions from the load balancer's HOST table (include/xsknf_gpu.h
xsknf_gpu_lb_sessions_remove_host, _drain_backend_host, _sessions_clear;
xsknf_amd/csrc/lb.cpp) against the set semantics of tests/lb_remove_cases.py:
after every call the dump equals the model, the result words are exact, and
xsknf_gpu_lb_host finds every survivor and no removed key.
tests/test_gpu_lb_remove.py holds the device table to the same model."""
import ctypes
import errno

import numpy as np
import pytest

from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from xsknf_amd import _lib, lb

H = lb.HOST_TABLE
EMPTY = np.zeros(0, dtype=lb.BACKEND_DTYPE)
CREATED, FAILED = lb.LB_STATS.index("sessions_created"), lb.LB_STATS.index("inserts_failed")


def small(bk=EMPTY):
    """A 64-slot table for 32 sessions, and its model."""
    return lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64), RC.Model(bk, 32, 64)


def put(L, M, ks, vs):
    L.sessions_put(ks, vs)
    M.sessions_put(ks, vs)


def remove(L, M, sids, pair=False):
    k = RC.key_records(sids)
    got, want = L.sessions_remove(k, pair=pair, which=H), M.remove(k, pair)
    assert got.tolist() == want.tolist(), f"result {got} != {want}"
    assert RC.same_dump(L, M, H) and L.info["host_sessions"] == len(M.sessions)
    return got


def check_found(L, M, sids):
    """xsknf_gpu_lb_host on one frame per sid (none towards a service): a stored
    key is rewritten to HIT_IFACE, an absent one passes.  Stores nothing."""
    umem, descs = RC.frames_of(sids)
    v, st = lb.lb_host(umem, descs, L, CC.INGRESS, CC.NIF)
    want = [RC.HIT_IFACE if CC.sid_bytes(s) in M.sessions else CC.PASS_IFACE for s in sids]
    assert v.tolist() == want and int(st[CREATED]) == 0
    assert RC.same_dump(L, M, H)


@pytest.mark.parametrize("kind", ["home", "wrap"])
@pytest.mark.parametrize("where", [[0], [5], [11], [0, 11], [3, 4, 5]])
def test_removal_from_a_probe_chain(kind, where):
    """Head, middle and tail of one chain of twelve, also where the chain wraps
    the table's end: every key further down the chain is still found."""
    sids = RC.chain_keys(kind)
    L, M = small()
    with L:
        put(L, M, *RC.stored(sids))
        check_found(L, M, sids)
        got = remove(L, M, [sids[i] for i in where])
        assert got.tolist() == [len(where), 0]
        assert all((CC.sid_bytes(s) in M.sessions) == (i not in where) for i, s in enumerate(sids))
        check_found(L, M, sids)
        # a removed key goes in again, behind the chain: found, and the others with it
        put(L, M, *RC.stored([sids[where[0]]]))
        check_found(L, M, sids)


def test_absent_duplicate_and_bad_proto():
    sids = RC.chain_keys("home")
    L, M = small()
    with L:
        put(L, M, *RC.stored(sids[:8]))
        assert remove(L, M, sids[8:]).tolist() == [0, 0]                    # absent
        assert remove(L, M, [sids[2]] * 5 + [sids[9]]).tolist() == [1, 0]   # a duplicate counts once
        other = tuple(sids[3][:4]) + (1,)                                   # the key's words with proto 1
        assert remove(L, M, [other, tuple(sids[3][:4]) + (0,), tuple(sids[3][:4]) + (255,)]).tolist() == [0, 0]
        k = RC.key_records([sids[3]])
        k["pad"] = 0xee                                                     # pad is ignored
        assert L.sessions_remove(k, which=H).tolist() == [1, 0] and M.remove(k).tolist() == [1, 0]
        check_found(L, M, sids)


def flows_table(n=6):
    """n flows created by xsknf_gpu_lb_host towards one backend: (L, M, bk, sids)."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, n, seed=11)
    L, M = small(bk)
    umem, descs = RC.frames_of(sids)
    mu = umem.copy()
    v, st = lb.lb_host(umem, descs, L, CC.INGRESS, CC.NIF)
    mv, ms = M.batch(mu, descs, CC.INGRESS, CC.NIF)
    assert np.array_equal(v, mv) and int(st[CREATED]) == 2 * n and RC.same_dump(L, M, H)
    return L, M, bk, sids


def test_pair_on_a_forward_and_on_a_backward_key():
    L, M, bk, sids = flows_table()
    with L:
        assert remove(L, M, [sids[0]], pair=True).tolist() == [2, 0]
        assert remove(L, M, [CC.bwd_sid(bk, sids[1])], pair=True).tolist() == [2, 0]
        assert remove(L, M, [sids[2]]).tolist() == [1, 0]                        # no pair: the backward half stays
        assert CC.sid_bytes(CC.bwd_sid(bk, sids[2])) in M.sessions
        assert remove(L, M, [CC.bwd_sid(bk, sids[2])], pair=True).tolist() == [1, 0]   # its partner is gone already
        # a key listed beside its partner: two, not three or four
        assert remove(L, M, [sids[3], CC.bwd_sid(bk, sids[3]), sids[3]], pair=True).tolist() == [2, 0]
        assert len(M.sessions) == 4


def test_pair_leaves_an_unpaired_entry_and_a_stranger():
    """A forward session stored alone; one whose partner key holds a session of
    the same direction; one whose partner key holds a backward session of
    another service: `pair` removes the listed key alone."""
    bk = CC.one_backend(17)
    a, b, c = RC.new_flows(bk, 3, seed=12)
    L, M = small(bk)
    with L:
        same_dir = LC.session(*CC.bwd_sid(bk, b), lb.TO_BACKEND, 1, 2, (0,) * 6, 0)
        stranger = LC.session(*CC.bwd_sid(bk, c), lb.TO_CLIENT, int(bk[0]["vaddr"]) + 1, int(bk[0]["vport"]), (0,) * 6, 0)
        put(L, M, *CC.sessions([CC.session_of(bk, s, lb.TO_BACKEND) for s in (a, b, c)] + [same_dir, stranger]))
        assert remove(L, M, [a, b, c], pair=True).tolist() == [3, 0]
        assert set(M.sessions) == {CC.sid_bytes(CC.bwd_sid(bk, b)), CC.sid_bytes(CC.bwd_sid(bk, c))}


def test_pair_leaves_a_backward_session_that_another_flow_replaced():
    """Two flows of one client store one backward key (tests/lb_cases.py
    "shared_b"); the later flow's value stands.  `pair` on the earlier flow
    leaves it, `pair` on the later one takes it."""
    rng = np.random.default_rng(13)
    bk, _, fl = LC.ordered_cause(rng, "shared_b")
    umem, descs = LC.pack_packed(fl, rng)
    keys = [LC.frame_sid(f) for f in fl]
    bsid, s1, s2 = keys[1], keys[2], keys[4]
    L, M = small(bk)
    with L:
        mu = umem.copy()
        lb.lb_host(umem, descs, L, 0, 2)
        M.batch(mu, descs, 0, 2)
        assert RC.same_dump(L, M, H) and set(M.sessions) == {bsid, s1, s2}
        assert RC.partner(bsid, M.sessions[bsid]) == s2                    # s2 stored it last
        one = np.zeros(1, dtype=lb.KEY_DTYPE)

        def rec(kb):
            one[0] = (LC._u32(kb, 0), LC._u32(kb, 4), LC._u16(kb, 8), LC._u16(kb, 10), kb[12], (0, 0, 0))
            return one

        got, want = L.sessions_remove(rec(s1), pair=True, which=H), M.remove(rec(s1), True)
        assert got.tolist() == want.tolist() == [1, 0] and RC.same_dump(L, M, H)   # the stranger stays
        got, want = L.sessions_remove(rec(s2), pair=True, which=H), M.remove(rec(s2), True)
        assert got.tolist() == want.tolist() == [2, 0] and not M.sessions and RC.same_dump(L, M, H)


def test_drain_over_mixed_backends_and_both_protocols():
    rng = np.random.default_rng(14)
    bk = LC.make_backends(rng, services=4, per=(2, 4))
    fl = LC.flows_batch(rng, bk, flows=60, filler=10)
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=256, slots=512) as L:
        M = RC.Model(bk, 256, 512)
        mu = umem.copy()
        lb.lb_host(umem, descs, L, 2, 4)
        M.batch(mu, descs, 2, 4)
        assert len(M.sessions) == 120 and RC.same_dump(L, M, H)
        used = sorted({(rep[1], rep[2], k[12]) for k, rep in M.sessions.items() if rep[0] == lb.TO_BACKEND})
        assert len(used) >= 4 and {p for _, _, p in used} == {6, 17}
        # the first backend's address and port under the OTHER protocol, both directions: they stay
        addr, port, proto = used[0]
        other = 6 + 17 - proto
        decoys = [LC.session(1, 2, 3, 4, other, lb.TO_BACKEND, addr, port, (0,) * 6, 0),
                  LC.session(addr, 5, port, 6, other, lb.TO_CLIENT, 7, 8, (0,) * 6, 0)]
        put(L, M, *CC.sessions(decoys))
        for addr, port, proto in used[:3]:
            got, want = L.drain_backend(addr, port, proto, which=H), M.drain(addr, port, proto)
            assert got.tolist() == want.tolist() and int(got[0]) >= 2 and int(got[0]) % 2 == 0
            assert RC.same_dump(L, M, H) and L.info["host_sessions"] == len(M.sessions)
        assert all(LC.key_bytes(d[0]) in M.sessions for d in decoys)
        assert L.drain_backend(1, 1, 6, which=H).tolist() == [0, 0]        # nobody's backend


def test_sessions_clear():
    L, M, bk, sids = flows_table()
    with L:
        remove(L, M, [sids[0]])
        L.sessions_clear(H)
        M.clear()
        assert RC.same_dump(L, M, H) and L.info["host_sessions"] == 0
        put(L, M, *RC.stored(RC.chain_keys("home")))
        check_found(L, M, RC.chain_keys("home"))


def test_every_einval_rule():
    lib = _lib.load()
    E = -errno.EINVAL
    k = RC.key_records(RC.chain_keys("home")[:3])
    res = np.full(4, 99, dtype=np.uint64)
    with lb.LoadBalancer.from_backends(EMPTY, max_sessions=32, slots=64) as L:
        h = L.handle
        assert lib.xsknf_gpu_lb_sessions_remove_host(None, k.ctypes.data, 3, 0, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, None, 3, 0, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, k.ctypes.data, 3, 2, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, k.ctypes.data, 3, 0x80000001, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove(None, k.ctypes.data, 3, 0, None, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove(h, None, 3, 0, None, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove(h, k.ctypes.data, 3, 4, None, None) == E
        assert lib.xsknf_gpu_lb_sessions_remove(h, k.ctypes.data, 3, 0, ctypes.c_void_p(0x1004), None) == E
        assert lib.xsknf_gpu_lb_drain_backend(h, 1, 2, 6, ctypes.c_void_p(0x1004), None) == E
        for proto in (0, 1, 7, 255):
            assert lib.xsknf_gpu_lb_drain_backend_host(h, 1, 2, proto, None) == E
            assert lib.xsknf_gpu_lb_drain_backend(h, 1, 2, proto, None, None) == E
        assert lib.xsknf_gpu_lb_drain_backend_host(None, 1, 2, 6, None) == E
        assert lib.xsknf_gpu_lb_drain_backend(None, 1, 2, 6, None, None) == E
        for which in (-1, 2):
            assert lib.xsknf_gpu_lb_sessions_clear(h, which, None) == E
        assert lib.xsknf_gpu_lb_sessions_clear(None, H, None) == E
        assert (res == 99).all()
        # n == 0: success, zeros in a result, with or without a list
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, None, 0, 1, res.ctypes.data) == 0
        assert res.tolist() == [0, 0, 99, 99]
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, k.ctypes.data, 0, 0, None) == 0
        assert lib.xsknf_gpu_lb_sessions_remove_host(h, k.ctypes.data, 3, 1, None) == 0   # a NULL result
        if L.info["device_bytes"] == 0:   # a host-only object has no device form
            N = -errno.ENODEV
            assert lib.xsknf_gpu_lb_sessions_remove(h, k.ctypes.data, 3, 0, None, None) == N
            assert lib.xsknf_gpu_lb_sessions_remove(h, None, 0, 0, None, None) == N
            assert lib.xsknf_gpu_lb_drain_backend(h, 1, 2, 6, None, None) == N
            assert lib.xsknf_gpu_lb_sessions_clear(h, lb.DEVICE_TABLE, None) == N


def test_reuse_fill_remove_and_fill_again():
    """Eight cycles on the 64-slot table: 16 new flows fill it to max_sessions,
    they are removed four flows at a time, 16 different flows follow.  256
    slots' worth of tombstones in 64 slots: without the rebuild the third fill
    finds no empty slot.  No insert ever fails, and the dump equals the model."""
    bk = CC.one_backend(6)
    flows = RC.new_flows(bk, 8 * 16, seed=15)
    L, M = small(bk)
    compacted = 0
    with L:
        for cycle in range(8):
            sids = flows[16 * cycle:16 * cycle + 16]
            umem, descs = RC.frames_of(sids, seed=cycle)
            mu = umem.copy()
            v, st = lb.lb_host(umem, descs, L, CC.INGRESS, CC.NIF)
            mv, ms = M.batch(mu, descs, CC.INGRESS, CC.NIF)
            assert int(st[FAILED]) == 0 and int(st[CREATED]) == 32 and np.array_equal(st, ms), f"cycle {cycle}"
            assert np.array_equal(v, mv) and RC.same_dump(L, M, H) and L.info["host_sessions"] == 32
            for part in range(0, 16, 4):
                got = remove(L, M, sids[part:part + 4], pair=True)
                assert int(got[RC.REMOVED]) == 8
                compacted += int(got[RC.COMPACTED])
            assert not M.sessions
    assert compacted >= 8   # 8 tombstones a call, the bound is 16: every third call


def test_after_a_compaction():
    """Seventeen of thirty sessions go in one call (17 > 64 / 4): the table is
    rebuilt.  Every survivor is found, a replaced value, a returning key and a
    new key go in, and the dump is right."""
    sids = RC.chain_keys("home") + RC.chain_keys("wrap") + [(9, 9, i, 9, 17) for i in range(1, 7)]
    L, M = small()
    with L:
        put(L, M, *RC.stored(sids))
        assert len(M.sessions) == 30
        got = remove(L, M, sids[::2] + sids[1:5:2])
        assert got.tolist() == [17, 1]
        check_found(L, M, sids)
        ks, vs = RC.stored([sids[1], sids[7], sids[0], (8, 8, 8, 8, 6)])
        vs["port"] += 1
        put(L, M, ks, vs)
        check_found(L, M, sids + [(8, 8, 8, 8, 6)])
        assert remove(L, M, sids, pair=True).tolist() == [15, 0]   # 13 survivors + 2 returned; 15 <= 16 tombstones
        assert remove(L, M, [(8, 8, 8, 8, 6)]).tolist() == [1, 0]
        assert remove(L, M, [(8, 8, 8, 8, 6)]).tolist() == [0, 0]
        put(L, M, *RC.stored(sids[:2]))
        assert remove(L, M, sids[:1]).tolist() == [1, 1]           # the 17th tombstone
        check_found(L, M, sids)
