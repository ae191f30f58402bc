"""The lbfw NF on the host (include/xsknf_gpu.h xsknf_gpu_lbfw_host): against what
the reference's own function left (tests/golden/lbfw_golden.npz, recorded by
tests/golden/make_lbfw_golden.py) byte for byte, against the dict model of
tests/lbfw_cases.py on random batches, against xsknf_gpu_lb_host where the two
NFs must agree, and the rules of the gate.  No GPU."""
import ctypes
import errno

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from xsknf_amd import LBFW_STATS, _lib, lb, lbfw
from xsknf_amd.firewall import Acl

GATED = WC.GATED


@pytest.fixture(scope="module")
def golden():
    return np.load(WC.GOLDEN)


def test_stats_names():
    assert LBFW_STATS is lbfw.LBFW_STATS and LBFW_STATS[7] == "acl_decided" and LBFW_STATS[:7] == lb.LB_STATS[:7]


@pytest.mark.parametrize("mode", ["afxdp", "combined"])
def test_host_equals_the_reference_function(golden, mode):
    """UMEM bytes, verdicts and the sorted session dump after every batch; the
    reference's MODE_COMBINED is acl=None."""
    g = golden
    with lb.LoadBalancer.from_backends(g["backends"], max_sessions=4096) as L, Acl.from_rules(g["rules"]) as A:
        L.sessions_put(g["pre_keys"], g["pre_values"])
        stats = []

        def call(b, umem, descs, ingress, nif):
            v, st = lbfw.lbfw_host(umem, descs, A if mode == "afxdp" else None, L, ingress, nif)
            stats.append(st)
            return umem, v
        WC.run_golden(g, mode, call, L.sessions_dump)
    assert all(WC.identity(st) for st in stats)
    assert all((int(st[GATED]) > 0) == (mode == "afxdp") for st in stats)


def test_fixture_holds_what_it_should(golden):
    """The ACL decides frames of service flows, of flows with pre-put sessions
    and of backward keys, with actions 0, -1 and positive ones; a batch has one
    interface and no batch has none; the gate changes the result."""
    g = golden
    d = FC.acl_dict(g["rules"])
    assert {0, -1} <= set(d.values()) and max(d.values()) > 0
    pre = {LC.key_bytes(k) for k in g["pre_keys"]}
    m = LC.Model(g["backends"], 1 << 20)
    nifs, on_service, on_session, on_backward, acts = [], 0, 0, 0, set()
    made_backward = set()
    for b in range(int(g["batches"])):
        nifs.append(int(g[f"params{b}"][1]))
        for kb in g[f"combined_sessions{b}"]:
            if int(kb[13]) == lb.TO_CLIENT:
                made_backward.add(bytes(kb[:13]))
        umem, descs = g[f"umem{b}"], g[f"descs{b}"]
        for key, v in zip(FC.keys_of(umem, descs), g[f"afxdp_verdicts{b}"]):
            if key is None or key not in d:
                continue
            assert int(v) == d[key]
            acts.add(d[key])
            on_service += (key[4:8] + key[10:12] + key[12:13]) in m.services
            on_session += key in pre
            on_backward += key in made_backward
        assert not np.array_equal(g[f"afxdp_verdicts{b}"], g[f"combined_verdicts{b}"])
    assert on_service > 20 and on_session > 5 and on_backward > 5 and {0, -1} <= acts and max(acts) > 0
    assert 1 in nifs and 0 not in nifs
    assert g["afxdp_sessions2"].shape[0] < g["combined_sessions2"].shape[0]
    # nif 1: the PASS verdicts are 0 where the load balancer's would be -1
    b = nifs.index(1)
    with lb.LoadBalancer.from_backends(g["backends"], max_sessions=4096) as L:
        L.sessions_put(g["pre_keys"], g["pre_values"])
        for i in range(b + 1):
            v, st = lb.lb_host(g[f"umem{i}"].copy(), g[f"descs{i}"], L, *(int(x) for x in g[f"params{i}"]))
        w = g[f"combined_verdicts{b}"]
        assert int(st[2]) > 0 and ((v != w) == ((v == -1) & (w == 0))).all() and int((v != w).sum()) == int(st[2])


def test_host_equals_the_model_on_random_batches():
    rng = np.random.default_rng(131)
    bk = LC.make_backends(rng)
    for trial in range(3):
        fl = LC.flows_batch(rng, bk, flows=80, filler=40)
        sw, _ = LC.sweep_frames(rng, phases=(trial,))
        fl += sw
        umem, descs = LC.pack_packed(fl, rng)
        descs = FC.with_outside(umem, descs, rng)
        ks, vs = LC.sessions_for(fl, rng)
        keys = WC.frame_keys(fl)
        held = keys[::3]
        near = [WC.flip(k, (7 * i) % 96) for i, k in enumerate(keys[1::3])]
        r, d = WC.rules(held + near, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(held) + len(near))])
        nif = (3, 1, 2)[trial]
        with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
            L.sessions_put(ks, vs)
            m = WC.Model(bk, 4096)
            m.sessions_put(ks, vs)
            for b in range(3):   # the second batch finds the first's sessions; the third runs without the gate
                u1, u2 = umem.copy(), umem.copy()
                v1, s1 = lbfw.lbfw_host(u1, descs, A if b < 2 else None, L, b, nif)
                v2, s2 = m.batch(u2, descs, b, nif, d if b < 2 else None)
                assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
                assert WC.identity(s1) and (int(s1[GATED]) > 100) == (b < 2)
            k1, w1 = L.sessions_dump()
            k2, w2 = m.dump()
            assert k1.tobytes() == k2.tobytes() and w1.tobytes() == w2.tobytes()


@pytest.mark.parametrize("nif", [3, 1])
def test_without_an_acl_it_is_the_load_balancer_but_for_pass(nif):
    """acl=None, nif > 1: xsknf_gpu_lb_host byte for byte, sessions and stats
    included.  nif == 1: the same but for the PASS verdicts, 0 and not -1."""
    rng = np.random.default_rng(132)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=60, filler=60)
    sw, _ = LC.sweep_frames(rng, phases=(5,))
    umem, descs = LC.pack_packed(fl + sw, rng)
    descs = FC.with_outside(umem, descs, rng)
    ks, vs = LC.sessions_for(fl + sw, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L1, \
            lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L2:
        for L in (L1, L2):
            L.sessions_put(ks, vs)
        for b in range(2):
            u1, u2 = umem.copy(), umem.copy()
            v1, s1 = lbfw.lbfw_host(u1, descs, None, L1, b, nif)
            v2, s2 = lb.lb_host(u2, descs, L2, b, nif)
            assert np.array_equal(u1, u2) and np.array_equal(s1, s2) and int(s1[GATED]) == 0 and int(s1[2]) > 0
            if nif > 1:
                assert np.array_equal(v1, v2)
            else:
                diff = v1 != v2
                assert int(diff.sum()) == int(s1[2]) and (v1[diff] == 0).all() and (v2[diff] == -1).all()
            assert L1.sessions_dump()[0].tobytes() == L2.sessions_dump()[0].tobytes()
            assert L1.sessions_dump()[1].tobytes() == L2.sessions_dump()[1].tobytes()
        # the two NFs alternate on ONE object: the sessions are the object's
        u1, u2 = umem.copy(), umem.copy()
        v1, s1 = lb.lb_host(u1, descs, L1, 0, 2)
        v2, s2 = lbfw.lbfw_host(u2, descs, None, L2, 0, 2)
        assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and int(s1[4]) == 0


def test_no_interface_is_einval_with_nothing_touched():
    rng = np.random.default_rng(133)
    bk = LC.make_backends(rng, services=2)
    fl = [LC.frame(rng, LC.service_sid(rng, bk)) for _ in range(4)]
    umem, descs = LC.pack_packed(fl, rng)
    lib = _lib.load()
    with lb.LoadBalancer.from_backends(bk, max_sessions=16) as L, Acl.from_rules(FC.random_rules(rng, 8)) as A:
        u = umem.copy()
        v = np.full(4, 0x5eadbeef, dtype=np.int32)
        st = np.full(8, 77, dtype=np.uint64)
        for acl in (A.handle, None):
            assert lib.xsknf_gpu_lbfw_host(u.ctypes.data, u.size, descs.ctypes.data, 4, 0, 0, acl, L.handle,
                                           v.ctypes.data, st.ctypes.data) == -errno.EINVAL
        assert np.array_equal(u, umem) and (v == 0x5eadbeef).all() and (st == 77).all()
        assert L.info["host_sessions"] == 0
        with pytest.raises(_lib.XsknfGpuError):
            lbfw.lbfw_host(u, descs, A, L, 0, 0)
        # the other argument rules are the load balancer's
        assert lib.xsknf_gpu_lbfw_host(None, 0, None, 4, 0, 1, None, L.handle, None, None) == -errno.EINVAL
        assert lib.xsknf_gpu_lbfw_host(None, 0, None, 0, 0, 1, None, None, None, None) == -errno.EINVAL
        assert lib.xsknf_gpu_lbfw_host(None, 0, None, 0, 0, 1, A.handle, L.handle, None, None) == 0
        stb = (ctypes.c_uint64 * 8)()
        f = lib.xsknf_gpu_lbfw_batch
        assert f(None, 0, None, 0, 0, 0, None, L.handle, None, None, 0, stb, None) == -errno.EINVAL   # nif 0, n 0
        assert f(None, 0, None, 0, 0, 1, None, None, None, None, 0, stb, None) == -errno.EINVAL
        assert f(None, 0, None, 0, 0, 1, A.handle, L.handle, None, None, 0, None, None) == -errno.EINVAL
        assert f(8, 0, None, 0, 0, 1, A.handle, L.handle, None, None, 0, stb, None) == -errno.EINVAL   # misaligned
        assert f(None, 0, None, 4, 0, 1, A.handle, L.handle, None, None, 0, stb, None) == -errno.EINVAL
        assert f(None, 0, None, 0, 0, 1, A.handle, L.handle, None, None, 0, stb, None) == 0


def test_an_action_of_zero_is_a_hit():
    """The same service-bound frame: with its sid in the ACL at action 0 the
    verdict is 0, no byte changes, no session is stored and [7] is 1; with a
    rule one bit away it is rewritten and two sessions are stored."""
    rng = np.random.default_rng(134)
    bk = LC.make_backends(rng, services=2, ifaces=4)
    bk["ifindex"] = 3    # (a rewritten frame's verdict is not 0)
    sid = LC.service_sid(rng, bk)
    f = LC.frame(rng, sid)
    umem, descs = LC.pack_packed([f], rng)
    key = WC.sid_key(sid)
    for rule_key, hit in ((key, True), (WC.flip(key, 37), False)):
        r, _ = WC.rules([rule_key], [0])
        with lb.LoadBalancer.from_backends(bk, max_sessions=16) as L, Acl.from_rules(r) as A:
            u = umem.copy()
            v, st = lbfw.lbfw_host(u, descs, A, L, 1, 4)
            if hit:
                assert int(v[0]) == 0 and np.array_equal(u, umem) and L.info["host_sessions"] == 0
                assert [int(x) for x in st] == [1, 0, 0, 0, 0, 0, 0, 1]
            else:
                assert int(v[0]) == 3 and not np.array_equal(u, umem) and L.info["host_sessions"] == 2
                assert [int(x) for x in st] == [1, 1, 0, 0, 2, 0, 0, 0]


def test_the_acl_wins_over_a_stored_session():
    rng = np.random.default_rng(135)
    bk = LC.make_backends(rng, services=2)
    sids = [(int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32)), 1000 + i, 2000, 6 if i % 2 else 17)
            for i in range(6)]
    fl = [LC.frame(rng, s, ihl=5 + i % 3) for i, s in enumerate(sids)]
    umem, descs = LC.pack_packed(fl, rng)
    ks, vs = LC.sessions_for(fl, rng, every=1)
    assert ks.shape[0] == 6
    r, d = WC.rules([WC.sid_key(s) for s in sids[::2]], [-1, 0, 7])
    with lb.LoadBalancer.from_backends(bk, max_sessions=16) as L, Acl.from_rules(r) as A:
        L.sessions_put(ks, vs)
        before = L.sessions_dump()
        u = umem.copy()
        v, st = lbfw.lbfw_host(u, descs, A, L, 0, 2)
        assert [int(x) for x in v[::2]] == [-1, 0, 7] and [int(x) for x in v[1::2]] == [int(x) for x in vs["ifindex"][1::2]]
        starts = (descs["addr"] & ((1 << 48) - 1)) + (descs["addr"] >> 48)
        for i in range(6):
            same = np.array_equal(u[int(starts[i]):int(starts[i]) + len(fl[i])], np.frombuffer(fl[i], dtype=np.uint8))
            assert same == (i % 2 == 0)
        assert [int(x) for x in st] == [6, 3, 0, 0, 0, 0, 0, 3] and WC.identity(st)
        after = L.sessions_dump()
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()


def test_device_call_without_a_device_returns_enodev():
    """In a process that sees no device both objects are host-only."""
    import os
    import subprocess
    import sys
    code = ("import sys, errno, ctypes; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from xsknf_amd import _lib, lb, firewall\n"
            "L = lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=4)\n"
            "A = firewall.Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE))\n"
            "assert L.info['device_bytes'] == 0 and A.info['device_bytes'] == 0\n"
            "buf = (ctypes.c_uint8 * 4096)(); a = (ctypes.addressof(buf) + 15) & ~15\n"
            "f = _lib.load().xsknf_gpu_lbfw_batch\n"
            "r1 = f(a, 64, a + 1024, 1, 0, 1, A.handle, L.handle, a + 2048, a + 2064, 1024, a + 3584, None)\n"
            "r2 = f(a, 64, a + 1024, 1, 0, 1, None, L.handle, a + 2048, a + 2064, 1024, a + 3584, None)\n"
            "print(r1 == -errno.ENODEV, r2 == -errno.ENODEV)\n") % FC.ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.split() == ["True", "True"], out.stdout
