"""The load balancer NF on the host (include/xsknf_gpu.h xsknf_gpu_lb_host and
the xsknf_gpu_lb_* object calls): against what the reference's own function
left (tests/golden/lb_golden.npz, recorded by tests/golden/make_lb_golden.py)
byte for byte, against the dict model of tests/lb_cases.py on random batches,
and the error rules.  No GPU."""
import ctypes
import errno

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import lb_cases as LC
from xsknf_amd import _lib, lb


@pytest.fixture(scope="module")
def golden():
    return np.load(LC.GOLDEN)


def golden_dump(g):
    """The fixture's final sessions as (keys, values) in the dump's order."""
    fk, fv = g["final_keys"], g["final_values"]
    k = np.zeros(fk.shape[0], dtype=lb.KEY_DTYPE)
    v = np.zeros(fk.shape[0], dtype=lb.VALUE_DTYPE)
    k.view(np.uint8).reshape(-1, 16)[:, :13] = fk
    raw = v.view(np.uint8).reshape(-1, 16)
    raw[:, 0:4] = fv[:, 4:8]      # addr
    raw[:, 4:6] = fv[:, 8:10]     # port
    raw[:, 6:8] = fv[:, 16:18]    # ifindex
    raw[:, 8:14] = fv[:, 10:16]   # mac
    raw[:, 14] = fv[:, 0]         # dir (an int of 0 or 1)
    assert not fv[:, 1:4].any()
    order = sorted(range(k.shape[0]), key=lambda i: (int(k[i]["saddr"]), int(k[i]["daddr"]),
                                                     int(k[i]["sport"]) | int(k[i]["dport"]) << 16, int(k[i]["proto"])))
    return k[order], v[order]


def run_golden(g, call):
    """The fixture's three batches through call(lb, umem, descs, ingress, nif) ->
    (umem after, verdicts); returns the LoadBalancer's final host/device dumps via `call`."""
    for b in range(3):
        umem = g[f"umem{b}"].copy()
        ingress, nif = (int(x) for x in g[f"params{b}"])
        after, verdicts = call(b, umem, g[f"descs{b}"], ingress, nif)
        bad = np.nonzero(verdicts != g[f"verdicts{b}"])[0]
        assert bad.size == 0, f"batch {b}: verdicts differ at {bad[:8]}: {verdicts[bad[:8]]} != {g[f'verdicts{b}'][bad[:8]]}"
        bad = np.nonzero(after != g[f"after{b}"])[0]
        assert bad.size == 0, f"batch {b}: {bad.size} UMEM bytes differ, first at {bad[:8]}"


def test_host_equals_the_reference_function(golden):
    """UMEM, verdicts and the final sessions, byte for byte."""
    g = golden
    with lb.LoadBalancer.from_backends(g["backends"], max_sessions=4096) as L:
        L.sessions_put(g["pre_keys"], g["pre_values"])
        stats = []

        def call(b, umem, descs, ingress, nif):
            v, st = lb.lb_host(umem, descs, L, ingress, nif)
            stats.append(st)
            return umem, v
        run_golden(g, call)
        k, v = L.sessions_dump()
        wk, wv = golden_dump(g)
        assert k.tobytes() == wk.tobytes() and v.tobytes() == wv.tobytes()
        assert L.info["host_sessions"] == wk.shape[0]
    assert all(int(st[0]) == g[f"descs{b}"].shape[0] for b, st in enumerate(stats))
    assert all(int(st[1] + st[2] + st[3]) == int(st[0]) for st in stats)
    assert int(stats[1][4]) > 100 and not any(int(st[5]) for st in stats)


def test_fixture_holds_what_it_should(golden):
    """Every branch, ihl 0..15 for both protocols among the rewritten frames, a
    UDP check of 0, ports whose promoted complement matters, nif 1."""
    g = golden
    seen, zero_udp, ports = set(), 0, set()
    for b in range(3):
        umem, after, descs = g[f"umem{b}"], g[f"after{b}"], g[f"descs{b}"]
        v = g[f"verdicts{b}"]
        assert (v == -1).any() and (v >= 0).any()
        for i in range(descs.shape[0]):
            addr, ln = int(descs[i]["addr"]), int(descs[i]["len"])
            off = (addr & ((1 << 48) - 1)) + (addr >> 48)
            if off + ln > umem.size or ln < 34:
                continue
            if not np.array_equal(umem[off:off + ln], after[off:off + ln]):
                f = umem[off:off + ln]
                ihl, proto = int(f[14]) & 15, int(f[23])
                seen.add((ihl, proto))
                nxt = 14 + 4 * ihl
                ports.update((int(f[nxt]) | int(f[nxt + 1]) << 8, int(f[nxt + 2]) | int(f[nxt + 3]) << 8))
                zero_udp += proto == 17 and ihl >= 5 and not f[nxt + 6] and not f[nxt + 7]
    assert seen == {(i, p) for i in range(16) for p in (6, 17)}
    assert zero_udp and {0x0000, 0xffff, 0x8000} <= ports
    assert int(golden["params2"][1]) == 1


def test_jhash_picks_the_fixtures_backends(golden):
    """The model's jhash and the library's agree with the reference's backend
    choices: every forward session the reference created names the backend
    that jhash(sid) % backends selects."""
    g = golden
    m = LC.Model(g["backends"], 1 << 20)
    pre = {LC.key_bytes(k) for k in g["pre_keys"]}
    checked = 0
    for kb, vb in zip(g["final_keys"], g["final_values"]):
        key = bytes(kb)
        if key in pre or int(vb[0]) != lb.TO_BACKEND:
            continue
        backs = m.services[key[4:8] + key[10:12] + key[12:13]]
        addr, port, mac, ifindex = backs[LC.jhash(key) % len(backs)]
        if len({b[:2] for b in backs}) > 1:
            checked += 1
        assert (addr, port) == (int.from_bytes(bytes(vb[4:8]), "little"), int.from_bytes(bytes(vb[8:10]), "little"))
        assert mac == bytes(vb[10:16]) and ifindex == int.from_bytes(bytes(vb[16:18]), "little")
    assert checked > 100
    # the kernel's published self-check values for jhash over bytes do not exist; pin two of ours
    assert LC.jhash(b"") == 0xdeadbeef and LC.jhash(bytes(13)) == LC.jhash(bytes(13), 0)


def test_host_equals_the_model_on_random_batches():
    rng = np.random.default_rng(31)
    bk = LC.make_backends(rng)
    for trial in range(3):
        fl = LC.flows_batch(rng, bk, flows=80, filler=40)
        sw, _ = LC.sweep_frames(rng, phases=(trial,))
        fl += sw
        umem, descs = LC.pack_packed(fl, rng)
        descs = FC.with_outside(umem, descs, rng)
        ks, vs = LC.sessions_for(fl, rng)
        with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L:
            L.sessions_put(ks, vs)
            m = LC.Model(bk, 4096)
            m.sessions_put(ks, vs)
            for b in range(2):   # the second batch finds the first's sessions
                u1, u2 = umem.copy(), umem.copy()
                v1, s1 = lb.lb_host(u1, descs, L, b, 3)
                v2, s2 = m.batch(u2, descs, b, 3)
                assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
                assert (int(s1[4]) > 0) == (b == 0)
            k1, w1 = L.sessions_dump()
            k2, w2 = m.dump()
            assert k1.tobytes() == k2.tobytes() and w1.tobytes() == w2.tobytes()


@pytest.mark.parametrize("which", ["existing_b", "shared_b", "vip_client"])
def test_ordered_causes_on_the_host(which):
    rng = np.random.default_rng(32)
    bk, (ks, vs), fl = LC.ordered_cause(rng, which)
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=64) as L:
        L.sessions_put(ks, vs)
        m = LC.Model(bk, 64)
        m.sessions_put(ks, vs)
        u1, u2 = umem.copy(), umem.copy()
        v1, s1 = lb.lb_host(u1, descs, L, 2, 4)
        v2, s2 = m.batch(u2, descs, 2, 4)
        assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
        assert L.sessions_dump()[1].tobytes() == m.dump()[1].tobytes()


def test_full_table_fails_inserts_in_the_loops_order():
    """max_sessions 8, 6 new flows (12 sessions): the first four flows fit, the
    fifth and sixth fail their forward insert and skip the backward one; every
    frame is still rewritten; a second batch fails again."""
    rng = np.random.default_rng(33)
    bk = LC.make_backends(rng, services=3)
    sids = [LC.service_sid(rng, bk) for _ in range(6)]
    fl = []
    for s in sids:
        fl += [LC.frame(rng, s), LC.frame(rng, LC.backward_sid(bk, s))]
    fl += [LC.frame(rng, s) for s in sids]
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=8) as L:
        m = LC.Model(bk, 8)
        for b in range(2):
            u1, u2 = umem.copy(), umem.copy()
            v1, s1 = lb.lb_host(u1, descs, L, 0, 2)
            v2, s2 = m.batch(u2, descs, 0, 2)
            assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
            # flows 5 and 6: two frames each fail their insert; their backward frames pass
            assert [int(x) for x in s1[:6]] == ([18, 16, 2, 0, 8, 4] if b == 0 else [18, 16, 2, 0, 0, 4])
        assert L.info["host_sessions"] == 8
        assert L.sessions_dump()[0].tobytes() == m.dump()[0].tobytes()
        # an odd capacity: the forward session fits, the backward one fails
    with lb.LoadBalancer.from_backends(bk, max_sessions=3) as L:
        m = LC.Model(bk, 3)
        u1, u2 = umem.copy(), umem.copy()
        v1, s1 = lb.lb_host(u1, descs, L, 0, 2)
        v2, s2 = m.batch(u2, descs, 0, 2)
        assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
        assert L.info["host_sessions"] == 3


def test_error_rules():
    rng = np.random.default_rng(34)
    lib = _lib.load()
    bk = LC.make_backends(rng, services=2)
    h = ctypes.c_void_p()
    E = errno
    assert lib.xsknf_gpu_lb_create(None, bk.ctypes.data, bk.size, 8, 0) == -E.EINVAL
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), None, 3, 8, 0) == -E.EINVAL
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), bk.ctypes.data, bk.size, lb.MAX_SESSIONS + 1, 0) == -E.EINVAL
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), bk.ctypes.data, bk.size, 8, 24) == -E.EINVAL      # no power of two
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), bk.ctypes.data, bk.size, 64, 64) == -E.EINVAL     # < 2 * max
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), bk.ctypes.data, bk.size, 8, lb.MAX_SLOTS * 2) == -E.EINVAL
    bad = bk.copy()
    bad["proto"][0] = 1
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), bad.ctypes.data, bad.size, 8, 0) == -E.EINVAL
    many = np.zeros(lb.MAX_SERVICES + 1, dtype=lb.BACKEND_DTYPE)
    many["vaddr"], many["proto"] = np.arange(many.size), 6
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), many.ctypes.data, many.size, 8, 0) == -E.EINVAL
    assert lib.xsknf_gpu_lb_create(ctypes.byref(h), many.ctypes.data, many.size - 1, 8, 0) == 0
    assert lib.xsknf_gpu_lb_destroy(h) == 0
    assert lib.xsknf_gpu_lb_destroy(None) == -E.EINVAL and lib.xsknf_gpu_lb_info(None, None) == -E.EINVAL
    w = ctypes.c_uint64(0)
    assert lib.xsknf_gpu_lb_workspace(lb.MAX_BATCH + 1, ctypes.byref(w)) == -E.EINVAL
    assert lib.xsknf_gpu_lb_workspace(5, None) == -E.EINVAL
    assert lb.lb_workspace(0) > 0 and lb.lb_workspace(1000) > lb.lb_workspace(10)
    with lb.LoadBalancer.from_backends(bk, max_sessions=2) as L:
        assert L.info["slots"] == 64 and L.info["services"] == 2 and L.info["backends"] == bk.size
        k, v = LC.session(1, 2, 3, 4, 6, lb.TO_BACKEND, 5, 6, [1, 2, 3, 4, 5, 6], 7)
        ks, vs = np.array([k] * 3, dtype=lb.KEY_DTYPE), np.array([v] * 3, dtype=lb.VALUE_DTYPE)
        ks["sport"] = [3, 4, 5]
        wrong = vs.copy()
        wrong["dir"][1] = 2
        assert lib.xsknf_gpu_lb_sessions_put(L.handle, ks.ctypes.data, wrong.ctypes.data, 3) == -E.EINVAL
        wrong = ks.copy()
        wrong["proto"][2] = 0
        assert lib.xsknf_gpu_lb_sessions_put(L.handle, wrong.ctypes.data, vs.ctypes.data, 3) == -E.EINVAL
        assert lib.xsknf_gpu_lb_sessions_put(L.handle, None, vs.ctypes.data, 3) == -E.EINVAL
        assert L.info["host_sessions"] == 0                      # nothing was stored by the refused calls
        assert lib.xsknf_gpu_lb_sessions_put(L.handle, ks.ctypes.data, vs.ctypes.data, 3) == -E.ENOSPC
        assert L.info["host_sessions"] == 2
        L.sessions_put(ks[:2], vs[:2])                           # replacing needs no room
        n = ctypes.c_uint32(0)
        assert lib.xsknf_gpu_lb_sessions_dump(L.handle, 0, ks.ctypes.data, vs.ctypes.data, 1, ctypes.byref(n)) == -E.ENOSPC
        assert n.value == 2
        assert lib.xsknf_gpu_lb_sessions_dump(L.handle, 7, ks.ctypes.data, vs.ctypes.data, 3, ctypes.byref(n)) == -E.EINVAL
        assert lib.xsknf_gpu_lb_host(None, 0, None, 4, 0, 1, L.handle, None, None) == -E.EINVAL
        assert lib.xsknf_gpu_lb_host(None, 0, None, 0, 0, 1, None, None, None) == -E.EINVAL
        st = (ctypes.c_uint64 * 8)()
        assert lib.xsknf_gpu_lb_batch(None, 0, None, 0, 0, 1, None, None, None, 0, st, None) == -E.EINVAL
        assert lib.xsknf_gpu_lb_batch(None, 0, None, 0, 0, 1, L.handle, None, None, 0, None, None) == -E.EINVAL
        assert lib.xsknf_gpu_lb_batch(8, 0, None, 0, 0, 1, L.handle, None, None, 0, st, None) == -E.EINVAL   # misaligned
        assert lib.xsknf_gpu_lb_batch(None, 0, None, 4, 0, 1, L.handle, None, None, 0, st, None) == -E.EINVAL
        assert lib.xsknf_gpu_lb_batch(None, 0, None, 0, 0, 1, L.handle, None, None, 0, st, None) == 0


def test_device_calls_without_a_device_return_enodev():
    """In a process that sees no device the object is host-only."""
    import subprocess
    import sys
    code = ("import sys, errno, ctypes; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from xsknf_amd import _lib, lb\n"
            "L = lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=4)\n"
            "assert L.info['device_bytes'] == 0\n"
            "buf = (ctypes.c_uint8 * 4096)(); a = (ctypes.addressof(buf) + 15) & ~15\n"
            "rc = _lib.load().xsknf_gpu_lb_batch(a, 64, a + 1024, 1, 0, 1, L.handle, a + 2048, a + 2064, 1024, a + 3584, None)\n"
            "n = ctypes.c_uint32(0)\n"
            "rd = _lib.load().xsknf_gpu_lb_sessions_dump(L.handle, 1, None, None, 0, ctypes.byref(n))\n"
            "print(rc == -errno.ENODEV, rd == -errno.ENODEV)\n") % FC.ROOT
    import os
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.split() == ["True", "True"], out.stdout
