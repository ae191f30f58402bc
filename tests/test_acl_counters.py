"""The ACL's hit counters on the host (include/xsknf_gpu.h
xsknf_gpu_acl_counters_*; xsknf_amd/csrc/acl.cpp, firewall_host.cpp,
lbfw_host.cpp): the host set against the plain-Python model of
tests/acl_counter_cases.py.  All results are exact integers."""
import ctypes
import errno

import numpy as np
import pytest

from tests import acl_counter_cases as CC
from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from xsknf_amd import _lib, firewall, lb, lbfw
from xsknf_amd.firewall import Acl

CASES = CC.update_cases()


def _acl(rules, slots=0):
    return Acl.from_rules(rules, slots)


def _setup(seed, n=40):
    rng = np.random.default_rng(seed)
    keys = UC.keys_away(rng, n, ())
    rules = FC.rules_from_keys(keys, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(n)])
    return rng, keys, rules


def test_batches_accumulate_and_the_totals_add_up():
    """Skewed hits, misses, every branch of the parse and descriptors outside the
    UMEM, three calls: the verdicts are the firewall's and the counts add up."""
    rng, keys, rules = _setup(5001)
    m = CC.Model(rules)
    dec, ph = FC.decision_frames(rng, phases=(0, 7))
    du, dd = FC.pack_unaligned(dec[::5], rng, ph[::5], tail=3)
    dd = FC.with_outside(du, dd, rng)
    with _acl(rules) as A:
        A.counters_enable()
        A.counters_enable()   # idempotent
        CC.check(A, m, what="fresh")
        for i in range(3):
            umem, descs = CC.frames_for_keys(CC.traffic(rng, keys, 300), rng)
            for u, d in ((umem, descs), (du, dd)):
                assert np.array_equal(firewall.firewall_host(u, d, A), m.batch(u, d))
            _, ctr, totals = CC.check(A, m, what=f"call {i}")
        assert int(totals[CC.HITS]) == int(ctr["packets"].sum()) and min(totals.tolist()) > 0
        assert int(ctr["packets"].max()) > 100 and int(ctr["bytes"].sum()) >= 54 * int(totals[CC.HITS])


def test_clear_zeroes_one_set():
    rng, keys, rules = _setup(5002)
    m = CC.Model(rules)
    umem, descs = CC.frames_for_keys(CC.traffic(rng, keys, 200), rng)
    with _acl(rules) as A:
        A.counters_enable()
        firewall.firewall_host(umem, descs, A)
        m.batch(umem, descs)
        CC.check(A, m)
        A.counters_clear()
        m.clear()
        _, ctr, totals = CC.check(A, m, what="cleared")
        assert not ctr["packets"].any() and not ctr["bytes"].any() and not totals.any()
        firewall.firewall_host(umem, descs, A)
        m.batch(umem, descs)
        CC.check(A, m, what="counting again")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_updates_keep_end_and_start_counters(case):
    CC.run_steps(case, _acl, lambda A, u, d: firewall.firewall_host(u, d, A), lambda A, ops: A.update(ops=ops),
                 lambda A, m, i: CC.check(A, m, what=f"{case[0]}, step {i}"))


def test_lbfw_host_counts_gated_frames_as_hits():
    rng = np.random.default_rng(5003)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=80, filler=40)
    umem, descs = LC.pack_packed(fl, rng)
    descs = FC.with_outside(umem, descs, rng)
    keys = WC.frame_keys(fl)
    r, d = WC.rules(keys[::3], [(0, -1, 2)[i % 3] for i in range(len(keys[::3]))])
    m = CC.Model(r)
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, _acl(r) as A:
        A.counters_enable()
        for i in range(2):
            hu = umem.copy()
            m.batch(hu, descs)   # (before the rewrite: the model reads the frames as they came)
            hv, hs = lbfw.lbfw_host(hu, descs, A, L, 0, 3)
            _, ctr, totals = CC.check(A, m, what=f"lbfw batch {i}")
            assert int(totals[CC.HITS]) == (i + 1) * int(hs[WC.GATED]) > 0
        assert int(totals[CC.MISSES]) > 0 and int(totals[CC.DECIDED]) > 0
        # the ACL's other NF goes on counting into the same set
        firewall.firewall_host(umem, descs, A)
        m.batch(umem, descs)
        CC.check(A, m, what="then the firewall")


def test_errors_before_any_work():
    rng, keys, rules = _setup(5004, n=10)
    lib = _lib.load()
    E = errno
    out = np.zeros(10, dtype=firewall.RULE_DTYPE)
    ctr = np.zeros(10, dtype=firewall.COUNTER_DTYPE)
    n = ctypes.c_uint32(99)
    dump, clear = lib.xsknf_gpu_acl_counters_dump, lib.xsknf_gpu_acl_counters_clear
    assert lib.xsknf_gpu_acl_counters_enable(None) == -E.EINVAL
    assert dump(None, 0, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.EINVAL
    assert clear(None, 0, None) == -E.EINVAL
    with _acl(rules) as A:
        h = A.handle
        # an object without counters
        assert dump(h, 0, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.EINVAL
        assert clear(h, 0, None) == -E.EINVAL
        with pytest.raises(_lib.XsknfGpuError):
            A.counters()
        A.counters_enable()
        assert dump(h, 2, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.EINVAL
        assert dump(h, -1, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.EINVAL
        assert dump(h, 0, out.ctypes.data, ctr.ctypes.data, 10, None, None) == -E.EINVAL
        assert dump(h, 0, None, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.EINVAL
        assert dump(h, 0, out.ctypes.data, None, 10, ctypes.byref(n), None) == -E.EINVAL
        assert clear(h, 2, None) == -E.EINVAL
        assert n.value == 99
        # cap: the count is told, at most cap entries are written
        tot = np.zeros(4, dtype=np.uint64)
        assert dump(h, 0, None, None, 0, ctypes.byref(n), tot.ctypes.data) == -E.ENOSPC and n.value == 10
        out["action"] = 1234
        assert dump(h, 0, out.ctypes.data, ctr.ctypes.data, 9, ctypes.byref(n), None) == -E.ENOSPC and n.value == 10
        assert int(out["action"][9]) == 1234
        assert dump(h, 0, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == 0
        assert out.tobytes() == A.dump().tobytes()
        if A.info["device_bytes"] == 0:   # a host-only object: no device set
            assert dump(h, 1, out.ctypes.data, ctr.ctypes.data, 10, ctypes.byref(n), None) == -E.ENODEV
            assert clear(h, 1, None) == -E.ENODEV


def test_an_acl_without_counters_is_what_it_was():
    rng, keys, rules = _setup(5005)
    umem, descs = CC.frames_for_keys(CC.traffic(rng, keys, 200), rng)
    ops = UC.ops_of(UC.deletes(keys[:20]) + UC.puts(CC.absent_keys(rng, 5, keys), [1] * 5))
    with _acl(rules, 64) as A, _acl(rules, 64) as B:
        B.counters_enable()
        assert {k: v for k, v in A.info.items() if k != "device_bytes"} == \
            {k: v for k, v in B.info.items() if k != "device_bytes"}
        if A.info["device_bytes"]:
            assert A.info["device_bytes"] == 20 * 64 and B.info["device_bytes"] == 20 * 64 + 16 * 64 + 32
        for step in range(2):
            assert np.array_equal(firewall.firewall_host(umem, descs, A), firewall.firewall_host(umem, descs, B))
            assert A.dump().tobytes() == B.dump().tobytes()
            A.update(ops=ops)   # (a rebuild: 20 deletes in 64 slots)
            B.update(ops=ops)
        assert A.info["tombstones"] == B.info["tombstones"] == 0 and A.info["rules"] == B.info["rules"] == 25
        n = ctypes.c_uint32(0)
        assert _lib.load().xsknf_gpu_acl_counters_dump(A.handle, 0, None, None, 0, ctypes.byref(n), None) == -errno.EINVAL
