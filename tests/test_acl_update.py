"""xsknf_gpu_acl_update on the host table (include/xsknf_gpu.h; xsknf_amd/csrc/acl.cpp):
after every call of every case of tests/acl_update_cases.py the dump equals the
dict model and xsknf_gpu_firewall_host answers as the dict does for every key
the case names and for one-bit near misses; the lbfw gate follows; two objects
given the same calls are equal; 20,000 random ops.  No GPU: in a process without
a device the call updates the host table alone."""
import ctypes
import errno

import numpy as np
import pytest

from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from xsknf_amd import ACL_DELETE, ACL_PUT, _lib, firewall, lb, lbfw
from xsknf_amd.firewall import Acl

CASES = UC.all_cases()


def _refused(acl, ops, err):
    rc = _lib.load().xsknf_gpu_acl_update(acl.handle, ops.ctypes.data if ops.size else None, ops.size, None)
    assert rc == -err, (rc, err)


def test_the_cases_hold_what_they_should():
    names = " / ".join(c.name for c in CASES)
    for word in ("middle of a chain", "re-put", "tombstone in front", "wraps", "slots - 1", "tombstone bound", "last op"):
        assert word in names
    assert ACL_PUT == firewall.PUT == 0 and ACL_DELETE == firewall.DELETE == 1
    assert firewall.OP_DTYPE.itemsize == 24 and firewall.OP_DTYPE.fields["op"][1] == 20
    # the chains collide where the hash restated in the case file says
    chain = CASES[3]
    homes = [UC.home(FC.rule_key(r)) for r in chain.rules[:5]]
    assert homes == [62] * 5
    big = next(c for c in CASES if "tombstone bound" in c.name)
    assert sum(UC.must_rebuild(big, i) for i in range(len(big.calls))) >= 2
    full = next(c for c in CASES if "slots - 1" in c.name)
    assert len(FC.acl_dict(full.rules)) == full.slots - 1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_table_follows_the_dict(case):
    umem, descs, keys = UC.probe_frames(case)
    share = UC.tombstone_share()
    rebuilds = 0
    with Acl.from_rules(case.rules, case.slots) as A, Acl.from_rules(case.rules, case.slots) as B:
        assert A.info["tombstones"] == 0
        assert A.dump().tobytes() == UC.sorted_rules(FC.acl_dict(case.rules)).tobytes()
        for i, (call, want) in enumerate(zip(case.calls, case.expected)):
            before, info0 = A.dump(), A.info
            if isinstance(call, tuple):
                _refused(A, *call)
                _refused(B, *call)
                assert A.dump().tobytes() == before.tobytes() and A.info == info0, f"call {i}: a refused call left a trace"
            else:
                A.update(ops=call)
                B.update(ops=call)
            got = A.dump()
            assert got.tobytes() == UC.sorted_rules(want).tobytes(), f"call {i}: the dump is not the dict"
            assert not got["pad"].any()
            v = firewall.firewall_host(umem, descs, A)
            assert np.array_equal(v, UC.verdicts_of(want, keys)), f"call {i}: lookups differ from the dict"
            info = A.info
            assert info["rules"] == len(want) and info["slots"] == case.slots
            assert info["tombstones"] <= case.slots // share and info["rules"] + info["tombstones"] < case.slots
            if UC.must_rebuild(case, i):
                assert info["tombstones"] == 0, f"call {i}: no rebuild"
                rebuilds += 1
            # determinism: the same calls, the same table
            assert B.dump().tobytes() == got.tobytes() and B.info == info
        if "tombstone bound" in case.name:
            assert rebuilds >= 2
        if "five at a time" in case.name:
            assert A.info["tombstones"] < 5 * 23   # they do not pile up: some call rebuilt


def test_max_probe_is_the_worst_live_key():
    """Five keys that start in one slot: max_probe 5; without the last 4; without
    the first still 4 (the others stay where they are); after the rebuild that
    many deletes force, the keys left move up."""
    rng = np.random.default_rng(4106)
    c = UC.keys_at(rng, 7, 5)
    rest = [UC.keys_at(rng, 24 + 2 * i, 1)[0] for i in range(14)]   # each alone in its slot
    with Acl.from_rules(FC.rules_from_keys(c + rest, [1] * (5 + len(rest))), 64) as A:
        lone = A.info["max_probe"]
        assert lone == 5
        A.update(deletes=FC.rules_from_keys([c[4]], [0]))
        assert A.info["max_probe"] == 4
        A.update(deletes=FC.rules_from_keys([c[0]], [0]))
        assert A.info["max_probe"] == 4 and A.info["tombstones"] == 2
        A.update(puts=FC.rules_from_keys([c[4]], [3]))          # into c[0]'s slot: the first probe
        assert A.info["max_probe"] == 4 and A.info["tombstones"] == 1
        A.update(deletes=FC.rules_from_keys(c[1:4] + rest, [0] * (3 + len(rest))))
        assert A.info == dict(A.info, rules=1, max_probe=1, tombstones=0)
        A.update(deletes=FC.rules_from_keys([c[4]], [0]))
        assert A.info["rules"] == 0 and A.info["max_probe"] == 0


def test_puts_and_deletes_arguments():
    """deletes apply before puts; ops excludes both; n == 0 in every form."""
    rng = np.random.default_rng(4107)
    k = UC.keys_away(rng, 4, ())
    with Acl.from_rules(FC.rules_from_keys(k[:2], [1, 2]), 64) as A:
        A.update(puts=FC.rules_from_keys([k[0], k[2]], [5, 6]), deletes=FC.rules_from_keys([k[0], k[1]], [0, 0]))
        assert FC.acl_dict(A.dump()) == {k[0]: 5, k[2]: 6}
        for kw in ({}, {"puts": FC.rules_from_keys([], [])}, {"ops": np.zeros(0, dtype=firewall.OP_DTYPE)}):
            A.update(**kw)
        assert FC.acl_dict(A.dump()) == {k[0]: 5, k[2]: 6}
        with pytest.raises(ValueError):
            A.update(puts=FC.rules_from_keys([k[3]], [1]), ops=np.zeros(0, dtype=firewall.OP_DTYPE))
        with pytest.raises(ValueError):
            A.update(ops=np.zeros(3, dtype=np.uint8))
        with pytest.raises(_lib.XsknfGpuError, match="rc=-22"):
            bad = firewall.make_ops(FC.rules_from_keys([k[3]], [1]), firewall.PUT)
            bad["op"] = 7
            A.update(ops=bad)


def test_c_abi_validation():
    lib = _lib.load()
    with Acl.from_rules(FC.random_rules(np.random.default_rng(1), 10), 64) as A:
        ops = firewall.make_ops(FC.random_rules(np.random.default_rng(2), 3), firewall.PUT)
        n = ctypes.c_uint32(77)
        assert lib.xsknf_gpu_acl_update(None, ops.ctypes.data, 3, None) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_update(A.handle, None, 3, None) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_update(A.handle, None, 0, None) == 0
        one = np.zeros(1, dtype=firewall.RULE_DTYPE)
        assert lib.xsknf_gpu_acl_dump(None, 0, one.ctypes.data, 1, ctypes.byref(n)) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_dump(A.handle, 0, one.ctypes.data, 1, None) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_dump(A.handle, 0, None, 1, ctypes.byref(n)) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_dump(A.handle, 2, one.ctypes.data, 1, ctypes.byref(n)) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_dump(A.handle, 0, one.ctypes.data, 1, ctypes.byref(n)) == -errno.ENOSPC and n.value == 10
        assert one.tobytes() == A.dump()[:1].tobytes()
        if not A.info["device_bytes"]:
            assert lib.xsknf_gpu_acl_dump(A.handle, 1, None, 0, ctypes.byref(n)) == -errno.ENODEV


def test_max_rules_bounds_the_map():
    """XSKNF_GPU_ACL_MAX_RULES rules in 2^21 slots: one more new key is -ENOSPC,
    a replace and a swap are not."""
    r = UC.distinct_new_rules(firewall.MAX_RULES + 2)
    with Acl.from_rules(r[:firewall.MAX_RULES], 1 << 21) as A:
        _refused(A, firewall.make_ops(r[-1:], firewall.PUT), errno.ENOSPC)
        A.update(puts=r[:1])
        A.update(deletes=r[1:2], puts=r[-2:-1])
        assert A.info["rules"] == firewall.MAX_RULES and A.info["tombstones"] <= 1


def test_lbfw_host_sees_the_update_at_once():
    """A deleted rule's frames fall through to the load balancer; a rule put
    with action 0 is a hit: xsknf_gpu_lbfw_host against the model with the dict
    the update leaves."""
    rng = np.random.default_rng(4108)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=80, filler=40)
    umem, descs = LC.pack_packed(fl, rng)
    keys = WC.frame_keys(fl)
    held, free = keys[::3], keys[1::3]
    r, d = WC.rules(held, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(held))])
    gone, zero = held[::2], free[::2]
    ops = UC.ops_of(UC.deletes(gone) + UC.puts(zero, [0] * len(zero)))
    d2 = UC.apply(d, ops)
    assert len(gone) > 10 and len(zero) > 10 and set(d2.values()) >= {0, -1}
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
        m = WC.Model(bk, 4096)
        for acl_dict in (d, d2):
            u1, u2 = umem.copy(), umem.copy()
            v1, s1 = lbfw.lbfw_host(u1, descs, A, L, 0, 3)
            v2, s2 = m.batch(u2, descs, 0, 3, acl_dict)
            assert np.array_equal(v1, v2) and np.array_equal(u1, u2) and np.array_equal(s1, s2)
            A.update(ops=ops)
        # the second batch: frames of `gone` made sessions, frames of `zero` were decided
        assert int(s1[WC.GATED]) > 0 and int(s1[4]) > 0
        k1, w1 = L.sessions_dump()
        k2, w2 = m.dump()
        assert k1.tobytes() == k2.tobytes() and w1.tobytes() == w2.tobytes()


def test_random_ops_against_the_dict():
    """20,000 seeded ops over 200 keys in 256 slots, in calls of 0 to 160 ops."""
    total = 0
    with Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE), 256) as A:
        for ops, want in UC.random_calls():
            A.update(ops=ops)
            total += ops.size
            assert A.dump().tobytes() == UC.sorted_rules(want).tobytes(), f"after {total} ops"
            info = A.info
            assert info["rules"] == len(want) and info["tombstones"] <= 256 // UC.tombstone_share()
        # every key of the universe, live or not, through the lookup
        rng = np.random.default_rng(4105)
        universe = [UC.random_key(rng) for _ in range(200)]
        umem, descs = FC.frames_for_rules(FC.rules_from_keys(universe, [0] * 200), rng)
        assert np.array_equal(firewall.firewall_host(umem, descs, A), UC.verdicts_of(want, universe))
    assert total == 20000 and 0 < len(want) < 200
