"""xsknf_gpu_acl_update on the device (include/xsknf_gpu.h; xsknf_amd/csrc/
acl_update_device.hip, kernel_acl_update.h): after every call the device table's
dump equals the host table's and xsknf_gpu_firewall_batch answers as
xsknf_gpu_firewall_host does (tests/test_acl_update.py holds the host table to
the dict model); the update takes its place in the stream's order with no wait;
record counts around the wave, the block's tile and the grid's sweep, read from
the code."""
import errno
import re

import numpy as np
import pytest

from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from tests import test_gpu_lbfw as GL
from xsknf_amd import _lib, firewall, lb
from xsknf_amd.firewall import Acl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = UC.all_cases()
T = FC.code_constant(r"constexpr int kThreads = (\d+);", "kernel_acl_update.h")        # records per block and step
G = T * FC.code_constant(r"constexpr int kMaxBlocks = (\d+);", "kernel_acl_update.h")  # records per sweep of the largest grid
COUNTS = [1, 63, 64, 65, T - 1, T, T + 1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def _batch(dev, du, size, dd, n, acl, stream=None):
    """Enqueue one xsknf_gpu_firewall_batch; returns the verdict tensor."""
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(s):   # (the sentinel fill on the batch's stream)
        dv = torch.full((n,), 0x5eadbeef, dtype=torch.int32, device=dev)
        firewall.firewall_batch_ptr(du.data_ptr(), size, dd.data_ptr(), n, acl, dv.data_ptr(), s.cuda_stream)
    return dv


def _same_tables(acl, what=""):
    h, d = acl.dump(), acl.dump(device=True)
    assert h.shape == d.shape and h.tobytes() == d.tobytes(), f"{what}: the device table is not the host table"
    return h


def test_sizes_are_read_from_the_code():
    src = open(FC.ROOT + "/xsknf_amd/csrc/kernel_acl_update.h").read()
    assert re.search(r"__launch_bounds__\(kThreads\)", src) and re.search(r"stride = gridDim\.x \* kThreads", src)
    assert re.search(r"if \(slot < a\.slots\)", src)
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/acl_update_device.hip").read()
    assert re.search(r"tiles < static_cast<uint32_t>\(acl_update::kMaxBlocks\) \? tiles : acl_update::kMaxBlocks", dsrc)
    assert T % 64 == 0 and G > T


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_table_follows_the_host_table(dev, case):
    umem, descs, keys = UC.probe_frames(case)
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    lib = _lib.load()
    with torch.cuda.device(dev), Acl.from_rules(case.rules, case.slots) as A:
        assert A.info["device_bytes"] == 20 * case.slots
        for i, (call, want) in enumerate(zip(case.calls, case.expected)):
            if isinstance(call, tuple):
                before = A.dump(device=True)
                ops, err = call
                rc = lib.xsknf_gpu_acl_update(A.handle, ops.ctypes.data, ops.size, None)
                assert rc == -err
                assert A.dump(device=True).tobytes() == before.tobytes(), f"call {i}: a refused call reached the device"
            else:
                A.update(ops=call)
            h = _same_tables(A, f"{case.name}, call {i}")
            assert h.tobytes() == UC.sorted_rules(want).tobytes()
            got = _batch(dev, du, umem.size, dd, descs.shape[0], A).cpu().numpy()
            assert np.array_equal(got, firewall.firewall_host(umem, descs, A)), f"{case.name}, call {i}: lookups differ"
            if UC.must_rebuild(case, i):
                assert A.info["tombstones"] == 0


def test_update_takes_its_place_in_the_stream(dev):
    """batch -> update -> batch on one non-default stream, one synchronize after
    all three: the first batch answers by the old rules, the second by the new.
    512 frames: keys kept, replaced, deleted, put, and never held."""
    rng = np.random.default_rng(4201)
    rules = FC.random_rules(rng, 512)
    assert len(FC.acl_dict(rules)) == 512
    rules["action"] = rng.integers(1, 30, 512)
    kept, replaced, deleted, new, never = (rules[i::5] for i in range(5))
    start = np.concatenate([kept, replaced, deleted])
    changed = replaced.copy()
    changed["action"] = -1
    umem, descs = FC.frames_for_rules(rules, rng)
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    with torch.cuda.device(dev), Acl.from_rules(start, 1024) as A:
        torch.cuda.synchronize(dev)
        old = firewall.firewall_host(umem, descs, A)
        s = torch.cuda.Stream(dev)
        assert s.cuda_stream != 0
        va = _batch(dev, du, umem.size, dd, 512, A, s)
        A.update(puts=np.concatenate([changed, new]), deletes=deleted, stream=s)
        vb = _batch(dev, du, umem.size, dd, 512, A, s)
        s.synchronize()
        fresh = firewall.firewall_host(umem, descs, A)
        assert np.array_equal(va.cpu().numpy(), old) and np.array_equal(vb.cpu().numpy(), fresh)
        d_old, d_new = FC.acl_dict(start), UC.apply(FC.acl_dict(start), np.concatenate(
            [firewall.make_ops(deleted, firewall.DELETE), firewall.make_ops(np.concatenate([changed, new]), firewall.PUT)]))
        assert np.array_equal(old, FC.model(umem, descs, d_old)) and np.array_equal(fresh, FC.model(umem, descs, d_new))
        assert (old != fresh).sum() == len(replaced) + len(deleted) + len(new)
        _same_tables(A)


def test_two_updates_back_to_back(dev):
    """Two updates on one stream with no wait between them, the second on slots
    the first dirtied (replaces, deletes of the first's puts, puts into the
    first's tombstones): neither overwrites the other's records."""
    rng = np.random.default_rng(4202)
    rules = FC.random_rules(rng, 600)
    first_new, second_new = FC.random_rules(rng, 300), FC.random_rules(rng, 300)
    with torch.cuda.device(dev), Acl.from_rules(rules, 2048) as A:
        s = torch.cuda.Stream(dev)
        again = first_new[:150].copy()
        again["action"] = 77
        A.update(puts=first_new, deletes=rules[:200], stream=s)
        A.update(puts=np.concatenate([again, second_new, rules[:50]]), deletes=first_new[150:], stream=s)
        s.synchronize()
        h = _same_tables(A)
        want = UC.apply(UC.apply(FC.acl_dict(rules), np.concatenate(
            [firewall.make_ops(rules[:200], firewall.DELETE), firewall.make_ops(first_new, firewall.PUT)])),
            np.concatenate([firewall.make_ops(first_new[150:], firewall.DELETE),
                            firewall.make_ops(np.concatenate([again, second_new, rules[:50]]), firewall.PUT)]))
        assert h.tobytes() == UC.sorted_rules(want).tobytes()
        # a third, once the stream has passed the first two: their buffers are free again
        A.update(deletes=second_new, stream=s)
        s.synchronize()
        assert _same_tables(A).shape[0] == len(want) - len(FC.acl_dict(second_new))


def test_record_counts_around_the_kernels_edges(dev):
    """Updates of n distinct new keys dirty exactly n slots: n around the wave
    and the block's tile, one after the other on one table."""
    total = 0
    with torch.cuda.device(dev), Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE), 4096) as A:
        for n in COUNTS:
            A.update(puts=UC.distinct_new_rules(n, base=total))
            total += n
            h = _same_tables(A, f"{n} records")
            assert h.shape[0] == total == A.info["rules"] and A.info["tombstones"] == 0
        assert FC.acl_dict(h) == FC.rules_dict_fast(UC.distinct_new_rules(total))


def test_one_record_past_the_largest_grids_sweep(dev):
    """kMaxBlocks x kThreads + 1 distinct new keys into 2^21 slots: the last
    record is the only one of the grid's second sweep."""
    r = UC.distinct_new_rules(G + 1)
    with torch.cuda.device(dev), Acl.from_rules(np.zeros(0, dtype=firewall.RULE_DTYPE), 1 << 21) as A:
        A.update(puts=r)
        h = _same_tables(A)
        assert h.shape[0] == G + 1
        order = np.argsort(r["saddr"], kind="stable")   # distinct saddr: the dump's order
        assert h.tobytes() == r[order].tobytes()


def test_forced_rebuild_sends_the_whole_table(dev):
    rng = np.random.default_rng(4203)
    keys = UC.keys_away(rng, 50, ())
    rules = FC.rules_from_keys(keys, range(50))
    gone = rules[:UC.SLOTS // UC.tombstone_share() + 1]
    umem, descs = FC.frames_for_rules(rules, rng)
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    with torch.cuda.device(dev), Acl.from_rules(rules, UC.SLOTS) as A:
        A.update(deletes=gone[:5])
        assert A.info["tombstones"] == 5
        _same_tables(A)
        A.update(deletes=gone[5:], puts=rules[:2])
        assert A.info["tombstones"] == 0 and A.info["rules"] == 50 - len(gone) + 2
        _same_tables(A)
        got = _batch(dev, du, umem.size, dd, 50, A).cpu().numpy()
        assert np.array_equal(got, firewall.firewall_host(umem, descs, A))
        assert (got[2:len(gone)] == 0).all() and np.array_equal(got[len(gone):], np.arange(len(gone), 50))


def test_lbfw_on_the_device_after_an_update(dev):
    """After a delete the rule's frames reach the load balancer; a rule put with
    action 0 decides its frames: xsknf_gpu_lbfw_batch against xsknf_gpu_lbfw_host,
    sessions included."""
    rng = np.random.default_rng(4204)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=80, filler=40)
    umem, descs = LC.pack_packed(fl, rng)
    keys = WC.frame_keys(fl)
    held, free = keys[::3], keys[1::3]
    r, _ = WC.rules(held, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(held))])
    with torch.cuda.device(dev), lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
        _, _, s0 = GL.check_batch(dev, A, L, umem, descs, 0, 3, "before")
        A.update(ops=UC.ops_of(UC.deletes(held[::2])))
        _, _, s1 = GL.check_batch(dev, A, L, umem, descs, 0, 3, "after the delete")
        assert int(s1[WC.GATED]) < int(s0[WC.GATED]) and int(s1[4]) > 0
        A.update(ops=UC.ops_of(UC.puts(free[::2], [0] * len(free[::2]))))
        _, v2, s2 = GL.check_batch(dev, A, L, umem, descs, 0, 3, "after the put")
        assert int(s2[WC.GATED]) > int(s1[WC.GATED])
        _same_tables(A)


def test_refused_and_empty_updates_leave_the_device_alone(dev):
    rng = np.random.default_rng(4205)
    rules = FC.rules_from_keys(UC.keys_away(rng, UC.SLOTS - 1, ()), range(UC.SLOTS - 1))
    more = firewall.make_ops(FC.random_rules(rng, 2), firewall.PUT)
    lib = _lib.load()
    with torch.cuda.device(dev), Acl.from_rules(rules, UC.SLOTS) as A:
        before = A.dump(device=True)
        s = torch.cuda.current_stream(dev).cuda_stream
        assert lib.xsknf_gpu_acl_update(A.handle, more.ctypes.data, 2, s) == -errno.ENOSPC
        bad = more.copy()
        bad["op"][1] = 2
        assert lib.xsknf_gpu_acl_update(A.handle, bad.ctypes.data, 2, s) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_update(A.handle, None, 2, s) == -errno.EINVAL
        assert lib.xsknf_gpu_acl_update(A.handle, None, 0, s) == 0           # n == 0
        assert lib.xsknf_gpu_acl_update(A.handle, more.ctypes.data, 0, s) == 0
        A.update()
        assert A.dump(device=True).tobytes() == before.tobytes() == A.dump().tobytes()
        assert A.info["rules"] == UC.SLOTS - 1 and A.info["tombstones"] == 0
