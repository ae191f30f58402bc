"""Ageing of the load balancer's HOST session table (include/xsknf_gpu.h
xsknf_gpu_lb_aging_enable, _clock, _sessions_expire_host, _sessions_ages;
xsknf_amd/csrc/lb.cpp, lb_table.h rule 11) against the model of
tests/lb_age_cases.py: after every step the ages dump, the result words and the
count equal the model, and every batch of xsknf_gpu_lb_host / _lbfw_host equals
the model's in verdicts, counters and frames.  tests/test_gpu_lb_age.py holds
the device table to the same cases."""
import ctypes
import errno

import numpy as np
import pytest

from tests import lb_age_cases as AC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from xsknf_amd import _lib, lb
from xsknf_amd.firewall import Acl

H, D = lb.HOST_TABLE, lb.DEVICE_TABLE


def make(bk, max_sessions, slots, enable=True):
    return AC.Rig(bk, max_sessions, slots, None, enable)


def test_enable_on_a_filled_table():
    AC.case_enable_on_a_filled_table(make)


def test_hits_stamp_the_session_they_use():
    AC.case_hits(make)


def test_new_flows_and_a_replaced_backward_session():
    AC.case_new_flows(make)


def test_a_full_table_has_room_after_expire():
    AC.case_full_table(make)


def test_the_pair_rule():
    AC.case_pair_rule(make)


def test_bounds_of_max_idle_and_a_wrapped_clock():
    AC.case_bounds(make)


@pytest.mark.parametrize("trigger", ["expire", "remove", "drain"])
def test_a_rebuild_carries_the_stamps(trigger):
    AC.case_rebuild(make, trigger)


def test_lbfw_gated_frames_stamp_nothing():
    AC.case_lbfw(make, Acl.from_rules)


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_a_mixed_run(seed):
    AC.case_mixed_run(make, seed)


def test_errors():
    """Before enable every call is -EINVAL; then a bad which, a NULL lb and a
    misaligned result_dev are; the device forms of a host-only object are -ENODEV."""
    lib = _lib.load()
    E, N = -errno.EINVAL, -errno.ENODEV
    bk = CC.one_backend(17)
    res = np.full(4, 99, dtype=np.uint64)
    k, a = np.zeros(4, dtype=lb.KEY_DTYPE), np.zeros(4, dtype=np.uint32)
    n, c = ctypes.c_uint32(7), ctypes.c_uint32(7)
    with lb.LoadBalancer.from_backends(bk, max_sessions=8, slots=64) as L:
        h = L.handle

        def calls(rd):
            return [lib.xsknf_gpu_lb_clock(h, H, 1, None), lib.xsknf_gpu_lb_clock(h, D, 1, None),
                    lib.xsknf_gpu_lb_sessions_expire_host(h, 0, res.ctypes.data),
                    lib.xsknf_gpu_lb_sessions_expire(h, 0, rd, None),
                    lib.xsknf_gpu_lb_sessions_ages(h, H, k.ctypes.data, a.ctypes.data, 4, ctypes.byref(n), ctypes.byref(c)),
                    lib.xsknf_gpu_lb_sessions_ages(h, D, k.ctypes.data, a.ctypes.data, 4, ctypes.byref(n), ctypes.byref(c))]

        assert calls(None) == [E] * 6
        assert (res == 99).all() and n.value == 7 and c.value == 7
        assert lib.xsknf_gpu_lb_aging_enable(None) == E
        L.aging_enable()
        for which in (-1, 2):
            assert lib.xsknf_gpu_lb_clock(h, which, 1, None) == E
            assert lib.xsknf_gpu_lb_sessions_ages(h, which, k.ctypes.data, a.ctypes.data, 4, ctypes.byref(n), None) == E
        assert lib.xsknf_gpu_lb_clock(None, H, 1, None) == E
        assert lib.xsknf_gpu_lb_sessions_expire_host(None, 0, None) == E
        assert lib.xsknf_gpu_lb_sessions_expire(None, 0, None, None) == E
        assert lib.xsknf_gpu_lb_sessions_expire(h, 0, ctypes.c_void_p(res.ctypes.data + 4), None) == E
        assert lib.xsknf_gpu_lb_sessions_ages(None, H, None, None, 0, ctypes.byref(n), None) == E
        assert lib.xsknf_gpu_lb_sessions_ages(h, H, None, None, 0, None, None) == E
        assert lib.xsknf_gpu_lb_sessions_ages(h, H, None, a.ctypes.data, 4, ctypes.byref(n), None) == E
        assert lib.xsknf_gpu_lb_sessions_ages(h, H, k.ctypes.data, None, 4, ctypes.byref(n), None) == E
        assert (res == 99).all() and L.sessions_ages(H)[2] == 0
        # a NULL result, and a cap below the count
        L.sessions_put(*RC.stored(RC.chain_keys("home")[:3]))
        assert lib.xsknf_gpu_lb_sessions_ages(h, H, k.ctypes.data, a.ctypes.data, 2, ctypes.byref(n), None) == -errno.ENOSPC
        assert n.value == 3
        L.clock(4, which=H)
        assert lib.xsknf_gpu_lb_sessions_expire_host(h, 3, None) == 0 and L.info["host_sessions"] == 0
        if L.info["device_bytes"] == 0:   # a host-only object has no device form
            assert calls(None)[1::2] == [N] * 3
            with pytest.raises(_lib.XsknfGpuError):
                L.expire(0)
            with pytest.raises(_lib.XsknfGpuError):
                L.clock(1)


def test_an_object_without_ageing_is_as_before():
    """Never enabled: batches, puts and removals work as ever, the object's
    device_bytes hold no stamps, and the ageing calls refuse it."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 12, seed=44)
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        M = RC.Model(bk, 32, 64)
        bytes0 = L.info["device_bytes"]
        assert bytes0 in (0, 16 * 2 * lb.MAX_SERVICES + 16 * 1 + 32 * 64 + 16)
        umem, descs = RC.frames_of(sids)
        mu = umem.copy()
        v, st = lb.lb_host(umem, descs, L, AC.I, AC.NIF)
        mv, ms = M.batch(mu, descs, AC.I, AC.NIF)
        assert np.array_equal(v, mv) and np.array_equal(st, ms) and np.array_equal(umem, mu)
        got, want = L.sessions_remove(RC.key_records(sids[:9]), pair=True, which=H), M.remove(RC.key_records(sids[:9]), True)
        assert got.tolist() == want.tolist() == [18, 1] and RC.same_dump(L, M, H)
        assert L.info["device_bytes"] == bytes0
        with pytest.raises(_lib.XsknfGpuError):
            L.sessions_ages(H)
