"""Ageing of the load balancer's DEVICE session table (include/xsknf_gpu.h
xsknf_gpu_lb_aging_enable, _clock, _sessions_expire, _sessions_ages;
xsknf_amd/csrc/kernel_lb_stamp.h, kernel_lb_expire.h, lb_remove_device.hip)
against the model of tests/lb_age_cases.py.  Every step goes to the device table
and, as its host form, to the host table; after every step both sessions_ages
dumps, both results and the counts equal the model.  Batches run through
check_batch of tests/test_gpu_lb.py (device == host, byte for byte) and the
model.  The cases are tests/test_lb_age.py's, plus what only the device has:
the grid's edges, the stream's order and device_bytes."""
import errno
import re

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import lb_age_cases as AC
from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from xsknf_amd import _lib, lb
from xsknf_amd.firewall import Acl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = LC.code_constant(r"constexpr int kThreads = (\d+);", "kernel_lb.h")                   # frames per block and step
G = T * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);", "kernel_lb.h")             # frames per sweep of the largest grid
TR = LC.code_constant(r"constexpr int kThreads = (\d+);", "kernel_lb_remove.h")           # slots per block and step
GR = TR * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);", "kernel_lb_remove.h")    # slots per sweep
H, D = lb.HOST_TABLE, lb.DEVICE_TABLE
I, NIF = AC.I, AC.NIF
CREATED, REWRITTEN = AC.CREATED, AC.REWRITTEN


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def make(dev):
    return lambda bk, max_sessions, slots, enable=True: AC.Rig(bk, max_sessions, slots, dev, enable)


def test_sizes_are_read_from_the_code():
    for name, ns in (("kernel_lb_stamp.h", "lb_stamp"), ("kernel_lb_expire.h", "lb_expire")):
        src = open(FC.ROOT + "/xsknf_amd/csrc/" + name).read()
        assert len(re.findall(r"__launch_bounds__\(kThreads\)", src)) == 1, name
        assert len(re.findall(r"stride = gridDim\.x \* kThreads", src)) == 1, name
        assert "constexpr int k" not in src, f"{name} has sizes of its own"
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/lb_remove_device.hip").read()
    assert re.search(r"lbr::lb_expire, grid_for\(a\.slots\), dim3\(lbr::kThreads\)", dsrc)
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/lb_device.hip").read()
    assert re.search(r"lbk::lb_stamp, grid, dim3\(lbk::kThreads\)", dsrc)
    assert T % 64 == 0 and G > T and GR & (GR - 1) == 0


def test_enable_on_a_filled_table(make):
    AC.case_enable_on_a_filled_table(make)


def test_hits_stamp_the_session_they_use(make):
    AC.case_hits(make)


def test_new_flows_and_a_replaced_backward_session(make):
    AC.case_new_flows(make)


def test_a_full_table_has_room_after_expire(make):
    AC.case_full_table(make)


def test_the_pair_rule(make):
    AC.case_pair_rule(make)


def test_bounds_of_max_idle_and_a_wrapped_clock(make):
    AC.case_bounds(make)


@pytest.mark.parametrize("trigger", ["expire", "remove", "drain"])
def test_a_rebuild_carries_the_stamps(make, trigger):
    AC.case_rebuild(make, trigger)


def test_lbfw_gated_frames_stamp_nothing(make):
    AC.case_lbfw(make, Acl.from_rules)


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_a_mixed_run(make, seed):
    AC.case_mixed_run(make, seed)


def test_batches_around_the_block(make):
    """T - 1, T and T + 1 frames, each batch half hits on earlier flows (their
    stamps move, those of the flows beside them do not) and half new flows."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 3 * T + 64, seed=51)
    with make(bk, 4096, 8192) as R:
        R.batch(*RC.fast_frames(sids[:64]), "sixty-four flows at 0")
        at = 64
        for t, n in enumerate((T - 1, T, T + 1)):
            R.clock(10 + t)
            known = sids[t:at:2][:n // 2]
            new = sids[at:at + n - len(known)]
            at += len(new)
            mix = known + new
            order = np.random.default_rng(52 + t).permutation(n)
            hv, hs = R.batch(*RC.fast_frames([mix[j] for j in order]), f"n = {n}")
            assert int(hs[CREATED]) == 2 * len(new) and int(hs[REWRITTEN]) == n
        assert set(R.ages_of(sids[:at])) == {0, 1, 2} and R.ages_of([CC.bwd_sid(bk, sids[0])]) == [12]


def test_one_batch_past_the_largest_grid(make):
    """G + 1 frames, filler but for hits and new flows at the first indices, at
    G - 1 and at G, the frame the first lane takes in its second trip."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 8, seed=53)
    with make(bk, 64, 128) as R:
        R.batch(*RC.frames_of(sids[:4]), "four flows at 0")
        R.clock(9)
        b = CC.Batch(G + 1, 54)
        where = {0: sids[0], 1: sids[4], T: sids[5], G - 1: sids[1], G: sids[6]}
        for i, s in where.items():
            b.put(i, s, ("x", s))
        hv, hs = R.batch(*b.arrays(), "G + 1 frames", model=sorted(where))
        assert int(hs[CREATED]) == 6 and int(hs[REWRITTEN]) == 5 and int(hs[0]) == G + 1
        assert R.ages_of(sids[:7]) == [0, 0, 9, 9, 0, 0, 0]


def test_expire_over_two_sweeps_of_the_grid(make):
    """A table of 2 G slots, 2000 flows, about half of them idle: one expire."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 2000, seed=55)
    with make(bk, 8192, 2 * GR) as R:
        assert R.L.info["slots"] == 2 * GR
        R.batch(*RC.fast_frames(sids), "two thousand flows at 0")
        R.clock(50)
        keep = np.random.default_rng(56).permutation(2000)[:1000].tolist()
        R.batch(*RC.fast_frames([sids[j] if j & 1 else CC.bwd_sid(bk, sids[j]) for j in keep]), "a thousand hits at 50")
        R.clock(60)
        assert R.expire(20) == [2000, 0]
        assert len(R.M.sessions) == 2000
        R.clock(200)
        assert R.expire(100) == [2000, 0]


def test_stream_order(dev, make):
    """clock(10), batch A, clock(20), expire(5), batch B enqueued on one stream
    with one synchronize at the end: A stamps with 10, so nothing of it outlives
    the expire at 20, and B creates every flow anew with stamp 20."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 96, seed=57)
    a_umem, descs = RC.fast_frames(sids[:48] + sids[64:80])
    b_umem, b_descs = RC.fast_frames(sids[:64] + sids[72:96])
    with make(bk, 1024, 2048) as R:
        L, M = R.L, R.M
        R.batch(*RC.fast_frames(sids[:64]), "sixty-four flows at 0")
        ua, ub = torch.from_numpy(a_umem).to(dev), torch.from_numpy(b_umem).to(dev)
        da = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        db = torch.from_numpy(b_descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        wa, wb = (torch.empty(lb.lb_workspace(d.shape[0]), dtype=torch.uint8, device=dev) for d in (da, db))
        torch.cuda.synchronize()
        L.clock(10)
        va, sa = lb.lb_batch(ua, da, L, I, NIF, workspace=wa)
        L.clock(20)
        res = L.expire(5)
        vb, sb = lb.lb_batch(ub, db, L, I, NIF, workspace=wb)
        # the host forms and the model, step by step
        ha, hb = a_umem.copy(), b_umem.copy()
        L.clock(10, which=H)
        M.clock = 10
        hva, hsa = lb.lb_host(ha, descs, L, I, NIF)
        mva, msa = M.batch(a_umem.copy(), descs, I, NIF)
        L.clock(20, which=H)
        M.clock = 20
        hres, want = L.expire(5, which=H), M.expire(5)
        hvb, hsb = lb.lb_host(hb, b_descs, L, I, NIF)
        mvb, msb = M.batch(b_umem.copy(), b_descs, I, NIF)
        torch.cuda.synchronize()
        assert want.tolist() == [160, 0] and hres.tolist() == res.cpu().tolist() == want.tolist()
        for got, host, model in ((va, hva, mva), (vb, hvb, mvb)):
            assert np.array_equal(got.cpu().numpy(), host) and np.array_equal(host, model)
        for got, host, model in ((sa, hsa, msa), (sb, hsb, msb)):
            assert got.cpu().numpy().astype(np.uint64).tolist() == host.tolist() == model.tolist()
        assert int(hsa[CREATED]) == 32 and int(hsb[CREATED]) == 176 and int(hsb[AC.ORDERED]) == 0
        assert np.array_equal(ua.cpu().numpy(), ha) and np.array_equal(ub.cpu().numpy(), hb)
        R.check("after the stream")
        assert set(R.ages_of(sids[:64] + sids[72:96])) == {0}


def test_device_bytes_and_errors(dev):
    """What ageing allocates, and when: 4 B per slot and the clock's 16 B at
    enable, the spare table's stamps with the first removal -- or at enable if
    the spare table is already there.  An object that never enables ageing holds
    none of it, and the ageing calls refuse it."""
    E = -errno.EINVAL
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 6, seed=58)
    base = 16 * 2 * lb.MAX_SERVICES + 16 * 1 + 32 * 64 + 16
    lib = _lib.load()
    res = torch.zeros(4, dtype=torch.int64, device=dev)
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:      # never enabled
        from tests.test_gpu_lb import check_batch

        assert L.info["device_bytes"] == base
        check_batch(dev, L, *RC.frames_of(sids), I, NIF, "no ageing")
        L.sessions_remove(RC.key_records(sids[:1]), pair=True)
        torch.cuda.synchronize()
        assert L.info["device_bytes"] == base + 32 * 64 and L.info["device_sessions"] == 10
        assert lib.xsknf_gpu_lb_clock(L.handle, D, 1, None) == E
        assert lib.xsknf_gpu_lb_sessions_expire(L.handle, 0, res.data_ptr(), None) == E
        with pytest.raises(_lib.XsknfGpuError):
            L.sessions_ages(D)
        L.aging_enable()                                                          # the spare table exists
        assert L.info["device_bytes"] == base + 32 * 64 + 4 * 64 + 16 + 4 * 64
        assert L.sessions_ages(D)[1].tolist() == [0] * 10
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        L.aging_enable()
        L.aging_enable()
        assert L.info["device_bytes"] == base + 4 * 64 + 16
        assert lib.xsknf_gpu_lb_sessions_expire(L.handle, 0, res.data_ptr() + 4, None) == E
        assert lib.xsknf_gpu_lb_clock(L.handle, 2, 1, None) == E
        assert L.expire(0).cpu().tolist() == [0, 0]
        assert L.info["device_bytes"] == base + 4 * 64 + 16 + 32 * 64 + 4 * 64
        assert lib.xsknf_gpu_lb_sessions_expire(L.handle, 0, None, None) == 0     # a NULL result
        torch.cuda.synchronize()
