"""The load balancer NF on the device (include/xsknf_gpu.h xsknf_gpu_lb_batch;
xsknf_amd/csrc/lb_device.hip, kernel_lb.h) against xsknf_gpu_lb_host on the same
inputs (tests/test_lb.py holds the host model to the dict model and to the
reference function's recorded results): every UMEM byte, every verdict, the
sorted session dump, the counters, the sentinels past verdicts[n), the
descriptors unchanged.  Sizes around the wave, the block's tile and the grid's
sweep, read from the code."""
import re

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import forward_cases as FWC
from tests import lb_cases as LC
from tests.test_lb import golden_dump, run_golden
from xsknf_amd import lb, route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = LC.code_constant(r"constexpr int kThreads = (\d+);")        # frames per block and step
G = T * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);")  # frames per sweep of the largest grid
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, G + 1]
SENT = 0x5eadbeef
ORDERED = lb.LB_STATS.index("ordered_batches")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def device_batch(dev, L, umem, descs, ingress, nif):
    """One xsknf_gpu_lb_batch through the C ABI: (UMEM after, verdicts, stats).
    The verdicts go into a sentinel-filled buffer of n + 64 words, the workspace
    is exactly as long as xsknf_gpu_lb_workspace says and starts as garbage."""
    n = descs.shape[0]
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    dv = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    ws = torch.full((lb.lb_workspace(n),), 0xa5, dtype=torch.uint8, device=dev)
    st = torch.full((8,), 77, dtype=torch.int64, device=dev) if n else torch.zeros(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        lb.lb_batch_ptr(du.data_ptr() if n else 0, umem.size, dd.data_ptr() if n else 0, n, ingress, nif, L,
                        dv.data_ptr(), ws.data_ptr(), ws.numel(), st.data_ptr(),
                        torch.cuda.current_stream(dev).cuda_stream)
    out = dv.cpu().numpy()
    assert (out[n:] == SENT).all(), "verdicts written past n"
    assert np.array_equal(dd.cpu().numpy(), np.ascontiguousarray(descs).view(np.uint8)), "descriptors written"
    return du.cpu().numpy(), out[:n], st.cpu().numpy().astype(np.uint64)


def check_batch(dev, L, umem, descs, ingress, nif, what="", ordered=0):
    """Device == host on one batch (each on its own session table of L)."""
    hu = umem.copy()
    hv, hs = lb.lb_host(hu, descs, L, ingress, nif)
    gu, gv, gs = device_batch(dev, L, umem, descs, ingress, nif)
    bad = np.nonzero(gv != hv)[0]
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {gv[bad[:8]]} != {hv[bad[:8]]}"
    bad = np.nonzero(gu != hu)[0]
    assert bad.size == 0, f"{what}: {bad.size} UMEM bytes differ, first at {bad[:8]}"
    assert int(gs[ORDERED]) == ordered, f"{what}: ordered-path counter {int(gs[ORDERED])}"
    gs[ORDERED] = 0
    assert np.array_equal(gs, hs), f"{what}: counters {gs} != {hs}"
    hk, hw = L.sessions_dump(lb.HOST_TABLE)
    gk, gw = L.sessions_dump(lb.DEVICE_TABLE)
    assert hk.tobytes() == gk.tobytes() and hw.tobytes() == gw.tobytes(), f"{what}: the session tables differ"
    i = L.info
    assert i["device_sessions"] == i["host_sessions"] == hk.shape[0]
    return hv, hs


def test_sizes_are_read_from_the_code():
    src = open(FC.ROOT + "/xsknf_amd/csrc/kernel_lb.h").read()
    assert len(re.findall(r"__launch_bounds__\(kThreads\)", src)) == 3
    assert len(re.findall(r"stride = gridDim\.x \* kThreads", src)) == 3
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/lb_device.hip").read()
    assert re.search(r"tiles < static_cast<uint32_t>\(lbk::kMaxBlocks\) \? tiles : lbk::kMaxBlocks", dsrc)
    assert T % 64 == 0 and G > T


@pytest.mark.parametrize("layout", ["packed", "aligned"])
def test_prepopulated_sessions_every_branch_and_phase(dev, layout):
    """Every branch x ihl 0..15 x TCP / UDP x both directions x all 16 start
    phases, packed back to back with zero gap (each frame's last bytes and the
    next frame's MACs share words), the last frame ending on the UMEM's last
    byte, out-of-UMEM descriptors mixed in; and the aligned 2 KiB layout.  No
    service: sessions exist only where they were put."""
    rng = np.random.default_rng(41)
    fl, ph = LC.sweep_frames(rng, phases=range(16) if layout == "packed" else (0,))
    if layout == "packed":
        # zero gap, the phase walk left to the frames' own lengths; every start phase occurs
        umem, descs = LC.pack_packed(fl, rng)
        starts = (descs["addr"] & ((1 << 48) - 1)) + (descs["addr"] >> 48)
        assert set((starts % 16).tolist()) == set(range(16))
        assert int(starts[-1]) + int(descs[-1]["len"]) == umem.size
        assert (starts[1:] == starts[:-1] + descs["len"][:-1]).all()
    else:
        umem, descs = FC.pack_aligned(fl, rng)
    ks, vs = LC.sessions_for(fl, rng, every=2)
    assert set(vs["dir"].tolist()) == {0, 1}
    descs = FC.with_outside(umem, descs, rng)
    with lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=4096) as L:
        L.sessions_put(ks, vs)
        hv, hs = check_batch(dev, L, umem, descs, 1, 3, layout)
        assert int(hs[1]) >= ks.shape[0] and int(hs[2]) and int(hs[3]) and not int(hs[4])


def test_sessions_created_in_the_batch(dev):
    """About 300 flows of 1-5 frames interleaved with backward frames before and
    after their flow's first frame; a second batch of the same flows finds every
    session.  The ordered counter stays 0: the parallel path ran."""
    rng = np.random.default_rng(42)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=300, filler=200)
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L:
        hv, hs = check_batch(dev, L, umem, descs, 2, 4, "first batch", ordered=0)
        assert int(hs[4]) == 600 and int(hs[2]) > 0 and int(hs[5]) == 0
        hv2, hs2 = check_batch(dev, L, umem, descs, 2, 4, "second batch", ordered=0)
        assert int(hs2[4]) == 0 and int(hs2[1]) > int(hs[1])   # backward frames ahead of their creator now hit


def test_one_flow_across_the_grid(dev):
    """Frames of one sid at indices 0, 63, 64, T-1, T, G+1 with differing source
    MACs among filler, backward frames between them: the backward session
    carries index 0's MAC."""
    rng = np.random.default_rng(43)
    bk = LC.make_backends(rng, services=2)
    n = G + 2
    fr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    fr[:, 12] = 0x86   # filler: not IPv4
    sid = LC.service_sid(rng, bk)
    bsid = LC.backward_sid(bk, sid)
    macs = {}
    for i in (0, 63, 64, T - 1, T, G + 1):
        macs[i] = rng.integers(0, 256, 6).tolist()
        fr[i] = np.frombuffer(LC.frame(rng, sid, length=64, smac=macs[i]), dtype=np.uint8)
    for i in (1, 65, T + 1, G):
        fr[i] = np.frombuffer(LC.frame(rng, bsid, length=64), dtype=np.uint8)
    descs = np.zeros(n, dtype=LC.frames.DESC_DTYPE)
    descs["addr"] = np.arange(n, dtype=np.uint64) * 64
    descs["len"] = 64
    with lb.LoadBalancer.from_backends(bk, max_sessions=16) as L:
        check_batch(dev, L, fr.reshape(-1), descs, 3, 4, "one flow", ordered=0)
        k, v = L.sessions_dump(lb.DEVICE_TABLE)
        back = v[v["dir"] == lb.TO_CLIENT]
        assert k.shape[0] == 2 and back.shape[0] == 1 and back[0]["mac"].tolist() == macs[0]


@pytest.mark.parametrize("which", ["existing_b", "shared_b", "vip_client"])
def test_each_ordered_cause_alone(dev, which):
    rng = np.random.default_rng(44)
    bk, (ks, vs), fl = LC.ordered_cause(rng, which)
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=64) as L:
        L.sessions_put(ks, vs)
        check_batch(dev, L, umem, descs, 2, 4, which, ordered=1)
        # the same frames again: every session exists, nothing is proposed
        check_batch(dev, L, umem, descs, 2, 4, which + " again", ordered=0)


def test_capacity_overflow_takes_the_ordered_path(dev):
    """max_sessions 8 with 6 new flows: the inserts fail in the loop's order."""
    rng = np.random.default_rng(45)
    bk = LC.make_backends(rng, services=3)
    sids = [LC.service_sid(rng, bk) for _ in range(6)]
    fl = []
    for s in sids:
        fl += [LC.frame(rng, s), LC.frame(rng, LC.backward_sid(bk, s))]
    fl += [LC.frame(rng, s) for s in sids]
    umem, descs = LC.pack_packed(fl, rng)
    with lb.LoadBalancer.from_backends(bk, max_sessions=8) as L:
        hv, hs = check_batch(dev, L, umem, descs, 0, 2, "overflow", ordered=1)
        assert [int(x) for x in hs[:6]] == [18, 16, 2, 0, 8, 4]
        check_batch(dev, L, umem, descs, 0, 2, "overflow again", ordered=1)


@pytest.fixture(scope="module")
def sized():
    rng = np.random.default_rng(46)
    bk = LC.make_backends(rng)
    umem, descs = LC.fixed_batch(rng, max(SIZES), bk)
    return bk, umem, descs


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(dev, sized, n):
    bk, umem, descs = sized
    with lb.LoadBalancer.from_backends(bk, max_sessions=1 << 18) as L:
        hv, hs = check_batch(dev, L, umem[:64 * n].copy(), descs[:n], 1, 2, f"n={n}", ordered=0)
        assert int(hs[0]) == n


def test_golden_fixture_through_the_c_abi(dev):
    g = np.load(LC.GOLDEN)
    with lb.LoadBalancer.from_backends(g["backends"], max_sessions=4096) as L:
        L.sessions_put(g["pre_keys"], g["pre_values"])
        ordered = []

        def call(b, umem, descs, ingress, nif):
            gu, gv, gs = device_batch(dev, L, umem, descs, ingress, nif)
            ordered.append(int(gs[ORDERED]))
            return gu, gv
        run_golden(g, call)
        assert ordered == [0, 1, 1]
        k, v = L.sessions_dump(lb.DEVICE_TABLE)
        wk, wv = golden_dump(g)
        assert k.tobytes() == wk.tobytes() and v.tobytes() == wv.tobytes()


def test_chain_lb_route_forward(dev):
    """lb_batch -> route_batch -> forward_frames on one stream with no host read
    between (the route's counts stay on the device), against the three host
    calls: every list entry and destination byte."""
    rng = np.random.default_rng(47)
    nif = 3
    bk = LC.make_backends(rng, ifaces=nif)
    fl = LC.flows_batch(rng, bk, flows=150, filler=100)
    umem, descs = FC.pack_aligned(fl, rng)
    n = descs.shape[0]
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L:
        hu = FWC.aligned_u8(umem.size)
        hu[:] = umem
        hv, hs = lb.lb_host(hu, descs, L, 0, nif)
        h_tx, h_fill, _, h_counts = route.route_host(descs, hv, nif)
        txa = FWC.aligned_descs(n)
        txa[:] = h_tx
        h_dst = [FWC.aligned_u8(umem.size, FWC.SENTINEL8) for _ in range(nif)]
        h_stats = route.forward_host(hu, h_dst, txa, h_counts)
        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            gv, gs = lb.lb_batch(du, dd, L, 0, nif)
            g_tx = torch.zeros((n, 2), dtype=torch.int64, device=dev)
            g_fill = torch.zeros(n, dtype=torch.int64, device=dev)
            ws = torch.zeros(route.route_workspace(n, nif) // 8, dtype=torch.int64, device=dev)
            route.route_batch_ptr(dd.data_ptr(), gv.data_ptr(), n, nif, g_tx.data_ptr(), g_fill.data_ptr(), 0,
                                  ws.data_ptr(), ws.numel() * 8, stream, sync=False)
            g_dst = [torch.full((umem.size,), FWC.SENTINEL8, dtype=torch.uint8, device=dev) for _ in range(nif)]
            fst = torch.zeros(3, dtype=torch.int64, device=dev)
            route.forward_frames_ptr(du.data_ptr(), umem.size, [t.data_ptr() for t in g_dst], [umem.size] * nif,
                                     g_tx.data_ptr(), ws.data_ptr(), n, fst.data_ptr(), stream, sync=False)
            torch.cuda.synchronize()
        assert np.array_equal(gv.cpu().numpy(), hv) and np.array_equal(du.cpu().numpy(), hu)
        counts = [int(c) for c in ws.cpu().numpy()[:nif + 1]]
        assert counts == h_counts[:nif + 1] and min(counts[:nif]) > 0
        total = sum(counts[:nif])
        assert np.array_equal(g_tx.cpu().numpy().view(np.uint8).reshape(-1)[:16 * total],
                              np.ascontiguousarray(h_tx).view(np.uint8).reshape(-1)[:16 * total])
        assert np.array_equal(g_fill.cpu().numpy().view(np.uint64)[:counts[nif]], h_fill[:counts[nif]])
        for i in range(nif):
            assert np.array_equal(g_dst[i].cpu().numpy(), h_dst[i]), f"interface {i}"
        assert [int(x) for x in fst.cpu().numpy()] == h_stats
        assert int(gs.cpu().numpy()[ORDERED]) == 0
