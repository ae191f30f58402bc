"""The lbfw NF on the device (include/xsknf_gpu.h xsknf_gpu_lbfw_batch;
xsknf_amd/csrc/lb_device.hip, kernel_lb.h lb_propose<true>) against
xsknf_gpu_lbfw_host on the same inputs (tests/test_lbfw.py holds the host model
to the dict model and to the reference function's recorded results): every UMEM
byte, every verdict, the sorted session dump, the counters, the ordered-path
counter, the sentinels past verdicts[n), the descriptors unchanged.  Sizes
around the wave, the block's tile and the grid's sweep, read from the code."""
import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import forward_cases as FWC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from xsknf_amd import lb, lbfw, route
from xsknf_amd.firewall import RULE_DTYPE, Acl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = LC.code_constant(r"constexpr int kThreads = (\d+);")        # frames per block and step
G = T * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);")  # frames per sweep of the largest grid
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, G + 1]
SENT = 0x5eadbeef
ORDERED, GATED = WC.ORDERED, WC.GATED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def device_batch(dev, A, L, umem, descs, ingress, nif):
    """One xsknf_gpu_lbfw_batch through the C ABI: (UMEM after, verdicts, stats).
    The verdicts go into a sentinel-filled buffer of n + 64 words, the workspace
    is exactly as long as xsknf_gpu_lb_workspace says and starts as garbage."""
    n = descs.shape[0]
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    dv = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    ws = torch.full((lb.lb_workspace(n),), 0xa5, dtype=torch.uint8, device=dev)
    st = torch.full((8,), 77, dtype=torch.int64, device=dev) if n else torch.zeros(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        lbfw.lbfw_batch_ptr(du.data_ptr() if n else 0, umem.size, dd.data_ptr() if n else 0, n, ingress, nif, A, L,
                            dv.data_ptr(), ws.data_ptr(), ws.numel(), st.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
    out = dv.cpu().numpy()
    assert (out[n:] == SENT).all(), "verdicts written past n"
    assert np.array_equal(dd.cpu().numpy(), np.ascontiguousarray(descs).view(np.uint8)), "descriptors written"
    return du.cpu().numpy(), out[:n], st.cpu().numpy().astype(np.uint64)


def check_batch(dev, A, L, umem, descs, ingress, nif, what="", ordered=0):
    """Device == host on one batch (each on its own session table of L).
    Returns the host's (UMEM after, verdicts, stats)."""
    hu = umem.copy()
    hv, hs = lbfw.lbfw_host(hu, descs, A, L, ingress, nif)
    gu, gv, gs = device_batch(dev, A, L, umem, descs, ingress, nif)
    bad = np.nonzero(gv != hv)[0]
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {gv[bad[:8]]} != {hv[bad[:8]]}"
    bad = np.nonzero(gu != hu)[0]
    assert bad.size == 0, f"{what}: {bad.size} UMEM bytes differ, first at {bad[:8]}"
    assert int(gs[ORDERED]) == ordered, f"{what}: ordered-path counter {int(gs[ORDERED])}"
    gs[ORDERED] = 0
    assert np.array_equal(gs, hs), f"{what}: counters {gs} != {hs}"
    assert WC.identity(hs)
    hk, hw = L.sessions_dump(lb.HOST_TABLE)
    gk, gw = L.sessions_dump(lb.DEVICE_TABLE)
    assert hk.tobytes() == gk.tobytes() and hw.tobytes() == gw.tobytes(), f"{what}: the session tables differ"
    i = L.info
    assert i["device_sessions"] == i["host_sessions"] == hk.shape[0]
    return hu, hv, hs


def starts_of(descs):
    return (descs["addr"] & ((1 << 48) - 1)) + (descs["addr"] >> 48)


@pytest.mark.parametrize("layout", ["packed", "aligned"])
def test_prepopulated_sessions_every_branch_and_phase(dev, layout):
    """The load balancer's decision sweep (every branch x ihl 0..15 x TCP / UDP x
    both directions x 16 start phases, zero gap, the last frame on the UMEM's
    last byte; and the aligned layout) with an ACL over every other session'd
    sid plus one-bit near misses of the ACL's keys.  An ACL'd frame keeps its
    bytes where the neighbour that shares its words is rewritten."""
    rng = np.random.default_rng(141)
    fl, ph = LC.sweep_frames(rng, phases=range(16) if layout == "packed" else (0,))
    if layout == "packed":
        umem, descs = LC.pack_packed(fl, rng)
        starts = starts_of(descs)
        assert set((starts % 16).tolist()) == set(range(16))
        assert int(starts[-1]) + int(descs[-1]["len"]) == umem.size
        assert (starts[1:] == starts[:-1] + descs["len"][:-1]).all()
    else:
        umem, descs = FC.pack_aligned(fl, rng)
    ks, vs = LC.sessions_for(fl, rng, every=1)   # every candidate: a gated frame's neighbours are rewritten
    assert set(vs["dir"].tolist()) == {0, 1}
    gate = np.arange(ks.shape[0]) % 4 < 2   # every other pair: both directions on either side of the gate
    held = [LC.key_bytes(k) for k in ks[gate]]
    near = [WC.flip(k, (13 * i) % 96) for i, k in enumerate(held)]
    near = [k for k in near if k not in set(held)]
    r, d = WC.rules(held + near, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(held))] + [9] * len(near))
    keys = FC.keys_of(umem, descs)
    n0 = descs.shape[0]
    descs = FC.with_outside(umem, descs, rng)
    with lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=8192) as L, \
            Acl.from_rules(r) as A:
        L.sessions_put(ks, vs)
        hu, hv, hs = check_batch(dev, A, L, umem, descs, 1, 3, layout)
        assert int(hs[GATED]) >= len(held) and int(hs[1]) >= ks.shape[0] - len(held) and int(hs[2]) and int(hs[3])
        assert set(vs["dir"][gate].tolist()) == set(vs["dir"][~gate].tolist()) == {0, 1}
        if layout == "packed":
            # gated frames between rewritten neighbours: their own bytes are the input's
            s = starts_of(descs)
            inside = [i for i in range(descs.shape[0]) if int(s[i]) + int(descs[i]["len"]) <= umem.size]
            assert len(inside) == n0
            changed = [not np.array_equal(hu[int(s[i]):int(s[i]) + int(descs[i]["len"])],
                                          umem[int(s[i]):int(s[i]) + int(descs[i]["len"])]) for i in inside]
            gated = [k in d for k in keys]
            assert not any(c and g for c, g in zip(changed, gated))
            assert sum(1 for j in range(1, n0 - 1) if gated[j] and (changed[j - 1] or changed[j + 1])) > 10


def test_sessions_created_in_the_batch(dev):
    """About 300 flows, a third of them ACL'd: those leave no session, the rest
    are created by the parallel path (ordered 0) and found by a second batch."""
    rng = np.random.default_rng(142)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=300, filler=200)
    umem, descs = LC.pack_packed(fl, rng)
    services = {(int(x["vaddr"]), int(x["vport"]), int(x["proto"])) for x in bk}
    fwd = [k for k in WC.frame_keys(fl) if (LC._u32(k, 4), LC._u16(k, 10), k[12]) in services]
    assert len(fwd) == 300
    r, d = WC.rules(fwd[::3], [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(100)])
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
        hu, hv, hs = check_batch(dev, A, L, umem, descs, 2, 4, "first batch", ordered=0)
        assert int(hs[4]) == 400 and int(hs[GATED]) >= 100 and int(hs[5]) == 0
        stored = {LC.key_bytes(k) for k in L.sessions_dump(lb.HOST_TABLE)[0]}   # (== the device table)
        assert not (stored & set(d)) and set(fwd) - set(d) <= stored
        hu2, hv2, hs2 = check_batch(dev, A, L, umem, descs, 2, 4, "second batch", ordered=0)
        assert int(hs2[4]) == 0 and int(hs2[1]) > int(hs[1]) and int(hs2[GATED]) == int(hs[GATED])


def _cause_inputs(which, gate_the_cause):
    rng = np.random.default_rng(144)
    bk, (ks, vs), fl = LC.ordered_cause(rng, which)
    distinct = WC.frame_keys(fl)
    extra_sids = [(0x0d000001 + i, 0x0e000001, 7000 + i, 53, 17) for i in range(4)]
    fl = fl[:2] + [LC.frame(rng, s) for s in extra_sids[:2]] + fl[2:] + [LC.frame(rng, s) for s in extra_sids[2:]]
    acl_keys = [WC.sid_key(s) for s in extra_sids]
    if gate_the_cause:
        # existing_b: [bsid, sid] -> the new flow; shared_b: [bsid, s1, s2] -> s2; vip_client: the flow that
        # hits service 2 (s2), whichever comes first
        if which == "existing_b":
            acl_keys.append(distinct[1])
        elif which == "shared_b":
            acl_keys.append(distinct[2])
        else:
            v2 = (0x0b00000b).to_bytes(4, "little")
            acl_keys.append([k for k in distinct if k[4:8] == v2][0])
    r, d = WC.rules(acl_keys, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(acl_keys))])
    return rng, bk, ks, vs, fl, r, d


@pytest.mark.parametrize("gate_the_cause", [False, True])
@pytest.mark.parametrize("which", ["existing_b", "shared_b", "vip_client"])
def test_each_ordered_cause(dev, which, gate_the_cause):
    """Each cause of the ordered path with unrelated ACL'd frames mixed in
    (ordered 1), and with the ACL on one of the two colliding flows, so that the
    cause is gone (ordered 0).  For the latter the dict model confirms on the
    CPU that the gated flow plays no part in the loop: the batch without its
    frames gives the other frames the same verdicts and bytes and leaves the
    same sessions, so nothing of the loop's order among the colliding flows is
    left to get wrong."""
    rng, bk, ks, vs, fl, r, d = _cause_inputs(which, gate_the_cause)
    umem, descs = LC.pack_packed(fl, rng)
    if gate_the_cause:
        keep = [i for i, f in enumerate(fl) if LC.frame_sid(f) not in d]
        assert len(keep) < len(fl) - 4
        m1, m2 = WC.Model(bk, 64), WC.Model(bk, 64)
        for m in (m1, m2):
            m.sessions_put(ks, vs)
        u1 = umem.copy()
        v1, _ = m1.batch(u1, descs, 2, 4, d)
        u2 = umem.copy()
        v2, _ = m2.batch(u2, descs[keep], 2, 4, d)
        s = starts_of(descs)
        assert np.array_equal(v1[keep], v2) and m1.dump()[0].tobytes() == m2.dump()[0].tobytes()
        assert m1.dump()[1].tobytes() == m2.dump()[1].tobytes()
        for i in keep:
            assert np.array_equal(u1[int(s[i]):int(s[i]) + len(fl[i])], u2[int(s[i]):int(s[i]) + len(fl[i])])
    with lb.LoadBalancer.from_backends(bk, max_sessions=64) as L, Acl.from_rules(r) as A:
        L.sessions_put(ks, vs)
        hu, hv, hs = check_batch(dev, A, L, umem, descs, 2, 4, which, ordered=0 if gate_the_cause else 1)
        assert int(hs[GATED]) >= 4
        # the same frames again: every session exists, nothing is proposed
        check_batch(dev, A, L, umem, descs, 2, 4, which + " again", ordered=0)


def test_capacity_counts_only_ungated_flows(dev):
    """max_sessions 8: four un-gated new flows fit exactly beside four gated
    ones (ordered 0); one more un-gated flow does not (ordered 1)."""
    rng = np.random.default_rng(145)
    bk = LC.make_backends(rng, services=3)
    sids = [LC.service_sid(rng, bk) for _ in range(9)]
    r, d = WC.rules([WC.sid_key(s) for s in sids[4:8]], [0, -1, 2, 5])
    for count, ordered in ((8, 0), (9, 1)):
        fl = []
        for s in sids[:count]:
            fl += [LC.frame(rng, s), LC.frame(rng, LC.backward_sid(bk, s))]
        fl += [LC.frame(rng, s) for s in sids[:count]]
        umem, descs = LC.pack_packed(fl, rng)
        with lb.LoadBalancer.from_backends(bk, max_sessions=8) as L, Acl.from_rules(r) as A:
            hu, hv, hs = check_batch(dev, A, L, umem, descs, 0, 2, f"{count} flows", ordered=ordered)
            assert int(hs[4]) == 8 and int(hs[GATED]) == 8 and int(hs[5]) == (0 if count == 8 else 2)
            assert L.info["device_sessions"] == 8


def test_acl_edge_cases(dev):
    """An ACL of a single (empty) slot, an empty ACL and acl=None give the same
    result, and with more than one interface that is the load balancer's."""
    rng = np.random.default_rng(146)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=60, filler=40)
    umem, descs = LC.pack_packed(fl, rng)
    none = np.zeros(0, dtype=RULE_DTYPE)
    with lb.LoadBalancer.from_backends(bk, max_sessions=1024) as L0:
        ru = umem.copy()
        rv, rs = lb.lb_host(ru, descs, L0, 1, 3)
    with Acl.from_rules(none, slots=1) as one, Acl.from_rules(none) as empty:
        assert one.info["slots"] == 1 and empty.info["rules"] == 0
        for A in (one, empty, None):
            with lb.LoadBalancer.from_backends(bk, max_sessions=1024) as L:
                hu, hv, hs = check_batch(dev, A, L, umem, descs, 1, 3, "edge", ordered=0)
                assert np.array_equal(hu, ru) and np.array_equal(hv, rv) and np.array_equal(hs, rs)


@pytest.fixture(scope="module")
def sized():
    rng = np.random.default_rng(147)
    bk = LC.make_backends(rng)
    umem, descs = LC.fixed_batch(rng, max(SIZES), bk)
    raw = umem.reshape(-1, 64)
    live = np.nonzero((raw[:, 12] == 8) & (raw[:, 13] == 0) & (raw[:, 14] == 0x45) & np.isin(raw[:, 23], (6, 17)))[0]
    keys = []
    for i in live[:1500].tolist() + live[-1500:].tolist():
        keys.append(bytes(raw[i, 26:38]) + bytes(raw[i, 23:24]))
    keys = list(dict.fromkeys(keys))[::3]
    r, d = WC.rules(keys, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(keys))])
    return bk, umem, descs, r


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes(dev, sized, n):
    bk, umem, descs, r = sized
    with lb.LoadBalancer.from_backends(bk, max_sessions=1 << 18) as L, Acl.from_rules(r) as A:
        hu, hv, hs = check_batch(dev, A, L, umem[:64 * n].copy(), descs[:n], 1, 2, f"n={n}", ordered=0)
        assert int(hs[0]) == n and (n < T or int(hs[GATED]) > 0)


@pytest.mark.parametrize("mode", ["afxdp", "combined"])
def test_golden_fixture_through_the_c_abi(dev, mode):
    g = np.load(WC.GOLDEN)
    with lb.LoadBalancer.from_backends(g["backends"], max_sessions=4096) as L, Acl.from_rules(g["rules"]) as A:
        L.sessions_put(g["pre_keys"], g["pre_values"])
        stats = []

        def call(b, umem, descs, ingress, nif):
            gu, gv, gs = device_batch(dev, A if mode == "afxdp" else None, L, umem, descs, ingress, nif)
            stats.append(gs)
            return gu, gv
        WC.run_golden(g, mode, call, lambda: L.sessions_dump(lb.DEVICE_TABLE))
        assert all(WC.identity(s) for s in stats)
        # batch 1 replaces a stored backward key, batch 2's shared backward key is gone only with the gate
        assert [int(s[ORDERED]) for s in stats] == ([0, 1, 0] if mode == "afxdp" else [0, 1, 1])


def test_alternating_with_the_load_balancer_on_one_object(dev):
    rng = np.random.default_rng(148)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=50, filler=30)
    umem, descs = LC.pack_packed(fl, rng)
    keys = WC.frame_keys(fl)
    r, d = WC.rules(keys[::4], [3] * len(keys[::4]))
    from tests.test_gpu_lb import check_batch as lb_check
    with lb.LoadBalancer.from_backends(bk, max_sessions=1024) as L, Acl.from_rules(r) as A:
        check_batch(dev, A, L, umem, descs, 0, 2, "lbfw", ordered=0)
        hv, hs = lb_check(dev, L, umem, descs, 0, 2, "lb on the same object", ordered=0)
        assert int(hs[4]) > 0   # the flows the gate held back are created now
        hu, hv2, hs2 = check_batch(dev, A, L, umem, descs, 0, 2, "lbfw again", ordered=0)
        assert int(hs2[4]) == 0 and int(hs2[GATED]) > 0


def test_chain_lbfw_route_forward(dev):
    """lbfw_batch -> route_batch -> forward_frames on one stream with no host
    read between, against the three host calls: every list entry and
    destination byte.  Gated frames with a positive action land in that
    interface's list."""
    rng = np.random.default_rng(149)
    nif = 3
    bk = LC.make_backends(rng, ifaces=nif)
    fl = LC.flows_batch(rng, bk, flows=150, filler=100)
    umem, descs = FC.pack_aligned(fl, rng)
    n = descs.shape[0]
    keys = WC.frame_keys(fl)[::3]
    r, d = WC.rules(keys, [(2, -1, 0, 1)[i % 4] for i in range(len(keys))])
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
        hu = FWC.aligned_u8(umem.size)
        hu[:] = umem
        hv, hs = lbfw.lbfw_host(hu, descs, A, L, 0, nif)
        h_tx, h_fill, _, h_counts = route.route_host(descs, hv, nif)
        txa = FWC.aligned_descs(n)
        txa[:] = h_tx
        h_dst = [FWC.aligned_u8(umem.size, FWC.SENTINEL8) for _ in range(nif)]
        h_stats = route.forward_host(hu, h_dst, txa, h_counts)
        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            gv, gs = lbfw.lbfw_batch(du, dd, A, L, 0, nif)
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
        st = gs.cpu().numpy()
        assert int(st[ORDERED]) == 0 and int(st[GATED]) > 0
        # a gated frame with action 2 is in interface 2's tx list, untouched
        fk = FC.keys_of(umem, descs)
        two = [i for i, k in enumerate(fk) if k in d and d[k] == 2]
        assert two and all(int(hv[i]) == 2 for i in two)
        lo = counts[0] + counts[1]
        g_addr = g_tx.cpu().numpy().view(np.uint64).reshape(-1, 2)[lo:lo + counts[2], 0]
        listed = set(int(x) for x in g_addr.tolist())
        assert all(int(descs[i]["addr"]) in listed for i in two)
        out2 = g_dst[2].cpu().numpy()
        for i in two:
            s, ln = int(descs[i]["addr"]), int(descs[i]["len"])
            assert np.array_equal(out2[s:s + ln], umem[s:s + ln])
