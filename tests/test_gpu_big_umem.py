"""The UMEM-addressing kernels with their frames around byte 2^32 of a device UMEM
of S = 2^32 + 8 MiB bytes (tests/big_umem_cases.py: the layout, the decoy 2^32
below every frame, the straddler's k table; tests/test_big_umem.py holds the host
forms to the same models): firewall_lookup, the load balancer's and lbfw's
kernels on the parallel and the ordered path, macswap_pass, route + forward_frames
into a second S-byte UMEM, every launch shape of the checksummer that
tests/test_gpu_parity.py runs, the device planner, and the multi-device calls
(span and packed scatter planned on the host and on the device, process, return)
over every device the process sees.  The references are the pure-Python models
and the RFC 1071 oracle on the window.  After every run, on the device: the
window and the tail equal the model's bytes, the decoy is as uploaded, every
other byte of the UMEM is zero -- so an offset that lost bit 32, or went through
a signed 32-bit intermediate, fails a verdict or a byte instead of passing.

Left out: the checksummer's host-path contexts (ZEROCOPY / STAGED / RESIDENT),
which would pin 4 GiB of host memory on a shared machine, and bases above 2^33
beyond the 128 GiB test of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import big_umem_cases as BC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as LBC
from tests import macswap_cases as MC
from tests import route_cases as RC
from tests.test_gpu_parity import SHAPES, launch_cfg
from tests.test_gpu_plan_dev import check_plan
from xsknf_amd import ChecksummerOptions, _lib, firewall, frames, lb, lbfw, macswap, multi, route

K_ALL, K_FEW, _ids = BC.K_ALL, BC.K_FEW, BC.k_ids

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = 0x5eadbeef
ORDERED = lb.LB_STATS.index("ordered_batches")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def umems(dev):
    """Two device UMEMs of S bytes, allocated once."""
    free, _ = torch.cuda.mem_get_info(dev)
    need = 2 * BC.S + (4 << 30)
    if free < need:
        pytest.skip(f"{free >> 20} MiB free on the device, {need >> 20} MiB needed")
    pair = [torch.zeros(BC.S, dtype=torch.uint8, device=dev) for _ in range(2)]
    assert all(t.data_ptr() % 4096 == 0 for t in pair)
    yield pair
    del pair
    torch.cuda.empty_cache()


@pytest.fixture
def umem(umems):
    umems[0].zero_()
    return umems[0]


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def put(buf, L):
    for at, b in L.regions():
        buf[at:at + b.size].copy_(torch.from_numpy(b))


def check(buf, L, win, tail, what=""):
    """The three comparisons, on the device."""
    for name, at, want in (("window", BC.WIN, win), ("tail", BC.S - BC.TAIL, tail), ("decoy", 0, L.decoy)):
        got = buf[at:at + want.size]
        if not torch.equal(got, torch.from_numpy(np.ascontiguousarray(want)).to(buf.device)):
            bad = np.flatnonzero(got.cpu().numpy() != want)
            raise AssertionError(f"{what}: {bad.size} bytes of the {name} differ, first at "
                                 f"{[hex(at + int(x)) for x in bad[:8]]}")
    for lo, hi in L.zero_spans():
        assert int(torch.count_nonzero(buf[lo:hi].view(torch.int64))) == 0, \
            f"{what}: a byte was written in [{lo:#x}, {hi:#x})"


def same_verdicts(got, want, what=""):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"


# ---- the firewall -------------------------------------------------------------------

@pytest.mark.parametrize("k,proto", K_ALL, ids=_ids(K_ALL))
def test_firewall(dev, umem, k, proto):
    L, rules = BC.firewall_case(k, proto)
    m, md = L.compact()
    want = FC.model(m, md, FC.acl_dict(rules))
    assert want[L.straddler] == 31 and (want[L.outside] == -1).all()
    put(umem, L)
    dd = _to_dev(L.descs, dev)
    with firewall.Acl.from_rules(rules) as acl:
        got = firewall.firewall_batch(umem, dd, acl).cpu().numpy()
    same_verdicts(got, want, f"firewall k={k}")
    check(umem, L, L.win, L.tail, f"firewall k={k}")
    assert np.array_equal(dd.cpu().numpy(), L.descs.view(np.uint8))


def test_firewall_through_the_c_abi(dev, umem):
    """xsknf_gpu_firewall_batch itself, with ctypes: umem_size as a uint64_t past 2^32."""
    L, rules = BC.firewall_case(30, 17, seed=1)
    m, md = L.compact()
    want = FC.model(m, md, FC.acl_dict(rules))
    put(umem, L)
    dd = _to_dev(L.descs, dev)
    n = L.descs.shape[0]
    dv = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    with firewall.Acl.from_rules(rules) as acl, torch.cuda.device(dev):
        rc = _lib.load().xsknf_gpu_firewall_batch(
            ctypes.c_void_p(umem.data_ptr()), ctypes.c_uint64(BC.S), ctypes.c_void_p(dd.data_ptr()), n, acl.handle,
            ctypes.c_void_p(dv.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0
        out = dv.cpu().numpy()
    assert (out[n:] == SENT).all()
    same_verdicts(out[:n], want, "the C ABI")
    check(umem, L, L.win, L.tail, "the C ABI")


# ---- the load balancer and lbfw -------------------------------------------------------

def _lb_run(dev, umem, run, k, proto, gated):
    L, bk, (ks, vs) = BC.lb_case(run, k, proto)
    m, md = L.compact()
    rules, gate = BC.gate_for(L, np.random.default_rng(k)) if gated else (None, None)
    model = (LBC if gated else LC).Model(bk, 4096)
    model.sessions_put(ks, vs)
    wv, ws = model.batch(m, md, 1, 3, acl=gate) if gated else model.batch(m, md, 1, 3)
    assert (wv[L.outside] == -1).all()
    put(umem, L)
    dd = _to_dev(L.descs, dev)
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as lbo:
        lbo.sessions_put(ks, vs)
        if gated:
            with firewall.Acl.from_rules(rules) as acl:
                gv, gs = lbfw.lbfw_batch(umem, dd, acl, lbo, 1, 3)
                gv, gs = gv.cpu().numpy(), gs.cpu().numpy().astype(np.uint64)
        else:
            gv, gs = lb.lb_batch(umem, dd, lbo, 1, 3)
            gv, gs = gv.cpu().numpy(), gs.cpu().numpy().astype(np.uint64)
        gk, gw = lbo.sessions_dump(lb.DEVICE_TABLE)
    what = f"{'lbfw' if gated else 'lb'} {run} k={k}"
    same_verdicts(gv, wv, what)
    # the ordered cause alone stands the batch down; the other two runs hold nothing that depends on
    # the loop's order, so they exercise lb_propose / lb_apply / lb_commit
    assert int(gs[ORDERED]) == (1 if run == "ordered" else 0), f"{what}: ordered_batches {int(gs[ORDERED])}"
    gs[ORDERED] = 0
    assert np.array_equal(gs, ws), f"{what}: stats {gs} != {ws}"
    wk, wvv = model.dump()
    assert gk.tobytes() == wk.tobytes() and gw.tobytes() == wvv.tobytes(), f"{what}: the session tables differ"
    check(umem, L, *L.split(m), what=what)
    assert np.array_equal(dd.cpu().numpy(), L.descs.view(np.uint8))


@pytest.mark.parametrize("k,proto", K_ALL, ids=_ids(K_ALL))
def test_lb_prepopulated_sessions(dev, umem, k, proto):
    _lb_run(dev, umem, "prepopulated", k, proto, gated=False)


@pytest.mark.parametrize("run", ["created", "ordered"])
@pytest.mark.parametrize("k,proto", K_FEW, ids=_ids(K_FEW))
def test_lb_sessions_created_and_the_ordered_path(dev, umem, k, proto, run):
    _lb_run(dev, umem, run, k, proto, gated=False)


@pytest.mark.parametrize("run", ["prepopulated", "created", "ordered"])
@pytest.mark.parametrize("k,proto", K_FEW, ids=_ids(K_FEW))
def test_lbfw(dev, umem, k, proto, run):
    _lb_run(dev, umem, run, k, proto, gated=True)


# ---- macswap ------------------------------------------------------------------------

@pytest.mark.parametrize("double", [False, True], ids=["swap", "double"])
@pytest.mark.parametrize("lens", [(14,), (14, 15, 17, 13)], ids=["14", "cycling"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_macswap(dev, umem, k, lens, double):
    L = BC.macswap_case(k, lens)
    m, md = L.compact()
    wu, wv = MC.model(m, md, 1, MC.REDIRECT, double, 3)
    put(umem, L)
    dd = _to_dev(L.descs, dev)
    gv = macswap.macswap_batch(umem, dd, 1, double_macswap=double, num_interfaces=3).cpu().numpy()
    same_verdicts(gv, wv, f"macswap k={k}")
    check(umem, L, *L.split(wu), what=f"macswap k={k}")


# ---- macswap -> route -> forward ------------------------------------------------------

@pytest.mark.parametrize("k", BC.K_COPY)
def test_macswap_route_forward_chain(dev, umems, k):
    """Interface 0 has the second S-byte UMEM, interface 1 the rx UMEM; the
    forward's capacity cuts the window's list in the middle."""
    rx, dst = umems
    rx.zero_()
    dst.zero_()
    L = BC.forward_case(k)
    D = L.other(np.random.default_rng(k))
    mu, mv, (tx, fill, order, counts), cap, cut, du, stats = BC.forward_expectation(L, D)
    put(rx, L)
    put(dst, D)
    n, nif = L.descs.shape[0], 2
    dd = _to_dev(L.descs, dev)
    gtx = torch.full((n * 16,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    gfill = torch.full((n * 8,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    god = torch.full((n * 4,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    ws = torch.empty(route.route_workspace(n, nif), dtype=torch.uint8, device=dev)
    gst = torch.zeros(route.FORWARD_STATS, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        v = macswap.macswap_batch(rx, dd, 1, num_interfaces=nif)
        route.route_batch_ptr(dd.data_ptr(), v.data_ptr(), n, nif, gtx.data_ptr(), gfill.data_ptr(), god.data_ptr(),
                              ws.data_ptr(), ws.numel(), s, sync=False)
        route.forward_frames_ptr(rx.data_ptr(), BC.S, [dst.data_ptr(), rx.data_ptr()], [BC.S, BC.S], gtx.data_ptr(),
                                 ws.data_ptr(), cap, gst.data_ptr(), s, sync=False)
        torch.cuda.synchronize(dev)
    same_verdicts(v.cpu().numpy(), mv, "chain")
    gcounts = [int(c) for c in ws[:8 * (nif + 1)].cpu().numpy().view(np.uint64)]
    RC.same_as((gtx.cpu().numpy().view(frames.DESC_DTYPE), gfill.cpu().numpy().view(np.uint64),
                god.cpu().numpy().view(np.uint32), gcounts), (tx, fill, order, counts), n, "chain")
    assert [int(x) for x in gst.cpu().numpy()] == stats
    check(rx, L, *L.split(mu), what="the rx UMEM")
    check(dst, D, *D.split(du), what="the destination")


# ---- the checksummer's device batches ---------------------------------------------------

def _csum(dev, umem, shape, k, fused=None, store_unchanged=False, iters=2, nif=3, ingress=1):
    L = BC.csum_case(sum(shape), k)
    m, md = L.compact()
    ov = BC.oracle_verdicts(L, m, md, ingress=ingress, iters=iters, action=O.REDIRECT, nif=nif)
    assert (ov >= 0).sum() > 300
    put(umem, L)
    dd = _to_dev(L.descs, dev)
    n = L.descs.shape[0]
    v = torch.empty(n, dtype=torch.int32, device=dev)
    cfg = launch_cfg(shape, fused=fused)
    if store_unchanged:
        cfg.fused_stores += 32
    with torch.cuda.device(dev):
        rc = _lib.load().xsknf_gpu_checksum_batch_cfg(
            ctypes.c_void_p(umem.data_ptr()), BC.S, ctypes.c_void_p(dd.data_ptr()), n, ingress,
            ctypes.byref(_lib.CsumOpts(iters, O.REDIRECT, nif, 0)), ctypes.c_void_p(v.data_ptr()), ctypes.byref(cfg), None)
        assert rc == 0
        torch.cuda.synchronize(dev)
    return L, m, ov, v.cpu().numpy()


def _shape_of(s):
    return s.values[0] if hasattr(s, "values") else s


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, _shape_of(s))) for s in SHAPES])
def test_checksummer_launch_shapes(dev, umem, shape):
    """Every shape of test_every_launch_shape_is_bit_exact, under its marks: the
    product shapes always, the others in the A/B build."""
    k = BC.K_CSUM[sum(shape) % len(BC.K_CSUM)]
    L, m, ov, gv = _csum(dev, umem, shape, k)
    same_verdicts(gv, ov, f"{shape} k={k}")
    check(umem, L, *L.split(m), what=f"{shape} k={k}")


def test_checksummer_store_unchanged_and_records(dev, umem):
    """One product shape with fused_stores + 32 (the unchanged checks stored
    again), and in records-only mode: the UMEM as it was, every frame without a
    record carrying the oracle's verdict."""
    shape = (16, 2, 2, 0, 0, 1, 24)
    L, m, ov, gv = _csum(dev, umem, shape, 41, store_unchanged=True)
    same_verdicts(gv, ov, "store32")
    check(umem, L, *L.split(m), what="store32")
    umem.zero_()
    L, m, ov, gv = _csum(dev, umem, shape, 41, fused=3, iters=1, nif=1, ingress=0)
    tagged = (gv.view(np.uint32) & 0xC0000000) == 0x40000000
    assert 0 < tagged.sum() and (ov[tagged] >= 0).all()
    same_verdicts(np.where(tagged, 0, gv), np.where(tagged, 0, ov), "records")
    check(umem, L, L.win, L.tail, what="records")


# ---- the device planner -----------------------------------------------------------------

@pytest.mark.parametrize("nshards", [1, 3, 8])
def test_shard_plan_dev(dev, nshards):
    """xsknf_gpu_shard_plan_dev on descriptors with these addresses, both modes,
    against the host planner (which tests/test_big_umem.py holds to shard.py)."""
    L = BC.forward_case(9)
    ranges, spans, sizes = check_plan(dev, L.descs, nshards, BC.S, umem_addr=0x7f00fffffff9)
    assert any(b0 < BC.B <= b1 for b0, b1 in spans) and max(b1 for _, b1 in spans) == BC.S
    assert multi.shard_plan(L.descs, nshards, BC.S) == (ranges, spans)


# ---- the multi-device calls ----------------------------------------------------------------

def _multi_case(umem):
    """The checksummer batch around 2^32 in the root UMEM: (layout, the compact
    array after the oracle's pass, the oracle's verdicts, the longest frame)."""
    L = BC.csum_case(77, 41)
    m, md = L.compact()
    ov = BC.oracle_verdicts(L, m, md, ingress=0, iters=1, action=O.REDIRECT, nif=1)
    put(umem, L)
    inr = np.ones(L.descs.shape[0], dtype=bool)
    inr[L.outside] = False
    return L, m, ov, int(L.descs["len"][inr].max())


def _span_shards(mdev, L, ndev, win=None, tail=None, verdicts=None):
    """Every shard of a span scatter against multi.shard_plan / shard_rebase:
    frame range, span, rebased descriptors and the span's bytes."""
    ranges, spans = multi.shard_plan(L.descs, ndev, BC.S)
    assert max(b1 for _, b1 in spans) == BC.S and min(b0 for b0, b1 in spans if b1) < BC.B
    for k in range(ndev):
        info = mdev.shard_info(k)
        assert (info["frame_lo"], info["frame_hi"]) == ranges[k] and (info["span_lo"], info["span_hi"]) == spans[k]
        assert info["flags"] == 0
        su, sv, sd = mdev.fetch(k, descs=True)
        lo, hi = ranges[k]
        want = multi.shard_rebase(L.descs[lo:hi], spans[k][0], BC.S)
        assert np.array_equal(sd.view(np.uint8), want.view(np.uint8)), f"shard {k}: rebased descriptors"
        bad = np.flatnonzero(su != L.image(*spans[k], win, tail))
        assert bad.size == 0, f"shard {k}: {bad.size} span bytes differ, first at {bad[:8] + spans[k][0]}"
        if verdicts is not None:
            same_verdicts(sv, verdicts[lo:hi], f"shard {k}")


def _packed_shards(mdev, L, ndev, umem):
    """Every shard of a packed scatter against multi.pack_plan: descriptors,
    packed size and every frame's bytes in its slot."""
    ranges, _ = multi.shard_plan(L.descs, ndev, BC.S)
    bounds = [0] + [hi for _, hi in ranges]
    want, sizes = multi.pack_plan(L.descs, bounds, umem.data_ptr(), BC.S)
    outside = set(L.outside.tolist())
    for k in range(ndev):
        info = mdev.shard_info(k)
        assert (info["frame_lo"], info["frame_hi"]) == ranges[k] and info["flags"] == _lib.SHARD_PACKED
        assert (info["span_lo"], info["span_hi"]) == (0, sizes[k])
        su, sv, sd = mdev.fetch(k, descs=True)
        lo, hi = ranges[k]
        assert np.array_equal(sd.view(np.uint8), want[lo:hi].view(np.uint8)), f"shard {k}: packed descriptors"
        for f in range(lo, hi):
            if f in outside:
                assert int(sd["addr"][f - lo]) >= su.size
                continue
            off, ln, p = BC.offset_of(int(L.descs["addr"][f])), int(L.descs["len"][f]), int(sd["addr"][f - lo])
            assert np.array_equal(su[p:p + ln], L.image(off, off + ln)), f"frame {f}: packed bytes"


@pytest.mark.parametrize("on_device", [False, True], ids=["scatter", "scatter_dev"])
def test_multi_span_scatter_and_process(dev, umem, on_device):
    """xsknf_gpu_multi_scatter / _scatter_dev(span) of a root UMEM of S bytes,
    then _multi_process: the shards before and after the pass, the counters, and
    the root UMEM as it was."""
    ndev = torch.cuda.device_count()
    L, m, ov, lmax = _multi_case(umem)
    dd = _to_dev(L.descs, dev)
    torch.cuda.synchronize()
    with multi.MultiDevice(range(ndev)) as mdev:
        if on_device:
            mdev.scatter_dev(0, umem.data_ptr(), BC.S, dd.data_ptr(), L.descs.shape[0], packed=False)
        else:
            mdev.scatter(0, umem.data_ptr(), BC.S, L.descs)
        _span_shards(mdev, L, ndev)
        mdev.process(ChecksummerOptions(), frame_len_max=lmax)
        _span_shards(mdev, L, ndev, *L.split(m), verdicts=ov)
        got = mdev.counters()
    want = multi.expected_counters(m, L.rebase(L.descs), ov)
    for name in ("frames", "bytes", "drop", "forward", "checks_sum"):      # (the sixth weighs absolute offsets)
        assert got[name] == want[name], name
    check(umem, L, L.win, L.tail, what="the root UMEM after a span scatter")


@pytest.mark.parametrize("on_device", [False, True], ids=["scatter_packed", "scatter_dev"])
def test_multi_packed_scatter_and_return(dev, umem, on_device):
    """xsknf_gpu_multi_scatter_packed / _scatter_dev(packed), then _multi_return:
    the packed shards against the host's pack plan, the returned root UMEM and
    verdicts against the oracle, the decoy and every other byte untouched."""
    ndev = torch.cuda.device_count()
    L, m, ov, lmax = _multi_case(umem)
    n = L.descs.shape[0]
    dd = _to_dev(L.descs, dev)
    v = torch.full((n,), 0x7eadbeef, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with multi.MultiDevice(range(ndev)) as mdev:
        if on_device:
            mdev.scatter_dev(0, umem.data_ptr(), BC.S, dd.data_ptr(), n, packed=True)
        else:
            mdev.scatter_packed(0, umem.data_ptr(), BC.S, L.descs)
        _packed_shards(mdev, L, ndev, umem)
        check(umem, L, L.win, L.tail, what="the root UMEM after a packed scatter")
        mdev.return_results(umem.data_ptr(), v.data_ptr(), ChecksummerOptions(), frame_len_max=lmax)
    torch.cuda.synchronize()
    same_verdicts(v.cpu().numpy(), ov, "returned verdicts")
    check(umem, L, *L.split(m), what="the returned root UMEM")
