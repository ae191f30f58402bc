"""The macswap NF on the device (include/xsknf_gpu.h xsknf_gpu_macswap_batch;
xsknf_amd/csrc/macswap_device.hip, kernel_macswap.h) against
xsknf_gpu_macswap_host on the same inputs (tests/test_macswap.py holds the host
model to the numpy model and to what the reference's function left): every
byte of the WHOLE UMEM buffer, so that a stray store shows, every verdict, the
sentinels past verdicts[n), the descriptors unchanged.  Sizes around the wave,
the block's tile and the grid's sweep, read from the code."""
import ctypes
import errno
import re

import numpy as np
import pytest

from tests import macswap_cases as MC
from tests import route_cases as RC
from xsknf_amd import _lib, frames, macswap, route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = MC.code_constant(r"constexpr int kThreads = (\d+);")        # kernel_macswap.h: frames per block and step
G = T * MC.code_constant(r"constexpr int kMaxBlocks = (\d+);")  # frames per sweep of the largest grid
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, G - 1, G, G + 1]
SENT = 0x5eadbeef


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def device_batch(dev, umem, descs, ingress=0, action=MC.REDIRECT, double=False, nif=1, du=None, n=None):
    """One xsknf_gpu_macswap_batch through the C ABI: (UMEM after, verdicts).
    The verdicts go into a sentinel-filled buffer of n + 64 words; the words
    past n must keep the sentinel and the descriptors their bytes."""
    n = descs.shape[0] if n is None else n
    du = _to_dev(umem, dev) if du is None else du
    dd = _to_dev(descs, dev)
    dv = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        macswap.macswap_batch_ptr(du.data_ptr() if n else 0, umem.size, dd.data_ptr() if n else 0, n, ingress,
                                  dv.data_ptr(), torch.cuda.current_stream(dev).cuda_stream, action=action,
                                  double_macswap=double, num_interfaces=nif)
    out = dv.cpu().numpy()
    assert (out[n:] == SENT).all(), "verdicts written past n"
    assert np.array_equal(dd.cpu().numpy(), np.ascontiguousarray(descs).view(np.uint8)), "descriptors written"
    return du.cpu().numpy(), out[:n]


def check(dev, umem, descs, ingress=0, action=MC.REDIRECT, double=False, nif=1, what=""):
    """Device == host on every UMEM byte and every verdict; returns the host's."""
    hu, hv = macswap.macswap_host(umem, descs, ingress, action=action, double_macswap=double, num_interfaces=nif)
    gu, gv = device_batch(dev, umem, descs, ingress, action, double, nif)
    bad = np.nonzero(gv != hv)[0]
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {gv[bad[:8]]} != {hv[bad[:8]]}"
    bad = np.nonzero(gu != hu)[0]
    assert bad.size == 0, f"{what}: {bad.size} UMEM bytes differ, first at {bad[:8]}"
    return hu, hv


def test_sizes_are_read_from_the_code():
    src = open(MC.ROOT + "/xsknf_amd/csrc/kernel_macswap.h").read()
    assert re.search(r"__launch_bounds__\(kThreads\)", src) and re.search(r"stride = gridDim\.x \* kThreads", src)
    dsrc = open(MC.ROOT + "/xsknf_amd/csrc/macswap_device.hip").read()
    assert re.search(r"tiles < static_cast<uint32_t>\(macswap::kMaxBlocks\) \? tiles : macswap::kMaxBlocks", dsrc)
    assert T % 64 == 0 and G > T


@pytest.mark.parametrize("base", [0, 1, 2, 3])
def test_tight_packing(dev, base):
    """4,096 frames of 14 bytes back to back from byte `base` on: the last
    swapped byte of a frame and the first of the next share an aligned word (a
    lane that stored whole words would race with its neighbour's).  The same
    with lengths cycling 14, 15, 17, 13: untouched short frames between swapped
    ones, every alignment in turn."""
    rng = np.random.default_rng(40 + base)
    u, d = MC.packed(rng, 4096, base)
    hu, hv = check(dev, u, d, what=f"14-byte frames from {base}")
    assert (hv == 0).all() and np.array_equal(hu[:base], u[:base])
    u, d = MC.packed(rng, 4096, base, lens=(14, 15, 17, 13), tail=base)
    hu, hv = check(dev, u, d, ingress=1, nif=3, what=f"cycling lengths from {base}")
    assert hv[:4].tolist() == [2, 2, 2, -1]
    # the descriptors in another order: neighbours in memory in different waves
    p = rng.permutation(4096)
    check(dev, u, d[p], ingress=1, nif=3, what=f"cycling lengths from {base}, permuted")


def test_every_phase_of_a_line(dev):
    """For every off % 128 a frame of 14 and one of 60 bytes with random canary
    bytes around: the 12 bytes straddle 4-, 16-, 64- and 128-byte boundaries in
    every way; in both address forms."""
    rng = np.random.default_rng(45)
    u, d = MC.phase_sweep(rng)
    assert sorted(set((MC.offsets(d) % 128).tolist())) == list(range(128))
    hu, hv = check(dev, u, d, ingress=2, action=MC.PASS, nif=4, what="phases")
    assert (hv == 3).all() and np.count_nonzero(hu != u) > 11 * d.shape[0]
    check(dev, u, MC.unaligned_form(d, rng), what="phases, base | off << 48")


def test_bounds_and_canaries(dev):
    """The UMEM is a 16-byte aligned slice inside a larger tensor with canaries
    on both sides; frames at offset 0 and in the last 14 bytes; descriptors
    outside the UMEM in each way rule 0 names.  The canaries, verdicts[n..) and
    the descriptors stay as they were."""
    rng = np.random.default_rng(46)
    for size in (4096 + 13, 4096, 14):
        u, d = MC.bounds_case(rng, size) if size > 14 else (rng.integers(0, 256, 14, dtype=np.uint8),
                                                            np.concatenate([MC.descs_of([0], [14]), MC.outside_descs(14)]))
        hu, hv = macswap.macswap_host(u, d, 0, num_interfaces=2)
        assert hv[hv >= 0].size >= 1 and not np.array_equal(hu[-14:], u[-14:]) and not np.array_equal(hu[:14], u[:14])
        pad = 4096
        big = rng.integers(0, 256, pad + size + pad, dtype=np.uint8)
        big[pad:pad + size] = u
        dbig = _to_dev(big, dev)
        assert dbig.data_ptr() % 16 == 0
        gu, gv = device_batch(dev, u, d, 0, nif=2, du=dbig[pad:pad + size])
        assert np.array_equal(gv, hv), size
        whole = dbig.cpu().numpy()
        assert np.array_equal(whole[pad:pad + size], hu), size
        assert np.array_equal(whole[:pad], big[:pad]) and np.array_equal(whole[pad + size:], big[pad + size:]), size


@pytest.fixture(scope="module")
def big():
    """G + 1 packed 64-byte frames with the host's result for each n of SIZES
    worked out from one run: frame i's bytes depend on n only through i < n."""
    rng = np.random.default_rng(47)
    u, d = MC.uniform(rng, G + 1, 64)
    hu, hv = macswap.macswap_host(u, d, 0, num_interfaces=2)
    for a in (u, d, hu, hv):
        a.setflags(write=False)
    return u, d, hu, hv


def test_batch_sizes_around_the_launch_edges(dev, big):
    """n = 0, 1, around the wave, the tile +- 1 and one full sweep of the
    largest grid - 1, + 0, + 1 (the second trip of the kernel's loop): frames
    past n are untouched."""
    u, d, hu, hv = big
    assert (hv == 1).all()
    for n in SIZES:
        du = _to_dev(u, dev)
        gu, gv = device_batch(dev, u, d, 0, nif=2, du=du, n=n)
        assert np.array_equal(gv, hv[:n]), f"n={n}"
        assert np.array_equal(gu[:64 * n], hu[:64 * n]), f"n={n}: frames"
        assert np.array_equal(gu[64 * n:], u[64 * n:]), f"n={n}: bytes past the batch"
        del du
    # the tensor form, on a stream of its own, in place
    du, dd = _to_dev(u[:64 * (T + 9)], dev), _to_dev(d[:T + 9], dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        v = macswap.macswap_batch(du, dd.view(torch.int64).reshape(-1, 2), 0, num_interfaces=2)
    s.synchronize()
    assert v.dtype == torch.int32 and np.array_equal(v.cpu().numpy(), hv[:T + 9])
    assert np.array_equal(du.cpu().numpy(), hu[:64 * (T + 9)])
    assert macswap.macswap_batch(du, dd[:0]).numel() == 0
    with pytest.raises(ValueError):
        macswap.macswap_batch(du.cpu(), dd)


def test_every_option(dev):
    """Every action x both swap modes x 1, 2, 3 and 0xffffffff interfaces (any
    nonzero count is accepted) x ingress 0, 1, nif - 1, 0xffffffff on 257 mixed
    frames; zero interfaces succeeds with DROP and is -EINVAL otherwise."""
    rng = np.random.default_rng(48)
    u, d = MC.mixed(rng)
    seen = set()
    for action in MC.ACTIONS:
        for double in (False, True):
            for nif in (1, 2, 3, 0xffffffff):
                for ingress in sorted({0, 1, nif - 1, 0xffffffff}):
                    hu, hv = check(dev, u, d, ingress, action, double, nif, what=f"{action} {double} {nif} {ingress:#x}")
                    assert np.array_equal(hu, u) == double
                    assert set(hv.tolist()) == {-1, MC.verdict(action, ingress, nif)}
                    seen.add(MC.verdict(action, ingress, nif))
    assert {-1, 0, 1, 2} <= seen
    hu, hv = check(dev, u, d, 0xfffffffd, MC.PASS, False, 0xffffffff, what="a verdict past 2^31")
    assert set(hv.tolist()) == {-1, -2}   # 0xfffffffe as an int32
    for double in (False, True):
        hu, hv = check(dev, u, d, 5, MC.DROP, double, 0, what="DROP, no interface")
        assert (hv == -1).all()
        for action in (MC.REDIRECT, MC.PASS):
            du = _to_dev(u, dev)
            with pytest.raises(_lib.XsknfGpuError):
                device_batch(dev, u, d, 0, action, double, 0, du=du)
            assert np.array_equal(du.cpu().numpy(), u)


def test_fixture_through_the_c_abi(dev):
    """tests/golden/macswap_golden.npz: what the reference's function left, from
    the device."""
    g = np.load(MC.GOLDEN)
    for b in range(int(g["batches"])):
        ingress, action, double, nif = (int(x) for x in g[f"params{b}"])
        gu, gv = device_batch(dev, g[f"umem{b}"], g[f"descs{b}"], ingress, action, bool(double), nif)
        assert np.array_equal(gv, g[f"verdicts{b}"]), b
        assert np.array_equal(gu, g[f"after{b}"]), b


def test_macswap_route_forward_chain(dev):
    """257 mixed frames, 2 interfaces, interface 1 with a UMEM of its own:
    macswap_batch -> route_batch (counts NULL) -> forward_frames enqueued on one
    stream with no host read between, against macswap_host -> route_host ->
    forward_host: every list entry and every byte of both UMEMs."""
    rng = np.random.default_rng(49)
    umem, descs = MC.mixed(rng)
    n, nif = descs.shape[0], 2
    hu, hv = macswap.macswap_host(umem, descs, 0, num_interfaces=nif)
    assert set(hv.tolist()) == {-1, 1}
    htx, hfill, hod, hcounts = RC.host_route_raw(descs, hv, nif)
    hdst = [None, ~umem]
    hstats = route.forward_host(hu, hdst, htx, hcounts)
    assert hstats[0] == hcounts[1] > 0

    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    ddst = [None, _to_dev(~umem, dev)]
    tx = torch.full((n * 16,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    fill = torch.full((n * 8,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    od = torch.full((n * 4,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
    ws = torch.empty(route.route_workspace(n, nif), dtype=torch.uint8, device=dev)
    stats = torch.zeros(route.FORWARD_STATS, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        v = macswap.macswap_batch(du, dd, 0, num_interfaces=nif)
        assert route.route_batch_ptr(dd.data_ptr(), v.data_ptr(), n, nif, tx.data_ptr(), fill.data_ptr(),
                                     od.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream,
                                     sync=False) is None
        assert route.forward_frames_ptr(du.data_ptr(), du.numel(), [0, ddst[1].data_ptr()], [0, ddst[1].numel()],
                                        tx.data_ptr(), ws.data_ptr(), n, stats.data_ptr(), stream.cuda_stream,
                                        sync=False) is None
    stream.synchronize()
    assert np.array_equal(v.cpu().numpy(), hv)
    counts = [int(c) for c in ws[:8 * (nif + 1)].cpu().numpy().view(np.uint64)]
    ntx, ndrop = sum(hcounts[:nif]), hcounts[nif]
    RC.same_as((tx.cpu().numpy().view(frames.DESC_DTYPE), fill.cpu().numpy().view(np.uint64),
                od.cpu().numpy().view(np.uint32), counts), (htx[:ntx], hfill[:ndrop], hod, hcounts), n, "chain")
    assert np.array_equal(du.cpu().numpy(), hu), "the rx UMEM"
    assert np.array_equal(ddst[1].cpu().numpy(), hdst[1]) and not np.array_equal(hdst[1], ~umem), "interface 1's UMEM"
    assert [int(x) for x in stats.cpu().numpy()] == hstats


def test_misaligned_pointers_write_nothing(dev):
    """A umem or descs off a 16-byte boundary or verdicts off a 4-byte one:
    -EINVAL before any launch, with every buffer as it was."""
    rng = np.random.default_rng(50)
    u, d = MC.packed(rng, 300, 0, tail=64)
    n = d.shape[0]
    du, dd = _to_dev(u, dev), _to_dev(np.concatenate([d, d[:1]]), dev)
    dv = torch.full((n + 8,), SENT, dtype=torch.int32, device=dev)
    o = _lib.MacswapOpts(MC.REDIRECT, 0, 2, 0)
    f = _lib.load().xsknf_gpu_macswap_batch
    s = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        for up, dp, vp in ((du.data_ptr() + 1, dd.data_ptr(), dv.data_ptr()),
                           (du.data_ptr() + 4, dd.data_ptr(), dv.data_ptr()),
                           (du.data_ptr() + 8, dd.data_ptr(), dv.data_ptr()),
                           (du.data_ptr(), dd.data_ptr() + 8, dv.data_ptr()),
                           (du.data_ptr(), dd.data_ptr() + 4, dv.data_ptr()),
                           (du.data_ptr(), dd.data_ptr(), dv.data_ptr() + 1),
                           (du.data_ptr(), dd.data_ptr(), dv.data_ptr() + 2)):
            assert f(up, u.size - 16, dp, n, 0, ctypes.byref(o), vp, s) == -errno.EINVAL
        torch.cuda.synchronize(dev)
        assert np.array_equal(du.cpu().numpy(), u) and (dv.cpu().numpy() == SENT).all()
        # a 4-byte aligned verdict array that is not 16-byte aligned is fine
        assert f(du.data_ptr(), u.size, dd.data_ptr(), n, 0, ctypes.byref(o), dv.data_ptr() + 4, s) == 0
    out = dv.cpu().numpy()
    hu, hv = macswap.macswap_host(u, d, 0, num_interfaces=2)
    assert out[0] == SENT and np.array_equal(out[1:n + 1], hv) and (out[n + 1:] == SENT).all()
    assert np.array_equal(du.cpu().numpy(), hu)
