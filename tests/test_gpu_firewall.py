"""The firewall NF on the device (include/xsknf_gpu.h xsknf_gpu_firewall_batch;
xsknf_amd/csrc/firewall_device.hip, kernel_firewall.h): the device's verdicts
against xsknf_gpu_firewall_host's on every frame (tests/test_firewall.py holds
the host model to the dict model and to the reference function's recorded
verdicts), the UMEM byte-identical after every call, nothing written past the
n verdicts.  Sizes around the wave, the block's tile and the grid's sweep, read
from the code."""
import re

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import route_cases as RC
from xsknf_amd import _lib, firewall, frames, route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = FC.code_constant(r"constexpr int kThreads = (\d+);")        # frames per block and step
G = T * FC.code_constant(r"constexpr int kMaxBlocks = (\d+);")  # frames per sweep of the largest grid
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, G + 1, 2 * G + 323]
SENT = 0x5eadbeef


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def _device_verdicts(dev, du, umem_size, dd, n, acl):
    """One xsknf_gpu_firewall_batch through the C ABI into a sentinel-filled
    buffer of n + 64 words; the words past n must keep the sentinel."""
    dv = torch.full((n + 64,), SENT, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        firewall.firewall_batch_ptr(du.data_ptr() if n else 0, umem_size, dd.data_ptr() if n else 0, n, acl,
                                    dv.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    out = dv.cpu().numpy()
    assert (out[n:] == SENT).all(), "verdicts written past n"
    return out[:n]


def _check(dev, umem, descs, rules, slots=0, what=""):
    """Device == host model on every frame; the UMEM untouched; returns the verdicts."""
    with firewall.Acl.from_rules(rules, slots) as acl:
        assert acl.info["device_bytes"] == 20 * acl.info["slots"]
        want = firewall.firewall_host(umem, descs, acl)
        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        got = _device_verdicts(dev, du, umem.size, dd, descs.shape[0], acl)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"
        assert np.array_equal(du.cpu().numpy(), umem), f"{what}: the UMEM was written"
        assert np.array_equal(dd.cpu().numpy(), np.ascontiguousarray(descs).view(np.uint8)), what
    return want


def test_sizes_are_read_from_the_code():
    src = open(FC.ROOT + "/xsknf_amd/csrc/kernel_firewall.h").read()
    assert re.search(r"__launch_bounds__\(kThreads\)", src) and re.search(r"stride = gridDim\.x \* kThreads", src)
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/firewall_device.hip").read()
    assert re.search(r"tiles < static_cast<uint32_t>\(firewall::kMaxBlocks\) \? tiles : firewall::kMaxBlocks", dsrc)
    assert T % 64 == 0 and G > T


def test_decision_sweep_every_phase(dev):
    """ihl 0..15 x protocol {6, 17, 1} x IPv4 / not x the 12 lengths around each
    rule's edge x all 16 start phases, back to back with random gaps in the
    base | off << 48 layout, the last frame ending on the UMEM's last byte,
    descriptors outside the UMEM directly before and after in-range ones; the
    ACL holds a third of the lookups' keys (every action), only the one-bit
    neighbours of another third, and nothing of the rest."""
    rng = np.random.default_rng(21)
    fl, ph = FC.decision_frames(rng)
    assert len(fl) == 16 * 3 * 2 * 12 * 16
    umem, descs = FC.pack_unaligned(fl, rng, ph)
    last = descs[-1]
    assert (int(last["addr"]) & ((1 << 48) - 1)) + (int(last["addr"]) >> 48) + int(last["len"]) == umem.size
    rules = FC.hit_miss_acl(FC.keys_of(umem, descs), rng)
    descs = FC.with_outside(umem, descs, rng)
    want = _check(dev, umem, descs, rules, what="unaligned")
    assert set(FC.ACTIONS) <= set(want.tolist())
    assert np.array_equal(want[::997], FC.model(umem, descs[::997], FC.acl_dict(rules)))


def test_decision_sweep_aligned_chunks(dev):
    """The aligned 2 KiB layout: one frame per chunk at a random headroom."""
    rng = np.random.default_rng(22)
    fl, _ = FC.decision_frames(rng, phases=(0,))
    umem, descs = FC.pack_aligned(fl, rng)
    rules = FC.hit_miss_acl(FC.keys_of(umem, descs), rng)
    want = _check(dev, umem, FC.with_outside(umem, descs, rng), rules, what="aligned")
    assert set(FC.ACTIONS) <= set(want.tolist())


def test_hits_and_near_misses(dev):
    """3,000 lookups of mixed ihl: exact keys with actions -1, 0, 1, 2, 31,
    0x7fffffff, -7 for a third; all 104 one-bit neighbours of the key but not
    the key for another third (-> 0); the rest absent."""
    rng = np.random.default_rng(23)
    fl = FC.lookup_frames(rng, 3000)
    umem, descs = FC.pack_unaligned(fl, rng)
    keys = FC.keys_of(umem, descs)
    assert all(k is not None for k in keys)
    rules = FC.hit_miss_acl(keys, rng)
    assert rules.shape[0] == 1000 + 1000 * 104
    want = _check(dev, umem, descs, rules, what="hits and near misses")
    assert np.array_equal(want[0::3], np.resize(np.array(FC.ACTIONS, dtype=np.int64), 1000).astype(np.int32))
    assert not want[1::3].any() and not want[2::3].any()


def test_full_table_and_tiny_acls(dev):
    """slots = 1024 with 1023 distinct rules: every cluster wraps past the last
    slot and a miss probes to the single empty slot; 1023 hits and 1023 misses.
    And ACLs of 0 and 1 rules."""
    rules, umem, descs = FC.full_table_case()
    want = _check(dev, umem, descs, rules, slots=1024, what="full table")
    assert np.array_equal(want[:1023], rules["action"]) and not want[1023:].any()
    assert not _check(dev, umem, descs, rules[:0], what="empty ACL").any()
    one = _check(dev, umem, descs, rules[5:6], what="one rule")
    assert np.flatnonzero(one).tolist() == ([5] if rules["action"][5] else [])
    _check(dev, umem, descs, rules[5:6], slots=2, what="one rule, two slots")


@pytest.fixture(scope="module")
def big():
    """2 G + 323 packed 64-byte frames over a 50,000-rule ACL: half carry a rule's
    key, half a key one bit off; every fifth descriptor has a random length
    0..64, so every way out of the parse occurs.  Shared, never written."""
    rng = np.random.default_rng(24)
    n = SIZES[-1]
    rules = FC.random_rules(rng, 50000)
    pick = rng.integers(0, rules.shape[0], n)
    umem, descs = FC.frames_for_rules(rules[pick], rng)
    flip = np.flatnonzero(rng.integers(0, 2, n) == 1)
    umem.reshape(-1, 64)[flip, 26 + rng.integers(0, 8, flip.size)] ^= 1
    descs["len"][::5] = rng.integers(0, 65, descs[::5].shape[0])
    acl = firewall.Acl.from_rules(rules)
    want = firewall.firewall_host(umem, descs, acl)
    for a in (umem, descs, want):
        a.setflags(write=False)
    yield umem, descs, acl, want
    acl.close()


def test_batch_sizes_around_the_loop_edges(dev, big):
    """n = 0, 1, around the wave, the tile +- 1, and past one and two sweeps of
    the largest grid (the second and third trips of the kernel's loop, the last
    partial and no multiple of 64)."""
    umem, descs, acl, want = big
    assert {-1, 0, 5}.issubset(set(want[:4096].tolist()))
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    for n in SIZES:
        got = _device_verdicts(dev, du, umem.size, dd, n, acl)
        bad = np.nonzero(got != want[:n])[0]
        assert bad.size == 0, f"n={n}: first differences at {bad[:8]}"
    assert np.array_equal(du.cpu().numpy(), umem)
    # the tensor form, on a stream of its own
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        v = firewall.firewall_batch(du, dd.view(torch.int64).reshape(-1, 2)[:T + 9], acl)
    s.synchronize()
    assert v.dtype == torch.int32 and np.array_equal(v.cpu().numpy(), want[:T + 9])
    assert firewall.firewall_batch(du, dd[:0], acl).numel() == 0
    with pytest.raises(ValueError):
        firewall.firewall_batch(du.cpu(), dd, acl)


def test_fixture_through_the_c_abi(dev, tmp_path):
    """tests/golden/firewall_golden.npz: the reference function's recorded
    verdicts from the device, the ACL read from its text; the UMEM is only read
    and the pool guard stays at 0."""
    g = np.load(FC.GOLDEN)
    p = tmp_path / "acl.txt"
    p.write_bytes(g["acl_text"].tobytes())
    umem = g["umem"]
    descs = g["descs"].copy().view(frames.DESC_DTYPE).reshape(-1)
    du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
    with firewall.Acl.from_file(str(p)) as acl:
        got = _device_verdicts(dev, du, umem.size, dd, descs.shape[0], acl)
    assert np.array_equal(got, g["verdicts"])
    assert np.array_equal(du.cpu().numpy(), umem)
    with torch.cuda.device(dev):
        assert _lib.pool_guard_trips() == 0


def test_firewall_route_forward_chain(dev):
    """257 mixed frames, 3 interfaces, interfaces 1 and 2 with UMEMs of their
    own: firewall_batch -> route_batch (counts NULL) -> forward_frames enqueued
    on one stream with no host read between, against firewall_host ->
    route_host -> forward_host: every list entry and every destination byte."""
    rng = np.random.default_rng(25)
    fl = FC.lookup_frames(rng, 200) + [FC.make_frame(rng, int(rng.integers(0, 120)), int(rng.integers(16)),
                                                     int(rng.choice([6, 17, 1])), bool(rng.integers(4)))
                                       for _ in range(57)]
    fl = [fl[i] for i in rng.permutation(257)]
    umem, descs = FC.pack_unaligned(fl, rng, tail=5)
    keys = [k for k in FC.keys_of(umem, descs) if k is not None]
    acts = [(-1, 0, 1, 2, 31)[i % 5] for i in range(len(keys))]
    rules = FC.rules_from_keys(keys[::2], acts[::2])
    n, nif = 257, 3
    with firewall.Acl.from_rules(rules) as acl:
        hv = firewall.firewall_host(umem, descs, acl)
        assert all((hv == a).any() for a in (-1, 0, 1, 2, 31))
        htx, hfill, hod, hcounts = RC.host_route_raw(descs, hv, nif)
        hdst = [None, ~umem, ~umem]
        hstats = route.forward_host(umem, hdst, htx, hcounts)
        assert hstats[0] == hcounts[1] + hcounts[2] > 0

        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        ddst = [None, _to_dev(~umem, dev), _to_dev(~umem, dev)]
        tx = torch.full((n * 16,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        fill = torch.full((n * 8,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        od = torch.full((n * 4,), RC.SENTINEL8, dtype=torch.uint8, device=dev)
        ws = torch.empty(route.route_workspace(n, nif), dtype=torch.uint8, device=dev)
        stats = torch.zeros(route.FORWARD_STATS, dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            v = firewall.firewall_batch(du, dd, acl)
            assert route.route_batch_ptr(dd.data_ptr(), v.data_ptr(), n, nif, tx.data_ptr(), fill.data_ptr(),
                                         od.data_ptr(), ws.data_ptr(), ws.numel(), stream.cuda_stream,
                                         sync=False) is None
            assert route.forward_frames_ptr(du.data_ptr(), du.numel(), [0] + [t.data_ptr() for t in ddst[1:]],
                                            [0] + [t.numel() for t in ddst[1:]], tx.data_ptr(), ws.data_ptr(), n,
                                            stats.data_ptr(), stream.cuda_stream, sync=False) is None
        stream.synchronize()
        assert np.array_equal(v.cpu().numpy(), hv)
        counts = [int(c) for c in ws[:8 * (nif + 1)].cpu().numpy().view(np.uint64)]
        ntx, ndrop = sum(hcounts[:nif]), hcounts[nif]
        RC.same_as((tx.cpu().numpy().view(frames.DESC_DTYPE), fill.cpu().numpy().view(np.uint64),
                    od.cpu().numpy().view(np.uint32), counts), (htx[:ntx], hfill[:ndrop], hod, hcounts), n, "chain")
        for k in (1, 2):
            assert np.array_equal(ddst[k].cpu().numpy(), hdst[k]), f"interface {k}'s UMEM"
            assert not np.array_equal(hdst[k], ~umem)
        assert [int(x) for x in stats.cpu().numpy()] == hstats
        assert np.array_equal(du.cpu().numpy(), umem)


def test_a_million_rules_on_the_device(dev):
    """The 1,000,000-rule ACL (2^21 slots, 40 MiB on the device): 65,536 hits and
    65,536 near misses against the dict, once."""
    rules, umem, descs, want = FC.million_case()
    with firewall.Acl.from_rules(rules) as acl:
        assert acl.info["device_bytes"] == 20 << 21
        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        got = _device_verdicts(dev, du, umem.size, dd, descs.shape[0], acl)
    assert np.array_equal(got, want)
