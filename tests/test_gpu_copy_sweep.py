"""The directed sweeps through the kernels that move frames around the checksum
pass: forward_frames (kernel_forward.h), pack_frames / apply_records /
shard_counters (multi.hip, with the device planner in front of them) and
scatter_checks (kernel_scatter.h, store modes 0 and 2).  The batches are those
of tests/sweep_cases.py -- every frame length at every start phase, the header
and fold sweeps -- and tests/copy_cases.py's tile sweep (the edges of a wave's
round robin over a 64-entry tile); tests/test_copy_sweep.py holds, on the CPU,
what they contain and the host functions these cases compare against.

Every comparison is bit-exact over every byte: the forward's destinations start
as the complement of the rx UMEM, a packed shard is compared slot by slot with
the UMEM, the results with the oracle's pass over the whole batch.  Each case is
one small batch; the module shares one MultiDevice and the cached batches.
"""
import ctypes

import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import copy_cases as C
from tests import forward_cases as FC
from tests import route_cases as RC
from tests import sweep_cases as S
from xsknf_amd import ChecksummerOptions, _lib, frames, multi, route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import test_gpu_sweep as GS  # noqa: E402
from tests.test_gpu_forward import DevForward  # noqa: E402
from tests.test_gpu_parity import PRODUCT_SHAPES, _pool_guard_never_trips, _results, launch_cfg  # noqa: E402,F401
from tests.test_gpu_plan_dev import _same_shards, _shards, _to_dev  # noqa: E402

SEED = GS.SEED
NIF, INGRESS = GS.NIF, GS.INGRESS
LANE, SPLIT = ("length", C.LANE_BOUNDS), ("length", C.SPLIT_BOUNDS)


def _kid(key):
    return key if isinstance(key, str) else key[0] + "-" + "-".join(map(str, key[1]))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def md(dev):
    with multi.MultiDevice(range(torch.cuda.device_count())) as m:
        yield m


# ---- cached batches and their oracle results ------------------------------------

_batches, _oracle, _fwd = {}, {}, {}
OWN = ("tile", "hnic", "lane-cut")


def _batch(key):
    """GS._batch's keys, and: "tile" (C.tile_sweep), "lane-cut" (the lane length
    sweep, its UMEM cut to its first and last frame), "hnic" -- the header sweep
    with every check in place: after one pass of the oracle a second pass finds
    the check it computes, except in the frames whose UDP header overlaps the IP
    addresses (ihl 2 and 3), which change again; and the frames whose
    check straddles two 64-byte sectors keep their first bytes, so that the
    sparse pass meets that choice of rewrite_check too."""
    if key not in OWN:
        return GS._batch(key)
    if key not in _batches:
        if key == "tile":
            b = C.tile_sweep(SEED + 3)
        elif key == "lane-cut":
            whole = GS._batch(LANE)
            off = whole.frame_offsets().astype(np.int64)
            lo, hi = int(off.min()), int((off + whole.descs["len"]).max())
            d = whole.descs.copy()
            d["addr"] = (off - lo).astype(np.uint64)          # (aligned-mode addresses: plain offsets)
            b = frames.HostBatch(whole.umem[lo:hi].copy(), d, "aligned")
        else:
            fresh, at, _, _ = GS._case("header", 1)
            b = fresh.copy()
            O.c_process_batch(b.umem, b.descs, ingress=INGRESS, iters=1, action=O.REDIRECT, nif=NIF)
            changed = C.changed_frames(fresh, at)
            again = np.flatnonzero(changed)[C.scatter_masks(fresh, changed)[0]]
            start, ln = fresh.frame_offsets().astype(np.int64), fresh.descs["len"].astype(np.int64)
            for i in again:
                b.umem[start[i]:start[i] + ln[i]] = fresh.umem[start[i]:start[i] + ln[i]]
        b.umem.setflags(write=False)
        _batches[key] = b
    return _batches[key]


def _case(key, iters):
    """(batch, positions and values of the bytes the oracle changes, its verdicts)."""
    if key not in OWN:
        return GS._case(key, iters)
    b = _batch(key)
    if (key, iters) not in _oracle:
        r = b.copy()
        ov = C.oracle_pass(O.c_process_batch, r.umem, r.descs, ingress=INGRESS, iters=iters, action=O.REDIRECT,
                           nif=NIF)
        at = np.flatnonzero(r.umem != b.umem)
        _oracle[(key, iters)] = (at, r.umem[at].copy(), ov)
    return (b,) + _oracle[(key, iters)]


def _after(b, at, vals):
    u = b.umem.copy()
    u[at] = vals
    return u


def _opts(iters):
    return ChecksummerOptions(action=O.REDIRECT, csum_iterations=iters)


def _root_umem(dev, host, base_off=0):
    """The root's UMEM `base_off` bytes into a 256-byte aligned allocation."""
    big = torch.zeros(host.size + base_off + 64, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 256 == 0
    umem = big[base_off:base_off + host.size]
    umem.copy_(torch.from_numpy(host.copy()))
    torch.cuda.synchronize()
    return big, umem


# ---- the forward ----------------------------------------------------------------

def _forward_inputs(key):
    if key not in _fwd:
        _fwd[key] = C.forward_inputs(_batch(key))
    return _fwd[key]


def _forward_same(dev, key, how, cap=None):
    """Route + xsknf_gpu_forward_frames over the batch, destinations ~rx, against
    xsknf_gpu_forward_host and the numpy model over route_host's lists: every
    byte of every destination, the stats; rx UMEM, descriptors and lists unchanged."""
    what = f"{_kid(key)} {how} cap={cap}"
    rx, d = _forward_inputs(key)
    v, sizes = C.verdicts(_batch(key), how)
    nif = len(sizes)
    fwd = DevForward(dev, rx, d, v, sizes, cap=cap, fill=C.complement(rx, sizes))
    got, stats = fwd.result()
    tx, _, _, full = route.route_host(d, v, nif)
    counts = full if cap is None else FC.clip_counts(full, nif, cap)
    txa = FC.aligned_descs(tx.shape[0])
    txa[:] = tx
    want = C.complement(rx, sizes)
    wstats = route.forward_host(rx, want, txa, counts)
    model, mstats = FC.model_flat(rx, sizes, txa, counts, init=C.complement(rx, sizes))
    assert stats == wstats == mstats, what
    FC.same_umems(got, model, what + " (model)")
    FC.same_umems(got, want, what + " (forward_host)")
    assert np.array_equal(fwd.rx.cpu().numpy(), rx), f"{what}: the rx UMEM changed"
    assert np.array_equal(fwd.dd.cpu().numpy().view(frames.DESC_DTYPE), d), f"{what}: the descriptors changed"
    ntx = sum(full[:nif])
    assert np.array_equal(fwd.tx.cpu().numpy()[:16 * ntx].view(frames.DESC_DTYPE), tx[:ntx]), what
    assert np.all(fwd.tx.cpu().numpy()[16 * ntx:] == RC.SENTINEL8), what
    return stats, counts, got


FORWARD = [(LANE, "one"), (LANE, "three"), (SPLIT, "one"), (SPLIT, "three"), ("tile", "one"), ("tile", "three"),
           ("tile", "ranges")]


@pytest.mark.parametrize("key,how", FORWARD, ids=[f"{_kid(k)}-{h}" for k, h in FORWARD])
def test_forward_sweeps(dev, key, how):
    """Every length 0..128 at every start phase (all 136 windows of a one-chunk
    frame through copy_edge, every phase pair at 2..9 chunks), frames past one
    round of 64 chunks, and the tile sweep's edges of the lane's resumed search:
    to one interface (the tx list is the batch, tile for tile), dealt to three
    (own UMEM, shared, own and smaller: neighbours land in different UMEMs), and
    in three runs with the interface boundaries mid-tile."""
    stats, counts, _ = _forward_same(dev, key, how)
    assert stats[0] > 0
    if how == "one":
        assert stats[0] + stats[2] == _batch(key).n
    if how == "three":
        assert stats[2] > 0
    if how == "ranges":
        assert counts[0] % 64 and (counts[0] + counts[1]) % 64


def test_forward_capacity_cuts_a_tile_of_the_tile_sweep(dev):
    """The capacity ends inside the first edge tile, between the frame that ends
    in chunk R - 1 and the one that starts in chunk R: the entries behind it
    keep ~rx."""
    b = _batch("tile")
    cap = 11 * 64 + 22
    off, ln, inr, nch = C.chunks(b.descs, b.umem.size)
    R = C.constants()[0]
    assert nch[11 * 64:cap].sum() == R and nch[cap] > 0 and nch[cap - 1] > 0
    stats, _, got = _forward_same(dev, "tile", "one", cap=cap)
    assert stats[0] + stats[2] == cap
    rx, _ = _forward_inputs("tile")
    later = np.flatnonzero(nch[cap:] > 0) + cap
    inv = ~rx
    first = later[0]                                         # (it shares a chunk with the last copied frame)
    assert first == cap and np.array_equal(got[0][off[first]:], inv[off[first]:])


# ---- the packed round trip ------------------------------------------------------

def _packed_round_trip(md, dev, key, iters, base_off=0):
    b, at, vals, ov = _case(key, iters)
    host, hd, n = b.umem, b.descs, b.n
    ndev = torch.cuda.device_count()
    big, umem = _root_umem(dev, host, base_off)
    v = torch.full((n,), 0x7eadbeef, dtype=torch.int32, device=dev)
    md.scatter_packed(0, umem.data_ptr(), host.size, hd)
    ranges, _ = multi.shard_plan(hd, ndev, host.size)
    wd, wsizes = multi.pack_plan(hd, [0] + [hi for _, hi in ranges], umem.data_ptr(), host.size)
    for k in range(ndev):
        info = md.shard_info(k)
        su, _, sd = md.fetch(k, descs=True)
        lo, hi = info["frame_lo"], info["frame_hi"]
        assert (lo, hi) == ranges[k] and info["flags"] == _lib.SHARD_PACKED
        assert (info["span_lo"], info["span_hi"]) == (0, wsizes[k]) and su.size == wsizes[k]
        for f in ("addr", "len", "options"):
            assert np.array_equal(sd[f], wd[f][lo:hi]), f"shard {k} descriptors: {f}"
        # every frame's packed bytes: its whole 16-byte chunks, as far as they lie inside the UMEM
        dst, src = C.slot_bytes(hd[lo:hi], sd["addr"], umem.data_ptr(), host.size)
        bad = np.flatnonzero(su[dst] != host[src])
        assert bad.size == 0, f"shard {k}: {bad.size} packed bytes differ, first from UMEM offsets {src[bad[:8]]}"
    md.return_results(umem.data_ptr(), v.data_ptr(), _opts(iters), num_interfaces=NIF, ingress_ifindex=INGRESS,
                      frame_len_max=int(hd["len"].max()))
    gv, gu = _results(v, umem)
    GS._same(b, at, vals, ov, gu, gv, f"{_kid(key)} iters {iters}")
    assert np.all(big.cpu().numpy()[:base_off] == 0) and np.all(big.cpu().numpy()[base_off + host.size:] == 0)


PACKED = [(k, it) for k in (LANE, SPLIT, "tile", "header") for it in (1, 2)] + [("fold", it) for it in S.FOLD_ITERS]


@pytest.mark.parametrize("key,iters", PACKED, ids=[f"{_kid(k)}-i{it}" for k, it in PACKED])
def test_packed_round_trip_sweeps(md, dev, key, iters):
    """scatter_packed -> return_results: before the return every byte pack_frames
    moved, of every frame, equals the UMEM's (vectorised, not sampled) and the
    descriptors equal the host plan's; afterwards the root's UMEM and verdicts
    equal the oracle's pass over the whole batch (apply_records on every record
    of the sweep; two iterations change every check)."""
    _packed_round_trip(md, dev, key, iters)


def test_packed_round_trip_umem_7_bytes_into_its_allocation(md, dev):
    """pack_frames' byte-by-byte branch: with the base 7 mod 16 every swept
    (length, phase) moves to another address phase, and the first and the last
    frame's chunks reach outside the UMEM (the batch is cut to its frames: the
    first starts on the UMEM's first byte, the last ends on its last)."""
    b = _batch("lane-cut")
    off, ln, _, _ = C.chunks(b.descs, b.umem.size)
    assert off.min() == 0 and (off + ln).max() == b.umem.size and (b.umem.size + 7) % 16
    _packed_round_trip(md, dev, "lane-cut", 1, base_off=7)


# ---- the plan made on the device ------------------------------------------------

PLANNED = [(k, p) for k in (LANE, SPLIT, "tile", "header", "fold") for p in (True, False)]


@pytest.mark.parametrize("key,packed", PLANNED, ids=[f"{_kid(k)}-{'packed' if p else 'span'}" for k, p in PLANNED])
def test_scatter_dev_equals_the_host_scatter(md, dev, key, packed):
    """plan_pack -> pack_frames (and the span plan) from descriptors on the
    device: shard info, bytes and descriptors equal the host scatter's."""
    b = _batch(key)
    ndev = torch.cuda.device_count()
    big, umem = _root_umem(dev, b.umem)
    (md.scatter_packed if packed else md.scatter)(0, umem.data_ptr(), b.umem.size, b.descs)
    want = _shards(md, ndev)
    dd = _to_dev(b.descs, dev)
    md.scatter_dev(0, umem.data_ptr(), b.umem.size, dd.data_ptr(), b.n, packed=packed)
    dd.zero_()
    torch.cuda.synchronize()
    _same_shards(_shards(md, ndev), want)
    assert sum(w[1].size for w in want) > 0


# ---- the span path and the counters ---------------------------------------------

@pytest.mark.parametrize("key", ["header", LANE, "tile"], ids=_kid)
def test_span_path_and_counters(md, dev, key):
    """scatter -> process -> counters: shard_counters' `len >= 42` at lengths 41,
    42 and 43 at every phase, a frame ending on the span's last byte, descriptors
    outside the UMEM; against the counters model over the oracle's result, and
    every shard's bytes and verdicts against the oracle."""
    b, at, vals, ov = _case(key, 1)
    ref = _after(b, at, vals)
    ndev = torch.cuda.device_count()
    big, umem = _root_umem(dev, b.umem)
    md.scatter(0, umem.data_ptr(), b.umem.size, b.descs)
    md.process(_opts(1), num_interfaces=NIF, ingress_ifindex=INGRESS, frame_len_max=int(b.descs["len"].max()))
    cnt = md.counters()
    shards = [(md.shard_info(k),) + md.fetch(k) for k in range(ndev)]
    want = C.counters_model(ref, b.descs, ov)
    assert want == multi.expected_counters(ref, b.descs, ov)
    assert cnt == want
    assert want["checks_sum"] > 0 and want["drop"] > 0 and want["forward"] > 0
    off, ln, inr, _ = C.chunks(b.descs, b.umem.size)
    for info, su, sv in shards:
        lo, hi = info["frame_lo"], info["frame_hi"]
        assert np.array_equal(sv, ov[lo:hi]), "verdicts"
        assert np.array_equal(su, ref[info["span_lo"]:info["span_hi"]]), "bytes"
        if hi > lo and inr[lo:hi].any():
            assert info["span_hi"] == int((off + ln)[lo:hi][inr[lo:hi]].max())      # a frame ends on the span's last byte
    assert np.array_equal(umem.cpu().numpy(), b.umem)                                # the root's UMEM is only read


# ---- scatter_checks -------------------------------------------------------------

SCATTER_SHAPES = [s for s in PRODUCT_SHAPES if GS._selectable(s) and s[4] in (0, 2)]
SCATTER_CASES = [(s, k) for s in SCATTER_SHAPES for k in ("length", "nic", "header", "hnic")]


def test_the_scatter_shapes_are_the_selectable_ones():
    assert len(SCATTER_SHAPES) == 12 and {s[4] for s in SCATTER_SHAPES} == {0, 2}
    assert {S.family(s) for s in SCATTER_SHAPES} == {"lane", "split", "group"}


def _launch(b, dev, shape, iters):
    umem, descs = GS._to_device(b, dev)
    assert umem.data_ptr() % 256 == 0          # rewrite_check's sector choice: as C.scatter_classes computes it (base 0 mod 64)
    v = torch.empty(b.n, dtype=torch.int32, device=dev)
    rc = _lib.load().xsknf_gpu_checksum_batch_cfg(
        ctypes.c_void_p(umem.data_ptr()), umem.numel(), ctypes.c_void_p(descs.data_ptr()), b.n, INGRESS,
        ctypes.byref(_lib.CsumOpts(iters, O.REDIRECT, NIF, 0)), ctypes.c_void_p(v.data_ptr()),
        ctypes.byref(launch_cfg(shape)), None)
    assert rc == 0
    return _results(v, umem)


@pytest.mark.parametrize("shape,kind", SCATTER_CASES, ids=[f"{GS._id(s)}-{k}" for s, k in SCATTER_CASES])
def test_scatter_checks_sweeps(dev, shape, kind):
    """Store modes 0 (per tile) and 2 (every check deferred) of every
    default-selectable shape over its own length sweep and the header sweep,
    fresh (dense: a record for every changed check) and with the checks already
    in place (sparse: few records), against the oracle: every byte and verdict.

    Mode 2 parks a record for exactly the frames whose check changes, so the
    record share is known from the oracle: at least 1/4 (scatter_dense) for the
    fresh batches, below 1/4 and above 0 (scatter_sparse) with the checks in
    place, and the changed frames hold every per-frame choice of rewrite_check.
    Mode 0 parks only frames of kDeferMinLen bytes or more (and, in the split
    and group kernels, only in tiles half full of them): these batches give it
    few or no records -- its in-line stores and the pass's early return are what
    run, and the comparison is the same."""
    key = {"length": ("length", S.boundaries(shape)), "nic": ("nic", S.boundaries(shape))}.get(kind, kind)
    b, at, vals, ov = _case(key, 1)
    changed = C.changed_frames(b, at)
    share = changed.sum() / b.n
    if shape[4] == 2:
        if kind in ("length", "header"):
            assert share >= 0.25, share
            cl = C.scatter_classes(b, changed)
            assert all(cl[k] > 0 for k in ("whole", "before", "past", "straddle")), cl
            if kind == "header":
                assert cl["straddle_inside"] > 0
        else:
            assert 0 < share < 0.25, share
            if kind == "hnic":
                cl = C.scatter_classes(b, changed)
                assert all(cl[k] > 0 for k in ("whole", "before", "past", "straddle_inside")), cl
    else:
        long_ = S.code_constant("csum_device.h", r"constexpr uint32_t kDeferMinLen = (\d+);")
        if S.family(shape) == "lane":          # (per frame there: kernel_lane.h) nothing is parked, the pass returns at once
            assert not (changed & (b.descs["len"] >= long_)).any()
    gv, gu = _launch(b, dev, shape, 1)
    GS._same(b, at, vals, ov, gu, gv, f"{GS._id(shape)} {kind}")
