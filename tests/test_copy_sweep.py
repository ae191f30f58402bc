"""The fixtures of tests/copy_cases.py on the CPU: that the reused length sweep and
the tile sweep hold what the copy kernels decide on (conditions counted from the
descriptors alone), and the host functions the GPU tests compare against --
xsknf_gpu_forward_host, the host planner's packed layout, the counters model --
against numpy restatements on these very batches; the oracle's pass over the
tile sweep is held to the reference's compiled function, as tests/test_sweep.py
does for the other sweeps.  tests/test_gpu_copy_sweep.py runs the kernels."""
import numpy as np
import pytest

from oracle import csum_oracle as O
from oracle import ref as R
from tests import copy_cases as C
from tests import forward_cases as FC
from tests import sweep_cases as S
from xsknf_amd import frames, multi, route
from xsknf_amd.shard import counters

SEED = 0x5357                     # the seeds of tests/test_sweep.py: the same batches
_cache = {}


def _batch(name):
    if name not in _cache:
        _cache[name] = {"lane": lambda: S.length_sweep(C.LANE_BOUNDS, SEED),
                        "split": lambda: S.length_sweep(C.SPLIT_BOUNDS, SEED),
                        "header": lambda: S.header_sweep(SEED + 1),
                        "tile": lambda: C.tile_sweep(SEED + 3)}[name]()
        _cache[name].umem.setflags(write=False)
    return _cache[name]


def _oracle(name, iters=1):
    """(the oracle's UMEM, its verdicts) under the GPU tests' options."""
    k = (name, iters)
    if k not in _cache:
        r = _batch(name).copy()
        v = C.oracle_pass(O.c_process_batch, r.umem, r.descs, ingress=1, iters=iters, action=O.REDIRECT, nif=3)
        _cache[k] = (r.umem, v)
    return _cache[k]


def test_rounds_and_trips_are_the_codes():
    assert C.constants() == (64, 256)
    assert S.boundaries((1, 5, 2, 0, 1, 0, 1024)) == C.LANE_BOUNDS
    assert S.boundaries((16, 2, 2, 0, 18, 1, 56)) == C.SPLIT_BOUNDS


def test_tile_sweep_holds_every_edge():
    b = _batch("tile")
    cov = C.tile_coverage(b)
    print({k: v for k, v in cov.items() if k != "totals"}, sorted(cov["totals"]))
    C.tile_coverage_holds(cov)
    in_order, max_gap, overlaps = S.packing(frames.HostBatch(b.umem, b.descs[C.chunks(b.descs, b.umem.size)[2]], ""))
    assert in_order and overlaps == 0 and max_gap <= 15                    # back to back
    # both zero-chunk kinds, both address forms
    off, ln, inr, nch = C.chunks(b.descs, b.umem.size)
    assert (~inr).sum() > 50 and (inr & (ln == 0)).sum() > 50
    assert (b.descs["addr"] >> np.uint64(48)).max() == 255


def test_a_thinned_tile_sweep_fails_its_conditions():
    """The conditions are not vacuous: without its last (partial) tile, without
    its first 11 (the totals), or with the out-of-range entries brought to
    length 0, the batch fails them."""
    b = _batch("tile")
    for thin in (b.descs[:b.n // 64 * 64], b.descs[11 * 64:]):
        with pytest.raises(AssertionError):
            C.tile_coverage_holds(C.tile_coverage(frames.HostBatch(b.umem, thin, "")))
    d = b.descs.copy()
    gone = ~C.chunks(d, b.umem.size)[2]
    d["addr"][gone], d["len"][gone] = 0, 0
    with pytest.raises(AssertionError):
        C.tile_coverage_holds(C.tile_coverage(frames.HostBatch(b.umem, d, "")))


def test_length_sweep_holds_every_window_and_phase_pair():
    cov = C.copy_coverage(_batch("lane"))
    print(cov)
    assert cov["windows"] == 136                            # every [b0, b1) of a one-chunk frame
    assert all(cov["pairs"][n] == 256 for n in range(2, 10)), cov["pairs"]
    assert cov["shared"] > _batch("lane").n // 4            # neighbours share chunks
    cov = C.copy_coverage(_batch("split"))
    assert cov["windows"] == 136 and cov["pairs"][2] == cov["pairs"][3] == 256
    assert cov["max_nch"] > C.constants()[0]                # frames past one round of 64 chunks


# ---- xsknf_gpu_forward_host against the numpy model, destinations ~rx ------------

FORWARD = [("lane", "one"), ("lane", "three"), ("split", "three"), ("tile", "one"), ("tile", "three"),
           ("tile", "ranges")]


@pytest.mark.parametrize("name,how", FORWARD, ids=[f"{a}-{b}" for a, b in FORWARD])
def test_forward_host_equals_the_model(name, how):
    b = _batch(name)
    rx, d = C.forward_inputs(b)
    v, sizes = C.verdicts(b, how)
    tx, _, _, counts = route.route_host(d, v, len(sizes))
    txa = FC.aligned_descs(tx.shape[0])
    txa[:] = tx
    want, wstats = FC.model_flat(rx, sizes, txa, counts, init=C.complement(rx, sizes))
    got = C.complement(rx, sizes)
    stats = route.forward_host(rx, got, txa, counts)
    assert stats == wstats
    FC.same_umems(got, want, f"{name} {how}")
    assert stats[0] > 0 and stats[1] > 0
    if how == "three":
        assert stats[2] > 0                                  # the smaller UMEM's far frames
    if how == "ranges":
        assert counts[0] % 64 and (counts[0] + counts[1]) % 64       # the interface boundaries fall mid-tile
    if name == "tile" and how != "ranges":
        # (the definition, per entry) and untouched bytes really are ~rx
        slow, sstats = FC.model(rx, sizes, txa, counts, init=C.complement(rx, sizes))
        assert sstats == wstats
        FC.same_umems(want, slow, "model_flat")
        assert (want[0] == ~rx[:want[0].size]).any() and (want[0] == rx[:want[0].size]).any()


# ---- the host planner's packed layout -------------------------------------------

@pytest.mark.parametrize("shift", [0, 7])
@pytest.mark.parametrize("nshards", [1, 3])
@pytest.mark.parametrize("name", ["lane", "split", "tile"])
def test_packed_layout_equals_its_restatement(name, nshards, shift):
    b = _batch(name)
    addr0 = 0x7F5A12340000 + shift
    ranges, _ = multi.shard_plan(b.descs, nshards, b.umem.size)
    bounds = [0] + [hi for _, hi in ranges]
    got, sizes = multi.pack_plan(b.descs, bounds, addr0, b.umem.size)
    waddr, wsizes = C.packed_layout(b.descs, bounds, addr0, b.umem.size)
    assert sizes == wsizes
    assert np.array_equal(got["addr"], waddr)
    assert np.array_equal(got["len"], b.descs["len"]) and np.array_equal(got["options"], b.descs["options"])
    off, ln, inr, nch = C.chunks(b.descs, b.umem.size, addr0 & 15)
    assert np.array_equal((got["addr"][inr] & np.uint64(15)).astype(np.int64), (off[inr] + addr0) & 15)
    assert np.all(got["addr"][~inr] == np.uint64(1 << 47))
    assert (~inr).any() == (name == "tile")
    for lo, hi in ranges:                                    # every slot is exactly the frame's chunks
        a = got["addr"][lo:hi].astype(np.int64)[nch[lo:hi] > 0] & ~15
        assert np.array_equal(np.diff(a), 16 * nch[lo:hi][nch[lo:hi] > 0][:-1])
    # the bytes a packed shard must hold: every moved byte has one place, inside the shard
    dst, src = C.slot_bytes(b.descs[:bounds[1]], got["addr"][:bounds[1]], addr0, b.umem.size)
    assert np.unique(dst).size == dst.size and dst.min() >= 0 and dst.max() < sizes[0]
    assert src.min() >= 0 and src.max() < b.umem.size


# ---- the counters ----------------------------------------------------------------

def test_counters_model_on_the_header_sweep():
    b = _batch("header")
    start, ln, rs, _, _ = S.geometry(b)
    for length in (41, 42, 43):
        assert set(rs[ln == length]) == set(range(16))                    # the `len >= 42` edge at every phase
    ou, ov = _oracle("header")
    assert list(counters(ov, b.descs["len"])) == [b.n, int(ln.sum()), int((ov == -1).sum()), int((ov >= 0).sum())]
    want = multi.expected_counters(ou, b.descs, ov)
    cs = cw = 0
    for s, l in zip(start.tolist(), ln.tolist()):
        if l >= 42:
            ck = int(ou[s + 40]) | int(ou[s + 41]) << 8
            cs += ck
            cw += ck * (s % 65521 + 1)
    assert want == dict(frames=b.n, bytes=int(ln.sum()), drop=int((ov == -1).sum()), forward=int((ov >= 0).sum()),
                        checks_sum=cs, checks_weighted=cw & (1 << 64) - 1)
    assert (start + ln).max() == b.umem.size - 16                          # a frame ends on the span's last byte


# ---- scatter_checks' choices -----------------------------------------------------

def test_scatter_choices_all_occur():
    """Over the lane length sweep and the header sweep, UMEM base 64-byte
    aligned: whole-sector rewrites, 2-byte stores with the sector crossing the
    frame's start and its end, and checks that straddle two sectors."""
    tot = {}
    for name in ("lane", "header"):
        b = _batch(name)
        ou, _ = _oracle(name)
        cl = C.scatter_classes(b, C.changed_frames(b, np.flatnonzero(ou != b.umem)))
        print(name, cl)
        assert all(cl[k] > 0 for k in ("whole", "before", "past", "straddle")), (name, cl)
        tot[name] = cl
    # the straddle decides only where the sector lies inside the frame: u + 6 >= 63, the header sweep's long ihl
    assert tot["lane"]["straddle_inside"] == 0 and tot["header"]["straddle_inside"] > 0
    # another base mod 64 moves every choice: the GPU test asserts the base it runs at
    assert C.scatter_classes(_batch("lane"), C.changed_frames(_batch("lane"), np.flatnonzero(
        _oracle("lane")[0] != _batch("lane").umem)), base=7) != tot["lane"]


# ---- the oracle on the tile sweep, held to the reference -------------------------

@pytest.fixture(scope="module")
def ref():
    if not R.available() and not R.build():
        pytest.skip("reference not compiled here (no oracle/_ref and no reference checkout)")
    return R.load()


def test_oracle_equals_reference_on_the_tile_sweep(ref):
    """(Neither is handed a descriptor outside the UMEM: C.oracle_pass.)"""
    b = _batch("tile")
    for it in (1, 2):
        a, c = b.copy(), b.copy()
        va = C.oracle_pass(R.process_batch, a.umem, a.descs, iters=it, action=O.REDIRECT, nif=3, ingress=1)
        vc = C.oracle_pass(O.c_process_batch, c.umem, c.descs, iters=it, action=O.REDIRECT, nif=3, ingress=1)
        assert np.array_equal(va, vc) and np.array_equal(a.umem, c.umem)
        assert not np.array_equal(a.umem, b.umem) and (va == -1).any() and (va == 2).any()
