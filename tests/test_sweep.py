"""The directed sweep batches of tests/sweep_cases.py, on the CPU: that each holds
what it is meant to hold (conditions on the fixtures, counted from the batches'
inputs alone), and that the oracle's pass over each equals the reference's own
compiled function -- so tests/test_gpu_sweep.py rests on the reference, not on
the restatement.  (tests/test_ref_pin.py pins the oracle on 20,000 random
frames; this extends the pin to the directed ones.)"""
import numpy as np
import pytest

from oracle import csum_oracle as O
from oracle import ref as R
from tests import sweep_cases as S

# one launch shape per boundary set in use (tests/test_gpu_sweep.py derives the
# same sets from test_gpu_parity.PRODUCT_SHAPES; that file needs torch)
SETS = {
    "lane": (1, 5, 2, 0, 1, 0, 1024),
    "split-w8": (16, 2, 2, 0, 18, 1, 24),
    "split-w8-pool": (16, 2, 2, 0, 18, 1, 56),
    "split-w4-pool": (16, 3, 2, 0, 18, 1, 52),
    "group-32x3": (32, 3, 2, 0, 5),
    "group-64x2": (64, 2, 4, 0, 5),
    "resident": "resident",
}
EXPECTED = {
    "lane": (5, 10, 15), "split-w8": (8, 40, 72), "split-w8-pool": (8, 40, 72), "split-w4-pool": (4, 52, 100),
    "group-32x3": (96, 192), "group-64x2": (128, 256), "resident": (96, 192),
}
SEED = 0x5357          # "SW"

_cache = {}


def _length(bounds):
    if bounds not in _cache:
        _cache[bounds] = S.length_sweep(bounds, SEED)
    return _cache[bounds]


def _header():
    if "header" not in _cache:
        _cache["header"] = S.header_sweep(SEED + 1)
    return _cache["header"]


def _fold():
    if "fold" not in _cache:
        _cache["fold"] = S.fold_sweep(SEED + 2)
    return _cache["fold"]


@pytest.fixture(scope="module")
def ref():
    if not R.available() and not R.build():
        pytest.skip("reference not compiled here (no oracle/_ref and no reference checkout)")
    return R.load()


@pytest.mark.parametrize("name", list(SETS))
def test_boundaries_are_the_codes(name):
    """What boundaries() reads from the sources today ("Directed sweeps"): a change of
    W, SPAN or the resident tile changes this list with it, knowingly."""
    assert S.boundaries(SETS[name]) == EXPECTED[name]


def test_one_edge_length_per_phase_pair():
    for nch in (2, 5, 96):
        for rs in range(16):
            for e in range(16):
                ln = S._edge_len(nch, rs, e)
                assert ln >= 0 and (rs + ln + 15) >> 4 == nch and (rs + ln) & 15 == e


@pytest.mark.parametrize("bounds", sorted(set(EXPECTED.values())), ids=lambda b: "-".join(map(str, b)))
def test_length_sweep_holds_every_edge(bounds):
    b = _length(bounds)
    cov = S.length_coverage(b, bounds)
    print(bounds, b.n, "frames", b.umem.size >> 20, "MiB", cov["pairs"])
    assert cov["dense_missing"] == 0              # every length 0..16 min(bounds) + 48 at every start phase
    assert len(cov["pairs"]) == 4 * len(bounds)
    assert all(v == 256 for v in cov["pairs"].values()), cov["pairs"]      # every (start, end) phase pair
    assert all(v == 2 for v in cov["parities"].values())                   # both parities of the UDP start
    assert cov["not_ihl5"] == 0
    in_order, max_gap, overlaps = S.packing(b)
    assert in_order and overlaps == 0 and max_gap <= 15                    # back to back
    assert (b.descs["addr"] >> np.uint64(48)).max() == 255                 # the base | off << 48 layout
    assert b.n <= 70_000 and b.umem.size <= 150 << 20
    # thinner elsewhere, but every length up to the last boundary's sweep is there
    assert np.array_equal(np.unique(b.descs["len"]), np.arange(16 * (max(bounds) + 2) + 1))


def test_header_sweep_holds_every_cell():
    b = _header()
    cov = S.header_coverage(b)
    print(b.n, "frames", cov)
    assert b.n == 16 * 131 * 16 == 33_536
    assert cov["cells"] == 16 * (S.HEADER_MAX_LEN + 1 - 15) * 16
    assert cov["short_cells"] == 15 * 16 and cov["short_min"] == cov["short_max"] == 16
    assert cov["other"] == 0.125                                     # one frame in 8
    for ihl, (dropped, summed) in cov["edge"].items():                     # `udp + 8 > end` at every ihl
        assert 14 + 4 * ihl + 8 <= S.HEADER_MAX_LEN
        assert dropped == 14 and summed == 14, (ihl, dropped, summed)      # (of 16: one in 8 is no IPv4/UDP)
    in_order, max_gap, overlaps = S.packing(b)
    assert in_order and overlaps == 0 and max_gap <= 15
    # the verdicts the rules of :34-55 give all occur: dropped, passed untouched, summed
    v = O.c_process_batch(b.umem.copy(), b.descs.copy(), iters=1, action=O.REDIRECT, nif=3, ingress=1)
    assert (v == -1).any() and (v == 0).any() and (v == 2).any()


def test_fold_sweep_holds_every_class():
    b = _fold()
    assert 150 < b.n <= 12 * len(S.FOLD_TARGETS) * 2
    for cls, it in S.FOLD_TARGETS:
        t, wrapped, parity, size = S.fold_classes(b, it)
        at = t == S.FOLD_CLASSES[cls]
        assert at.any(), (cls, it)
        assert set(parity[at]) == {0, 1}, (cls, it)
        if cls != "1fffe" or it == 7919:
            assert set(size[at]) >= ({64, 570, 1500, 9000} if cls != "1fffe" else {9000}), (cls, it, set(size[at]))
    t, wrapped, _, size = S.fold_classes(b, 7919)
    assert wrapped[size == 9000].all() and wrapped.any() and set(size[wrapped]) >= {570, 1500, 9000}
    t, wrapped, _, _ = S.fold_classes(b, -3)
    assert not wrapped.any() and (t < 0xFFFF).all()                        # zero passes: the pseudo-header alone
    # classified from the oracle's output: checks 0x0000 and 0xFFFF both occur,
    # exactly on the frames the closed form puts in those classes
    seen = set()
    for it in S.FOLD_ITERS:
        r = b.copy()
        v = O.c_process_batch(r.umem, r.descs, iters=it, action=O.REDIRECT, nif=1)
        assert (v == 0).all()                                              # every frame is summed
        c = S.written_checks(b, r.umem)
        t, _, _, _ = S.fold_classes(b, it)
        assert np.array_equal(c, ~(t & 0xFFFF) & 0xFFFF), it
        assert np.array_equal(c == 0x0000, t == 0xFFFF)
        assert (c[t == 0x1FFFE] == 0x0001).all()                           # (a second fold would give 0x0000)
        assert np.array_equal(c == 0xFFFF, (t == 0x10000) | (t == 0))
        seen |= set(np.unique(c[(c == 0) | (c == 0xFFFF)]).tolist())
    assert seen == {0x0000, 0xFFFF}


def _same_as_reference(b, **kw):
    a, c = b.copy(), b.copy()
    va = R.process_batch(a.umem, a.descs, **kw)
    vc = O.c_process_batch(c.umem, c.descs, **kw)
    assert np.array_equal(va, vc), (kw, np.nonzero(va != vc)[0][:8])
    assert np.array_equal(a.umem, c.umem), (kw, np.nonzero(a.umem != c.umem)[0][:8])
    assert not np.array_equal(a.umem, b.umem)                              # (something was written)


@pytest.mark.parametrize("bounds", sorted(set(EXPECTED.values())), ids=lambda b: "-".join(map(str, b)))
def test_oracle_equals_reference_on_the_length_sweep(ref, bounds):
    for it in (1, 2):
        _same_as_reference(_length(bounds), iters=it, action=O.REDIRECT, nif=3, ingress=1)


def test_oracle_equals_reference_on_the_header_sweep(ref):
    for it in (1, 2):
        _same_as_reference(_header(), iters=it, action=O.REDIRECT, nif=3, ingress=1)


def test_oracle_equals_reference_on_the_fold_sweep(ref):
    for it in S.FOLD_ITERS:
        _same_as_reference(_fold(), iters=it, action=O.REDIRECT, nif=1)
