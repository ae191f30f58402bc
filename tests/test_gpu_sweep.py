"""The directed sweeps of tests/sweep_cases.py through the gfx950 kernels: every
frame length and alignment across each kernel family's pass and item edges, the
header rules against every ihl, and the fold's edge sums.  Each case is one
launch (or one pass of a host path) over a cached batch; every verdict and the
whole UMEM are compared with the oracle's, which tests/test_sweep.py holds to
the reference's own function on these very batches.
"""
import ctypes

import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import staged_cases as SC
from tests import sweep_cases as S
from xsknf_amd import Checksummer, ChecksummerOptions, frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.test_gpu_parity import PRODUCT_SHAPES, _pool_guard_never_trips, _results, launch_cfg  # noqa: E402,F401

SEED = 0x5357
NIF, INGRESS = 3, 1
FWD = (INGRESS + 1) % NIF

# The launch shapes default_cfg() (checksummer.hip: the lane kernel with per-tile
# transposed windows, and per lane for long launches; the split kernel W = 8 static
# and pooled, W = 4 pooled) and pcie_small_batch_cfg() (host_path.hip: the group
# kernels) can select, taken from PRODUCT_SHAPES less its store mode.
_SPLIT_DEFAULTS = {((16, 2, 2), 24), ((16, 2, 2), 56), ((16, 3, 2), 52)}
_OTHER_DEFAULTS = {(1, 5, 2), (32, 3, 2), (64, 2, 4)}


def _selectable(s):
    if S.family(s) == "split":
        return (s[:3], s[6]) in _SPLIT_DEFAULTS
    return s[:3] in _OTHER_DEFAULTS


FAMILIES = sorted({s[:4] + s[5:] for s in PRODUCT_SHAPES if _selectable(s)}, key=lambda s: (len(s), s))
# the mode each runs with in the product: in-line sectors (lane), deferred + own
# patches (split), in-line 2-byte stores over PCIe (group)
PRODUCT_MODE = {"lane": 1, "split": 18, "group": 5}
RECORDS_ONLY, INLINE_2B = 3, 5


def _with_mode(fam, mode):
    return fam[:4] + (mode,) + fam[4:]


def _modes(fam):
    m = [PRODUCT_MODE[S.family(_with_mode(fam, 0))], RECORDS_ONLY, INLINE_2B]
    if S.family(_with_mode(fam, 0)) == "group":
        m.append(1)           # (PRODUCT_SHAPES lists the group shapes with in-line sectors too)
    return sorted(set(m))


LENGTH_CASES = [(_with_mode(f, m), it) for f in FAMILIES for m in _modes(f) for it in (1, 2)]


def _id(shape):
    return "-".join(map(str, shape))


def test_the_families_are_product_shapes():
    assert len(FAMILIES) == 7
    for f in FAMILIES:
        fam = S.family(_with_mode(f, 0))
        if fam != "group":    # (the host path sets the group shapes' 2-byte stores itself)
            assert _with_mode(f, PRODUCT_MODE[fam]) in PRODUCT_SHAPES
        assert any(s[:4] + s[5:] == f for s in PRODUCT_SHAPES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- cached batches and their oracle results ------------------------------------

_batches, _oracle = {}, {}


def _batch(key):
    """key: ("length", bounds), ("nic", bounds), "header" or "fold"."""
    if key not in _batches:
        if key == "header":
            b = S.header_sweep(SEED + 1)
        elif key == "fold":
            b = S.fold_sweep(SEED + 2)
        elif key[0] == "length":
            b = S.length_sweep(key[1], SEED)
        else:
            b = _batch(("length", key[1])).copy()
            assert frames.offload_checks_host(b) > b.n // 2
        b.umem.setflags(write=False)
        _batches[key] = b
    return _batches[key]


def _case(key, iters, nif=NIF, ingress=INGRESS):
    """(batch, positions and values of the bytes the oracle changes, its verdicts);
    computed once per (batch, options), before the launch that is compared."""
    b = _batch(key)
    k = (key, iters, nif, ingress)
    if k not in _oracle:
        r = b.copy()
        ov = O.c_process_batch(r.umem, r.descs, ingress=ingress, iters=iters, action=O.REDIRECT, nif=nif)
        at = np.flatnonzero(r.umem != b.umem)
        _oracle[k] = (at, r.umem[at].copy(), ov)
    return (b,) + _oracle[k]


def _same(b, at, vals, ov, gu, gv, what=""):
    bad = np.flatnonzero(gv != ov)
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {_where(b, bad[:8])}"
    want = b.umem.copy()
    want[at] = vals
    diff = np.flatnonzero(gu != want)
    if diff.size:
        start = b.frame_offsets().astype(np.int64)
        fr = np.unique(np.searchsorted(start, diff, side="right") - 1)
        raise AssertionError(f"{what}: {diff.size} UMEM bytes differ, first at {diff[:8]}, in or after frames "
                             f"{fr[:8]}: {_where(b, fr[:8])}")


def _where(b, idx):
    """(len, nch, start phase, end phase, ihl) of the given frames, for a failure's message."""
    start, ln, rs, e, nch = S.geometry(b)
    out = []
    for i in idx:
        ihl = int(b.umem[start[i] + 14]) & 15 if ln[i] >= 15 else -1
        out.append(dict(len=int(ln[i]), nch=int(nch[i]), rs=int(rs[i]), e=int(e[i]), ihl=ihl))
    return out


def _to_device(b, dev):
    umem = torch.from_numpy(b.umem.copy()).to(dev)
    descs = torch.from_numpy(b.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    return umem, descs


def _launch_cfg(b, dev, shape, iters):
    from xsknf_amd import _lib
    lib = _lib.load()
    umem, descs = _to_device(b, dev)
    v = torch.empty(b.n, dtype=torch.int32, device=dev)
    rc = lib.xsknf_gpu_checksum_batch_cfg(
        ctypes.c_void_p(umem.data_ptr()), umem.numel(), ctypes.c_void_p(descs.data_ptr()), b.n, INGRESS,
        ctypes.byref(_lib.CsumOpts(iters, O.REDIRECT, NIF, 0)), ctypes.c_void_p(v.data_ptr()),
        ctypes.byref(launch_cfg(shape)), None)
    assert rc == 0
    return _results(v, umem)


def _apply_records(b, rec_words, gu):
    """Records-only mode (include/xsknf_gpu.h): the UMEM is only read; a tagged
    word carries the frame's UDP offset and check, and stands for the forward
    verdict.  Returns (the UMEM with the records applied, the verdicts)."""
    assert np.array_equal(gu, b.umem)
    rec = rec_words.view(np.uint32)
    tagged = (rec & 0xC0000000) == 0x40000000
    host, verd = b.umem.copy(), rec_words.copy()
    at = b.frame_offsets().astype(np.int64)[tagged] + ((rec[tagged] >> 16) & 0x7F).astype(np.int64) + 6
    host[at] = (rec[tagged] & 0xFF).astype(np.uint8)
    host[at + 1] = ((rec[tagged] >> 8) & 0xFF).astype(np.uint8)
    verd[tagged] = FWD
    return host, verd


# ---- per product shape: the length sweep over its own boundaries ----------------

@pytest.mark.parametrize("shape,iters", LENGTH_CASES, ids=[f"{_id(s)}-i{it}" for s, it in LENGTH_CASES])
def test_length_sweep_every_product_shape(dev, shape, iters):
    """length_sweep(boundaries(shape)) through xsknf_gpu_checksum_batch_cfg: every
    length up to past the shape's first edge at every start phase, and every
    (start phase, end phase) pair at every chunk count from one below to two
    above each edge -- where the split kernel's phase A hands over to items and
    an item to the next, the lane kernel's window to its tail loop, a group pass
    to the next -- under the shape's product store mode, records only and
    in-line 2-byte stores, at one and two iterations."""
    bounds = S.boundaries(shape)
    b, at, vals, ov = _case(("length", bounds), iters)
    gv, gu = _launch_cfg(b, dev, shape, iters)
    if shape[4] == RECORDS_ONLY:
        gu, gv = _apply_records(b, gv, gu)
    _same(b, at, vals, ov, gu, gv, _id(shape))


_NIC_SHAPES = [_with_mode(f, PRODUCT_MODE[S.family(_with_mode(f, 0))]) for f in FAMILIES
               if S.family(_with_mode(f, 0)) in ("lane", "split")]


@pytest.mark.parametrize("shape", _NIC_SHAPES, ids=_id)
def test_length_sweep_with_nic_checks(dev, shape):
    """The split and lane sweeps with the checks a NIC's offload wrote: the
    kernels find most checks in place and elide the store, at the same edges.
    More than half of the frames keep their bytes; all equal the oracle's."""
    bounds = S.boundaries(shape)
    b, at, vals, ov = _case(("nic", bounds), 1)
    start = b.frame_offsets().astype(np.int64)
    changed = np.unique(np.searchsorted(start, at, side="right") - 1).size
    assert b.n - changed > b.n // 2, (changed, b.n)
    assert changed > 0
    gv, gu = _launch_cfg(b, dev, shape, 1)
    _same(b, at, vals, ov, gu, gv, _id(shape))


# ---- the default entry points: header rules and fold edges ----------------------

def _pool_min_mean():
    return S.code_constant("checksummer.hip", r"constexpr uint32_t kPoolMinMean = (\d+);")


def _entry(dev, b, iters, hint, mean=0):
    """Through Checksummer.process_batch (xsknf_gpu_checksum_batch_lens)."""
    cs = Checksummer(ChecksummerOptions(action=O.REDIRECT, csum_iterations=iters), num_interfaces=NIF,
                     frame_len_hint=hint, frame_len_mean=mean)
    umem, descs = _to_device(b, dev)
    v = cs.process_batch(umem, descs, ingress_ifindex=INGRESS)
    return _results(v, umem) + (cs.launch_cfg().window_chunks,)


# (hint, mean): the lane kernel, the pooled W = 8 split kernel, the jumbo one;
# and a mean under / over kPoolMinMean: the static and the pooled W = 8 schedule
def _entries():
    m = _pool_min_mean()
    return [(64, 0, 1024), (1500, 0, 56), (9000, 0, 52), (1500, m - 1, 24), (1500, m, 56)]


@pytest.mark.parametrize("k", range(5), ids=["hint64", "hint1500", "hint9000", "mean-below", "mean-above"])
def test_header_sweep_default_entry_points(dev, k):
    """Every ihl x every length 0..130 x every start phase, one frame in 8 no
    IPv4 or no UDP: the rules of checksummer_user.c:34-55 at every ihl's own
    `udp + 8 > end` length, through each kernel the default shapes choose."""
    hint, mean, window = _entries()[k]
    b, at, vals, ov = _case("header", 1)
    gv, gu, w = _entry(dev, b, 1, hint, mean)
    assert w == window
    _same(b, at, vals, ov, gu, gv, f"hint {hint} mean {mean}")


@pytest.mark.parametrize("iters", S.FOLD_ITERS)
@pytest.mark.parametrize("k", range(5), ids=["hint64", "hint1500", "hint9000", "mean-below", "mean-above"])
def test_fold_sweep_default_entry_points(dev, k, iters):
    """Pre-fold sums with lo + hi == 0xFFFF, 0x10000 (the carry the single fold
    drops) and 0x1FFFE, sums that wrap 2^32 under 7919 iterations, and zero
    passes (-3), at even and odd starts in every size class."""
    hint, mean, window = _entries()[k]
    b, at, vals, ov = _case("fold", iters)
    gv, gu, w = _entry(dev, b, iters, hint, mean)
    assert w == window
    _same(b, at, vals, ov, gu, gv, f"hint {hint} mean {mean} iters {iters}")


# ---- the host paths -------------------------------------------------------------

def _host_path(b, path, batch, iters=1, hint=1500, submit=False):
    from xsknf_amd import HostPath
    cs = Checksummer(ChecksummerOptions(action=O.REDIRECT, csum_iterations=iters), num_interfaces=NIF,
                     frame_len_hint=hint)
    umem = b.umem.copy()
    out = np.full(b.n, 7, dtype=np.int32)
    with HostPath(cs, umem, path=path, max_batch=batch) as hp:
        if submit:
            t = [hp.submit(b.descs[lo:lo + batch], out[lo:lo + batch], ingress_ifindex=INGRESS)
                 for lo in range(0, b.n, batch)]
            hp.wait(t[-1])
        else:
            for lo in range(0, b.n, batch):
                hp.process_batch(b.descs[lo:lo + batch], ingress_ifindex=INGRESS, verdicts=out[lo:lo + batch])
        st = hp.stats()
    assert st["frames"] == b.n
    return out, umem, st


@pytest.mark.parametrize("shape,batch", [((32, 3, 2, 0, 5), 256), ((64, 2, 4, 0, 5), 2048)], ids=["32x3", "64x2"])
def test_length_sweep_zerocopy_group_shapes(dev, shape, batch):
    """The zero-copy host path runs batches of up to 256 frames as 32 x 3 groups
    and up to 2048 as 64 x 2 (pcie_small_batch_cfg): each shape's sweep in
    batches of its size, frames read and checks written in host memory."""
    m = S.code_match("host_path.hip", r"cfg\.lanes_per_frame = n <= (\d+) \? (\d+) : (\d+);")
    big = S.code_constant("host_path.hip", r"if \(n > (\d+)\) return;")
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), big) == (256, 32, 64, 2048)
    assert (batch <= 256) == (shape[0] == 32) and batch <= big
    b, at, vals, ov = _case(("length", S.boundaries(shape)), 1)
    gv, gu, _ = _host_path(b, "zerocopy", batch)
    _same(b, at, vals, ov, gu, gv, f"zerocopy {batch}")


def test_length_sweep_staged_split(dev):
    """STAGED: each batch of the packed, in-order sweep is one DMA run to the
    device mirror, the pooled W = 8 split kernel leaves records, and the host
    applies them."""
    b, at, vals, ov = _case(("length", S.boundaries((16, 2, 2, 0, 18, 1, 56))), 1)
    gv, gu, st = _host_path(b, "staged", 4096)
    _same(b, at, vals, ov, gu, gv, "staged")
    assert st["bytes_h2d"] == sum(SC.counters(b.descs[lo:lo + 4096], b.umem.size, 4096)[0]
                                  for lo in range(0, b.n, 4096))


def test_length_sweep_resident(dev):
    """The resident kernel's 8 x 12-chunk tiles (1536 B a pass): its sweep in
    256-frame ring entries."""
    b, at, vals, ov = _case(("length", S.boundaries("resident")), 1)
    gv, gu, st = _host_path(b, "resident", 256, submit=True)
    _same(b, at, vals, ov, gu, gv, "resident")
    assert st["resident_batches"] == -(-b.n // 256)
