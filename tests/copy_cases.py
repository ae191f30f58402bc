"""What tests/test_copy_sweep.py (CPU) and tests/test_gpu_copy_sweep.py share: the
directed batches of tests/sweep_cases.py turned on the kernels that move frames
around the checksum pass -- forward_frames (kernel_forward.h), pack_frames,
apply_records and shard_counters (kernel_pack.h), scatter_checks (kernel_scatter.h).

They decide on the quantities the sweeps hold at every value: a frame's 16-byte
chunk count from its aligned-down start, its partial first and last chunk, and
the place of a chunk in a wave's round robin over a 64-entry tile.  The length
sweep holds every length at every start phase; `tile_sweep` adds the tile
edges: chunk totals around a round (64 chunks) and a trip (64 kUnroll chunks,
the forward's unrolled loop), frames that end and start, or lie, on those edges
with partial chunks, frames longer than a trip at either end of a tile, and
zero-chunk entries around them.  All sizes are read from the sources by pattern.

Bytes that cannot hide a miss: the forward's destinations start as the bitwise
complement of the rx UMEM, so a frame byte that is not copied and an outside
byte that is both differ from the model, whatever the payload.
"""
import numpy as np

from tests import forward_cases as FC
from tests import sweep_cases as S
from tests.route_cases import code_constant, code_match
from xsknf_amd import frames

OUT = np.uint64(1 << 40)          # added to an address: outside any UMEM here
MASK48 = np.uint64((1 << 48) - 1)


def constants():
    """(R, P): chunks per round of a wave's round robin and per trip of the
    forward's chunk loop, from the code.  The tile is 64 entries in both
    kernels, the pack strides by one round."""
    h = "kernel_forward.h"
    tile = code_constant(h, r"const uint64_t e = t \* (\d+) \+ lane;")
    unroll = code_constant(h, r"constexpr int kUnroll = (\d+);")
    code_match(h, r"for \(uint64_t k0 = lane; k0 < chunks; k0 \+= 64ull \* kUnroll\)")
    code_match(h, r"const uint64_t k = k0 \+ 64ull \* u;")
    code_match(h, r"if \(k >= f_hi\) \{")
    ptile = code_constant("kernel_pack.h", r"const uint64_t f = t \* (\d+) \+ lane;")
    stride = code_constant("kernel_pack.h", r"for \(uint32_t k = lane; k < total; k \+= (\d+)\) \{")
    assert tile == ptile == stride == 64
    return 64, 64 * unroll


def offsets(descs):
    a = descs["addr"].astype(np.uint64)
    return ((a & MASK48) + (a >> np.uint64(48))).astype(np.int64)


def chunks(descs, umem_size, base=0):
    """(offset, len, in range?, nch) per descriptor, as forward_frames and
    pack_frames count them for a UMEM at address `base` mod 16: an entry of
    length 0 or outside the UMEM has no chunk."""
    off, ln = offsets(descs), descs["len"].astype(np.int64)
    inr = (off <= umem_size) & (ln <= umem_size - np.minimum(off, umem_size))
    nch = np.where(inr & (ln > 0), (((off + base) & 15) + ln + 15) >> 4, 0)
    return off, ln, inr, nch


def oracle_pass(fn, umem, descs, **kw):
    """fn (oracle.csum_oracle.c_process_batch or oracle.ref.process_batch) over
    the batch IN PLACE, as tests/oracles.py runs the full-size batches: a
    descriptor outside the UMEM never reaches the reference (the kernel's rx
    validation drops it; xsknf_gpu's boundary gives it -1, untouched), so such
    descriptors get -1 here and only the others go to fn."""
    inr = chunks(descs, umem.size)[2]
    v = np.full(descs.shape[0], -1, dtype=np.int32)
    v[inr] = fn(umem, np.ascontiguousarray(descs[inr]), **kw)
    return v


# ---- the tile sweep -------------------------------------------------------------

TOTALS = lambda R, P: (1, R - 1, R, R + 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P + 1)  # noqa: E731
EDGES = lambda R, P: (R, 2 * R, 3 * R, P, 2 * P)                                                    # noqa: E731
ZERO, GONE = "zero", "gone"       # the two zero-chunk entries: length 0, a descriptor outside the UMEM


def _frame(rng, nch, rs=None, e=None):
    """(len, start phase) of a frame of nch chunks; rs, e: its phases (random if None)."""
    if rs is None:
        rs = int(rng.integers(0, 16))
    if e is None:
        e = int(rng.integers(rs + 1, 17)) & 15 if nch == 1 else int(rng.integers(0, 16))
    elif nch == 1 and 0 < e <= rs:          # one chunk: the window needs b0 < b1 (both given, both odd)
        rs, e = (e, rs) if e < rs else (rs - 2 if rs == 15 else rs, min(rs + 2, 15))
    ln = S._edge_len(nch, rs, e)
    assert ln > 0 and (rs + ln + 15) >> 4 == nch
    return ln, rs


def _fill(rng, total, k):
    """k entries holding `total` chunks in all, the cuts random: frames of
    random phases, and zero-chunk entries of both kinds where a part is empty."""
    cuts = np.sort(rng.integers(0, total + 1, k - 1)) if k > 1 else np.zeros(0, dtype=np.int64)
    parts = np.diff(np.concatenate([[0], cuts, [total]]))
    return [_frame(rng, int(p)) if p else (ZERO if i % 2 else GONE) for i, p in enumerate(parts)]


def _tiles(rng, R, P):
    odd = lambda: int(rng.integers(0, 8)) * 2 + 1          # noqa: E731
    tiles = []
    # chunk totals around a round and a trip; total 1: the frame between two runs of zero-chunk entries
    for tot in TOTALS(R, P):
        if tot == 1:
            tiles.append([ZERO, GONE] * 10 + [_frame(rng, 1)] + [GONE, ZERO] * 21 + [ZERO])
        else:
            tiles.append(_fill(rng, tot, 64))
    for E in EDGES(R, P):
        # frame A ends in chunk E - 1, the next entry B starts in chunk E, both partial
        # there; a zero-chunk entry before A and after B
        a, b = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        head = _fill(rng, E - a, 20)
        tiles.append(head + [ZERO, _frame(rng, a, odd(), odd()), _frame(rng, b, odd(), odd()), GONE] +
                     _fill(rng, int(rng.integers(30, 90)), 64 - 24))
        # one frame of two chunks, E - 1 and E, both partial; zero-chunk entries around it
        rs = odd()
        e = odd()
        head = _fill(rng, E - 1, 31)
        tiles.append(head + [GONE, _frame(rng, 2, rs, e), ZERO] + _fill(rng, int(rng.integers(30, 90)), 64 - 34))
        # and one long frame holding both from the inside (its edge chunks are whole)
        tiles.append(_fill(rng, E - 5, 12) + [_frame(rng, 11, odd(), odd())] + _fill(rng, 40, 51))
    # one frame of more than a trip: the tile's first entry, its last, in the middle
    long_ = lambda: _frame(rng, P + int(rng.integers(3, 60)), odd(), odd())      # noqa: E731
    tiles.append([long_()] + _fill(rng, 70, 63))
    tiles.append(_fill(rng, 70, 63) + [long_()])
    tiles.append(_fill(rng, 40, 31) + [long_()] + _fill(rng, 40, 32))
    # runs of zero-chunk entries at the head and the tail of a tile with work in it
    tiles.append([ZERO, GONE, GONE, ZERO] * 4 + _fill(rng, R + 9, 30) + [GONE, ZERO] * 9)
    # two plain tiles (the forward's interface boundaries fall inside them) and a partial last one
    tiles.append(_fill(rng, 150, 64))
    tiles.append(_fill(rng, 150, 64))
    tiles.append(_fill(rng, 50, 23))
    assert all(len(t) == 64 for t in tiles[:-1]) and len(tiles[-1]) < 64
    return tiles


def tile_sweep(seed):
    """Frames grouped in aligned 64-entry tiles (entry 64 t is a wave's first),
    packed back to back like the length sweep (neighbours share chunks), ihl 5,
    payload and gaps random.  What it holds is counted by tile_coverage()."""
    R, P = constants()
    rng = np.random.default_rng(seed)
    entries = [x for t in _tiles(rng, R, P) for x in t]
    gone = np.array([x == GONE for x in entries])
    lens = np.array([0 if isinstance(x, str) else x[0] for x in entries], dtype=np.int64)
    phases = np.zeros(lens.size, dtype=np.int64)
    end = 0
    for i, x in enumerate(entries):          # (a zero-chunk entry sits where the last frame ended: no gap of its own)
        phases[i] = end & 15 if isinstance(x, str) else x[1]
        end += ((phases[i] - end) & 15) + lens[i]
    b = S._packed(lens, phases, rng)
    b.descs["addr"][gone] += OUT
    b.descs["len"][gone] = 100 + np.arange(int(gone.sum())) % 1400      # (bytes they would have, were they inside)
    return b


def tile_coverage(b):
    """What a batch's aligned 64-entry tiles hold, from its descriptors and the
    UMEM's size alone (R, P from the code):
    totals -- the tiles' chunk totals; split[E] / single[E] / inside[E] -- tiles
    where a frame's last chunk is E - 1 and the NEXT entry's first is E, where a
    frame's two chunks are E - 1 and E, where a longer frame holds both; each
    counted only with odd phases at both ends of the frames at the edge;
    zero_before / zero_after -- the kinds of zero-chunk entry directly before and
    after those edge frames; long_at -- where frames of more than P chunks sit
    in their tile; head_run / tail_run -- the longest run of zero-chunk entries
    at the head / tail of a tile that has chunks; last -- entries in the last tile."""
    R, P = constants()
    off, ln, inr, nch = chunks(b.descs, b.umem.size)
    rs, e = off & 15, (off + ln) & 15
    oddf = (rs & 1 == 1) & (e & 1 == 1)
    kind = np.where(nch > 0, "", np.where(inr, ZERO, GONE))
    cov = dict(totals=set(), split={}, single={}, inside={}, zero_before=set(), zero_after=set(), long_at=set(),
               head_run=0, tail_run=0, last=b.n % 64 or 64, n=b.n, bytes=int(b.umem.size))
    for t0 in range(0, b.n, 64):
        c = nch[t0:t0 + 64]
        m = c.size
        pre = np.concatenate([[0], np.cumsum(c)])
        cov["totals"].add(int(pre[-1]))
        lo, hi = pre[:-1], pre[1:] - 1          # a frame's first and last chunk of the tile (c > 0)
        for j in np.flatnonzero(c > P):
            cov["long_at"].add("first" if j == 0 else "last" if j == 63 else "middle")
        for E in EDGES(R, P):
            for j in np.flatnonzero((c > 0) & (hi == E - 1)):
                if j + 1 < m and c[j + 1] > 0 and oddf[t0 + j] and oddf[t0 + j + 1]:
                    cov["split"][E] = cov["split"].get(E, 0) + 1
                    if j > 0 and c[j - 1] == 0:
                        cov["zero_before"].add(str(kind[t0 + j - 1]))
                    if j + 2 < m and c[j + 2] == 0:
                        cov["zero_after"].add(str(kind[t0 + j + 2]))
            for j in np.flatnonzero((c > 0) & (lo <= E - 1) & (hi >= E) & oddf[t0:t0 + m]):
                two = lo[j] == E - 1 and hi[j] == E
                cov["single" if two else "inside"][E] = cov["single" if two else "inside"].get(E, 0) + 1
                if two and j > 0 and c[j - 1] == 0:
                    cov["zero_before"].add(str(kind[t0 + j - 1]))
                if two and j + 1 < m and c[j + 1] == 0:
                    cov["zero_after"].add(str(kind[t0 + j + 1]))
        if pre[-1]:
            work = np.flatnonzero(c > 0)
            cov["head_run"] = max(cov["head_run"], int(work[0]))
            cov["tail_run"] = max(cov["tail_run"], int(m - 1 - work[-1]))
    return cov


def tile_coverage_holds(cov):
    """The conditions on tile_sweep(), asserted."""
    R, P = constants()
    assert set(TOTALS(R, P)) <= cov["totals"], sorted(set(TOTALS(R, P)) - cov["totals"])
    for E in EDGES(R, P):
        assert cov["split"].get(E, 0) >= 1, ("split", E, cov["split"])
        assert cov["single"].get(E, 0) >= 1, ("single", E, cov["single"])
        assert cov["inside"].get(E, 0) >= 1, ("inside", E, cov["inside"])
    assert cov["zero_before"] == {ZERO, GONE} and cov["zero_after"] == {ZERO, GONE}, cov
    assert cov["long_at"] == {"first", "last", "middle"}, cov["long_at"]
    assert cov["head_run"] >= 8 and cov["tail_run"] >= 8
    assert cov["last"] < 64
    assert cov["n"] <= 5000 and cov["bytes"] <= 4 << 20


# ---- the reused length sweep, restated for the copy kernels ---------------------

LANE_BOUNDS, SPLIT_BOUNDS = (5, 10, 15), (8, 40, 72)


def copy_coverage(b):
    """From the batch alone: windows -- distinct [b0, b1) windows of one-chunk
    frames (136 = all with 0 <= b0 < b1 <= 16); pairs[n] -- distinct (start
    phase, end phase) pairs among the frames of n chunks, n = 2..9; shared -- the
    neighbours that share a 16-byte chunk; max_nch."""
    off, ln, inr, nch = chunks(b.descs, b.umem.size)
    rs = off & 15
    one = nch == 1
    windows = np.unique(rs[one] * 32 + rs[one] + ln[one]).size
    pairs = {n: int(np.unique(rs[nch == n] * 16 + ((off + ln)[nch == n] & 15)).size) for n in range(2, 10)}
    live = np.flatnonzero(nch > 0)
    shared = int((((off + ln)[live[:-1]] - 1) >> 4 == off[live[1:]] >> 4).sum())
    return dict(windows=int(windows), pairs=pairs, shared=shared, max_nch=int(nch.max()))


# ---- the forward: lists, destinations and the model ------------------------------

def forward_inputs(b):
    """(rx UMEM, descriptors) of a batch as aligned arrays, the options non-zero."""
    rx = FC.aligned_u8(b.umem.size)
    rx[:] = b.umem
    rx.setflags(write=False)
    d = FC.aligned_descs(b.n)
    d["addr"], d["len"], d["options"] = b.descs["addr"], b.descs["len"], 7
    d.setflags(write=False)
    return rx, d


def complement(rx, dst_sizes):
    """The destinations before a forward: ~rx over each one's length (None, "rx":
    no array).  Aligned, writable, fresh with every call."""
    out = []
    for s in dst_sizes:
        if not isinstance(s, int):
            out.append(None)
            continue
        a = FC.aligned_u8(s, 0)
        k = min(s, rx.size)
        a[:k] = ~rx[:k]
        out.append(a)
    return out


def verdicts(b, how):
    """(verdicts, dst_sizes).  "one": every frame to one interface with a UMEM of
    its own, so the tx list is the batch and its tiles.  "three": the frames
    dealt in turn to an interface with its own UMEM, one that shares the rx UMEM
    and one with a smaller UMEM of its own (its far frames are skipped):
    neighbouring frames land in different UMEMs.  "ranges": the same three kinds
    in three runs of frames in batch order, the cuts inside the last two full
    tiles -- the tx list is the batch again, with an interface boundary mid-tile
    on either side of a run of entries that are not looked at."""
    size, n = int(b.umem.size), b.n
    if how == "one":
        return np.zeros(n, dtype=np.int32), [size]
    if how == "three":
        return (np.arange(n) % 3).astype(np.int32), [size, None, (size // 2 + 1000) & ~15]
    assert how == "ranges"
    full = n // 64 * 64
    a, c = full - 128 + 21, full - 64 + 37
    v = np.full(n, 2, dtype=np.int32)
    v[:a], v[a:c] = 0, 1
    return v, [size, None, size]


# ---- scatter_checks' per-frame choice -------------------------------------------

def scatter_masks(b, changed, base=0):
    """Per frame whose check a pass changes (`changed`: a mask; such frames hold
    their ihl byte), with the UMEM at an address `base` mod 64: (straddle,
    before, past) as rewrite_check decides them -- the check's two bytes lie in
    two 64-byte sectors, its sector starts before the frame, ends past it."""
    off, ln = offsets(b.descs)[changed], b.descs["len"].astype(np.int64)[changed]
    u = 14 + 4 * (b.umem[off + 14].astype(np.int64) & 15)
    chk, fp = off + u + 6 + base, off + base
    sec = chk & ~63
    return chk & 63 == 63, sec < fp, sec + 64 > fp + ln


def scatter_classes(b, changed, base=0):
    """How rewrite_check writes the changed frames' checks, counted: the whole
    64-byte sector, or two bytes because the sector starts before the frame
    ("before"), ends past it ("past"), or the check straddles two sectors
    ("straddle", taken first; "straddle_inside": with the sector inside the
    frame, where the straddle alone decides)."""
    straddle, before, past = scatter_masks(b, changed, base)
    whole = ~straddle & ~before & ~past
    return dict(whole=int(whole.sum()), before=int((~straddle & before).sum()), past=int((~straddle & past).sum()),
                straddle=int(straddle.sum()), straddle_inside=int((straddle & ~before & ~past).sum()))


def changed_frames(b, at):
    """The mask of frames that hold one of the byte positions `at` (sorted
    frames, no overlaps: the sweeps' layout)."""
    start = b.frame_offsets().astype(np.int64)
    m = np.zeros(b.n, bool)
    m[np.unique(np.searchsorted(start, at, side="right") - 1)] = True
    return m


# ---- the counters ----------------------------------------------------------------

def counters_model(umem_after, descs, verdicts):
    """xsknf_gpu_multi_counters' six sums over a whole batch, directly: frames,
    bytes of every descriptor, drops, forwards, and over the frames of 42 bytes
    or more inside the UMEM the check at +40 (little-endian) and the same times
    (offset mod 65521) + 1, modulo 2^64."""
    off, ln, inr, _ = chunks(descs, umem_after.size)
    at = off[inr & (ln >= 42)]
    ck = umem_after[at + 40].astype(np.uint64) | umem_after[at + 41].astype(np.uint64) << np.uint64(8)
    w = (at % 65521 + 1).astype(np.uint64)
    return dict(frames=int(descs.shape[0]), bytes=int(ln.sum()), drop=int((verdicts == -1).sum()),
                forward=int((verdicts >= 0).sum()), checks_sum=int(ck.sum(dtype=np.uint64)),
                checks_weighted=int((ck * w).sum(dtype=np.uint64)))


# ---- the packed layout, restated -------------------------------------------------

def packed_layout(descs, bounds, umem_addr, umem_size):
    """numpy restatement of xsknf_gpu_shard_pack_plan: (packed addresses, sizes).
    A frame inside the UMEM gets the 16-byte slots that hold its chunks, at its
    address mod 16 in the first; one of no bytes gets no slot; one outside is
    marked 1 << 47."""
    off, ln, inr, nch = chunks(descs, umem_size, umem_addr & 15)
    addr = np.full(descs.shape[0], 1 << 47, dtype=np.uint64)
    sizes = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        slot = 16 * nch[lo:hi]
        pos = np.cumsum(slot) - slot
        a = (pos + ((off[lo:hi] + umem_addr) & 15)).astype(np.uint64)
        addr[lo:hi] = np.where(inr[lo:hi], a, addr[lo:hi])
        sizes.append(int(slot.sum()))
    return addr, sizes


def slot_bytes(descs, packed_addr, umem_addr, umem_size):
    """(indices into a shard's packed bytes, indices into the UMEM): every byte
    pack_frames moves for these frames -- each frame's whole 16-byte chunks of
    memory, clipped to the UMEM -- as two flat index arrays."""
    off, ln, inr, nch = chunks(descs, umem_size, umem_addr & 15)
    live = nch > 0
    first = ((off + umem_addr) & ~15) - umem_addr          # the first chunk, relative to the UMEM (may be < 0)
    lo = np.maximum(first, 0)[live]
    hi = np.minimum(first + 16 * nch, umem_size)[live]
    slot = (packed_addr.astype(np.int64) & ~15)[live] - first[live]      # slot index of UMEM byte 0
    cnt = hi - lo
    run = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    src = np.repeat(lo, cnt) + run
    return np.repeat(slot, cnt) + src, src
