"""What tests/test_sweep.py (CPU) and tests/test_gpu_sweep.py share: directed
batches that put every frame length and alignment on the edges at which the
checksum kernels change behaviour, and the functions that count, from a batch's
inputs alone, what it holds.

The kernels count a frame in 16-byte chunks from its aligned-down start:
nch = ceil((start % 16 + len) / 16) (make_ref, csum_device.h).  Each family
steps through a frame in units read here from its source (`boundaries`), never
copied: a change of W, SPAN or the resident tile moves the sweep with it, and a
pattern the code no longer holds is an error (route_cases.code_match).

A wrong sum at such an edge is a conjunction -- the frame's last chunk is the
first or last of a pass or item, at one start phase (start % 16), one end phase
((start + len) % 16) and one parity of the UDP start -- so the batches hold
every (start phase, end phase) pair at every chunk count around every edge.

The phases are those of the frame's offset in the UMEM: they are the kernels'
when the UMEM's base is 16-byte aligned (device allocations, page-aligned host
buffers and numpy's arrays are).
"""
import numpy as np

from tests.route_cases import code_constant, code_match
from xsknf_amd import frames

HDR = frames.HDR_LEN          # 42: Ethernet + IPv4 (ihl 5) + UDP
U5 = 34                       # the UDP header's offset at ihl 5
AROUND = (-1, 0, 1, 2)        # chunk counts swept around a boundary B: B - 1 .. B + 2


# ---- the boundaries, from the kernels' sources ----------------------------------

def _kernel_window(shape):
    return (shape[5], shape[6]) if len(shape) > 5 else (0, 0)


def family(shape):
    """'resident', 'lane', 'split' or 'group' for a launch shape as
    tests/test_gpu_parity.py lists them (lanes per frame, chunks per lane,
    frames per group, ring, store mode[, kernel, window field])."""
    if shape == "resident":
        return "resident"
    kernel, _ = _kernel_window(shape)
    if kernel == 1:
        return "split"
    return "lane" if shape[0] == 1 else "group"


def split_window(shape):
    """W of a split shape: its window field less the flags, as the Variant table
    of checksummer.hip instantiates it (XSKNF_S's first argument, or the W the
    pooled macros XSKNF_SC / XSKNF_SC4 pass to launch_split)."""
    lpf, nch, u = shape[:3]
    _, window = _kernel_window(shape)
    transposed = code_constant("checksummer_internal.h", r"constexpr int kWinTransposed = (\d+);")
    pool = code_constant("checksummer_internal.h", r"constexpr int kWinPool = (\d+);")
    assert window & transposed, "the product's split shapes load their windows transposed"
    w = window - transposed - (window & pool)
    if window & pool:
        m = code_match("checksummer.hip",
                       r"#define (XSKNF_SC\w*)\(L, N, U\) \\\n\s*\{L, N, U, &launch_split<%d, L, N, U, true, \d+>, "
                       r"XSKNF_GPU_KERNEL_SPLIT, %d \+ kWinTransposed \+ kWinPool\}" % (w, w))
        code_match("checksummer.hip", r"%s\(%d, %d, %d\)[,;\s]" % (m.group(1), lpf, nch, u))
    else:
        code_match("checksummer.hip", r"XSKNF_S\(%d, %d, %d, %d, 1\)" % (w, lpf, nch, u))
    return w


def boundaries(shape):
    """The chunk counts at which `shape` changes behaviour (sorted, a tuple).

    * split: W + k SPAN, k = 0..2 -- a frame of nch <= W chunks ends in phase A,
      one of more gets ceil((nch - W) / SPAN) payload items of SPAN = LPF * NCH
      chunks, the last of them partial (kernel_split.h);
    * lane: k NCH, k = 1..3 -- the window, then the per-lane tail loop
      (kernel_lane.h);
    * group: k LPF NCH, k = 1..2 -- pass 0 in registers, the later passes of
      finish_long_frames (kernel_group.h);
    * "resident": k kResLpf kResNch, k = 1..2 -- the same tiles (kernel_resident.h).
    """
    fam = family(shape)
    if fam == "resident":
        m = code_match("kernel_resident.h", r"constexpr int kResLpf = (\d+), kResNch = (\d+), kResSpt = \d+;")
        code_match("kernel_resident.h", r"group_tiles<kResLpf, kResNch, kResSpt>\(a, g, G\)")
        span = int(m.group(1)) * int(m.group(2))
        return tuple(span * k for k in (1, 2))
    lpf, nch = shape[0], shape[1]
    if fam == "lane":
        code_match("checksummer.hip", r"XSKNF_LA?\(%d, %d\)" % (nch, shape[2]))
        code_match("kernel_lane.h", r"for \(int k = NCH; k < r\.nch; \+\+k\) chunk_sum\(")
        return tuple(nch * k for k in (1, 2, 3))
    if fam == "group":
        code_match("checksummer.hip", r"XSKNF_V\(%d, %d, %d\)" % (lpf, nch, shape[2]))
        code_match("kernel_group.h", r"constexpr int SPAN = LPF \* NCH;")
        code_match("kernel_group.h", r"for \(int p = SPAN; __builtin_amdgcn_ballot_w64\(pend && p < r\.nch\); p \+= SPAN\)")
        code_match("kernel_group.h", r"if \(do_sum && r\.nch > span\)")
        return tuple(lpf * nch * k for k in (1, 2))
    w = split_window(shape)
    code_match("kernel_split.h", r"constexpr int SPAN = LPF \* NCH;")
    code_match("kernel_split.h", r"const bool more = do_sum && r\.nch > W && ")
    code_match("kernel_split.h", r"\(r\.nch - W \+ SPAN - 1\) / SPAN\)")
    return tuple(w + k * lpf * nch for k in (0, 1, 2))


# ---- laying frames out ----------------------------------------------------------

def _layout(lens, phases):
    """Frame starts for frames packed back to back in the given order, each
    after only the 0..15 gap bytes that bring its start to its phase; and the
    UMEM's size (16 bytes past the last frame, as frames.unaligned_batch)."""
    lens = np.asarray(lens, dtype=np.int64)
    phases = np.asarray(phases, dtype=np.int64)
    starts = np.empty(lens.size, dtype=np.int64)
    end = 0
    for i, (ln, ph) in enumerate(zip(lens.tolist(), phases.tolist())):
        s = end + ((ph - end) & 15)
        starts[i] = s
        end = s + ln
    return starts, end + 16


def _descs(starts, lens):
    """base | offset << 48 descriptors, the offsets cycling through 0..255."""
    offs = np.minimum(np.arange(starts.size, dtype=np.int64) % 256, starts).astype(np.uint64)
    d = np.zeros(starts.size, dtype=frames.DESC_DTYPE)
    d["addr"] = (starts.astype(np.uint64) - offs) | (offs << np.uint64(frames.OFFSET_SHIFT))
    d["len"] = np.asarray(lens, dtype=np.uint32)
    return d


def _put_headers(umem, starts, lens, h):
    """The first min(len, 42) bytes of every frame from the rows of h."""
    cols = np.arange(h.shape[1], dtype=np.int64)
    mask = cols[None, :] < np.asarray(lens, dtype=np.int64)[:, None]
    umem[(starts[:, None] + cols[None, :])[mask]] = h[mask]


def _packed(lens, phases, rng, header_edit=None):
    starts, total = _layout(lens, phases)
    umem = rng.integers(0, 256, size=total, dtype=np.uint8)      # gaps and payload random
    h = frames.headers(lens, rng.integers(0, 256, size=len(lens)))
    if header_edit is not None:
        header_edit(h)
    _put_headers(umem, starts, lens, h)
    return frames.HostBatch(umem, _descs(starts, lens), "unaligned")


def geometry(b):
    """(start, len, start phase, end phase, nch) of every frame, from the batch."""
    start = b.frame_offsets().astype(np.int64)
    ln = b.descs["len"].astype(np.int64)
    rs = start & 15
    return start, ln, rs, (start + ln) & 15, (rs + ln + 15) >> 4


def packing(b):
    """(frames in address order?, the largest gap between neighbours, frames
    whose start overlaps the previous frame) -- back to back means gaps 0..15."""
    start, ln, _, _, _ = geometry(b)
    gap = start[1:] - (start + ln)[:-1]
    return bool(np.all(np.diff(start) >= 0)), int(gap.max(initial=0)), int((gap < 0).sum())


# ---- the length sweep -----------------------------------------------------------

def dense_limit(bounds):
    """Every length up to here sits at every start phase."""
    return 16 * min(bounds) + 48


def _edge_len(nch, rs, e):
    """The length that gives a frame of start phase rs nch chunks and end phase e."""
    return 16 * (nch - 1) + (e if e else 16) - rs


def length_requests(bounds):
    """The (len, start phase) pairs of length_sweep(bounds), unordered:
    every length 0..dense_limit at every phase; around every boundary B, every
    (start phase, end phase) pair at every nch in [B - 1, B + 2]; in between and
    up to the last boundary's sweep, every length at a few phases."""
    lim = dense_limit(bounds)
    ln, ph = np.meshgrid(np.arange(lim + 1), np.arange(16), indexing="ij")
    parts = [np.stack([ln.ravel(), ph.ravel()], axis=1)]
    rs, e = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    rs, e = rs.ravel(), e.ravel()
    for b in bounds:
        for d in AROUND:
            nch = b + d
            assert nch >= 2
            parts.append(np.stack([16 * (nch - 1) + np.where(e == 0, 16, e) - rs, rs], axis=1))
    top = 16 * (max(bounds) + AROUND[-1])
    thin = 4 if top <= 2048 else 2          # (the long sets stay within their size)
    ln = np.arange(lim + 1, top + 1)
    for j in range(thin):
        parts.append(np.stack([ln, (5 * ln + j * (16 // thin) + j) & 15], axis=1))
    return np.unique(np.concatenate(parts).astype(np.int64), axis=0)


def length_sweep(bounds, seed):
    """The frames of length_requests(bounds) in a seeded random order (so every
    tile mixes short and long frames), ihl 5, packed back to back in the
    unaligned (base | off << 48) layout; gaps and payload random, so a write
    outside a frame shows in the whole-UMEM comparison."""
    rng = np.random.default_rng(seed)
    req = length_requests(tuple(bounds))
    req = req[rng.permutation(req.shape[0])]
    return _packed(req[:, 0], req[:, 1], rng)


def length_coverage(b, bounds):
    """Counts behind length_sweep's conditions, from the batch alone:
    dense_missing -- (len, start phase) pairs absent among len 0..dense_limit;
    pairs[(B, nch)] -- distinct (start phase, end phase) pairs among the frames
    of nch chunks, for nch in [B - 1, B + 2] (256 = all);
    parities[(B, nch)] -- distinct parities of the UDP start among them;
    not_ihl5 -- frames of 15 bytes or more whose version/ihl byte is not 0x45."""
    start, ln, rs, e, nch = geometry(b)
    lim = dense_limit(bounds)
    dense = np.zeros((lim + 1, 16), bool)
    sel = ln <= lim
    dense[ln[sel], rs[sel]] = True
    pairs, parities = {}, {}
    for bd in bounds:
        for d in AROUND:
            at = nch == bd + d
            pairs[(bd, bd + d)] = int(np.unique(rs[at] * 16 + e[at]).size)
            parities[(bd, bd + d)] = int(np.unique((start[at] + U5) & 1).size)
    has_ihl = ln >= 15
    return dict(dense_missing=int((~dense).sum()), pairs=pairs, parities=parities,
                not_ihl5=int((b.umem[start[has_ihl] + 14] != 0x45).sum()))


# ---- the header sweep -----------------------------------------------------------

HEADER_MAX_LEN = 130


def header_sweep(seed):
    """Every ihl nibble 0..15 x every length 0..130 x every start phase 0..15
    (33,536 frames, all inside the 97-byte header window and a little past it),
    in a seeded random order, packed.  One frame in 8 (two of the 16 start
    phases of every (ihl, length)) is no IPv4 (ethertype
    IPv6, VLAN, ARP) or no UDP (TCP, ICMP, 255), in turn.  The rules of
    checksummer_user.c:34-55 against ihl: `udp + 8 > end` decides at
    len == 14 + 4 ihl + 7 / + 8, which every ihl meets here at every phase."""
    rng = np.random.default_rng(seed)
    ihl, ln, ph = np.meshgrid(np.arange(16), np.arange(HEADER_MAX_LEN + 1), np.arange(16), indexing="ij")
    order = rng.permutation(ihl.size)
    ihl, ln, ph = ihl.ravel()[order], ln.ravel()[order], ph.ravel()[order]
    etypes = np.array([[0x86, 0xDD], [0x81, 0x00], [0x08, 0x06]], dtype=np.uint8)
    protos = np.array([6, 1, 255], dtype=np.uint8)

    def edit(h):
        h[:, 14] = 0x40 | ihl
        k = np.arange(ihl.size)
        odd = (5 * ihl + 3 * ln + ph) % 8 == 3          # 2 of a cell's 16 start phases
        eth = odd & (k // 8 % 2 == 0)
        h[eth, 12:14] = etypes[(k[eth] // 16) % 3]
        pr = odd & ~eth
        h[pr, 23] = protos[(k[pr] // 16) % 3]

    return _packed(ln, ph, rng, edit)


def header_coverage(b):
    """From the batch alone: cells -- distinct (ihl, len, start phase) among the
    frames that hold their ihl byte (len >= 15: 16 x 116 x 16 when complete);
    short_cells -- distinct (len, start phase) among the shorter ones and how
    many frames each has (16 when complete); other -- the share of frames of
    24 bytes or more that are not IPv4/UDP; edge[ihl] -- for each ihl, the start
    phases seen among IPv4/UDP frames at the last length that is dropped and
    the first that is summed: len == 14 + 4 ihl + 7 and + 8 (33 and 34 for ihl < 3)."""
    start, ln, rs, _, _ = geometry(b)
    has = ln >= 15
    ihl = np.zeros(ln.size, dtype=np.int64)
    ihl[has] = b.umem[start[has] + 14] & 15
    cells = np.unique((ihl[has] * 256 + ln[has]) * 16 + rs[has]).size
    sc, cnt = np.unique(ln[~has] * 16 + rs[~has], return_counts=True)
    full = ln >= 24
    plain = np.zeros(ln.size, bool)
    plain[full] = ((b.umem[start[full] + 12] == 0x08) & (b.umem[start[full] + 13] == 0x00) &
                   (b.umem[start[full] + 23] == 17))
    edge = {}
    for i in range(16):
        u = 14 + 4 * i
        first = max(u + 8, 34)          # (ihl < 3: `len < 34` decides first, :43-46)
        edge[i] = tuple(int(np.unique(rs[plain & (ihl == i) & (ln == first - k)]).size) for k in (1, 0))
    return dict(cells=int(cells), short_cells=int(sc.size), short_min=int(cnt.min()), short_max=int(cnt.max()),
                other=float(1.0 - plain[full].mean()), edge=edge)


# ---- the fold sweep -------------------------------------------------------------

FOLD_LENGTHS = {64: (63, 64, 65), 570: (569, 570, 571), 1500: (1499, 1500, 1501), 9000: (8999, 9000, 9001)}
FOLD_CLASSES = {"ffff": 0xFFFF, "10000": 0x10000, "1fffe": 0x1FFFE}
FOLD_ITERS = (1, 2, 7919, -3)      # the counts the batch runs under; -3: zero passes, s is the pseudo-header's
FOLD_TARGETS = [("ffff", 1), ("10000", 1), ("ffff", 2), ("10000", 2), ("ffff", 7919), ("10000", 7919),
                ("1fffe", 7919)]   # (class, the count it is built for)
M32 = (1 << 32) - 1


def _le16_sum(x):
    """Sum of the little-endian 16-bit words of a byte array, a trailing byte low."""
    x = x.astype(np.int64)
    return int(x[0::2].sum()) + 256 * int(x[1::2].sum())


def closed_form(f, iters):
    """(pseudo, P, s) of one ihl-whatever frame that the reference sums (numpy
    statement of csum_device.h's closed form, as oracle.np_packet_processor):
    s = pseudo + max(iters, 0) P mod 2^32 before the fold, P the UDP bytes' word
    sum with the check as 0."""
    u = 14 + 4 * (int(f[14]) & 15)
    le = lambda i: int(f[i]) | int(f[i + 1]) << 8          # noqa: E731
    pseudo = le(26) + le(28) + le(30) + le(32) + 0x1100 + le(u + 4)
    body = f[u:].copy()
    body[6:8] = 0
    p = _le16_sum(body)
    return pseudo, p, (pseudo + max(int(iters), 0) * p) & M32


def _words_with_sum(rng, n, total):
    """n random 16-bit words that sum to `total` (0 <= total <= 65535 n)."""
    w = rng.integers(0, 65536, n).astype(np.int64)
    d = int(total) - int(w.sum())
    sign = 1 if d > 0 else -1
    room = (65535 - w) if d > 0 else w
    if d:
        w += sign * (room * abs(d) // max(int(room.sum()), 1))
        left = abs(int(total) - int(w.sum()))
        room = (65535 - w) if d > 0 else w
        w[np.flatnonzero(room > 0)[:left]] += sign
    assert int(w.sum()) == int(total) and w.min() >= 0 and w.max() <= 65535
    return w


def _fold_frame(rng, length, cls, it):
    """A well-formed frame of `length` bytes whose pre-fold sum under `it`
    iterations has lo + hi == FOLD_CLASSES[cls], by the choice of its last
    aligned 16-bit payload word; None where no such word exists."""
    f = rng.integers(0, 256, size=length, dtype=np.uint8)
    f[:HDR] = frames.headers([length], rng.integers(0, 256, size=1))[0]
    f[26:30] = rng.integers(0, 256, size=4)                  # any source address
    f[40:42] = rng.integers(0, 256, size=2)                  # an old check (the reference clears it)
    k = (length - U5) // 2 - 1                               # the last aligned word: bytes at, at + 1
    at = U5 + 2 * k
    want = FOLD_CLASSES[cls]
    if cls == "1fffe":
        # s = 2^32 - 1: it P = -1 - pseudo (mod 2^32), it odd.  Over every sum A of the
        # source address's two words, the P that solves it; keep an A whose P the
        # frame's free words (4 .. k) can make, then make it.
        assert it % 2 == 1
        inv = pow(it, -1, 1 << 32)
        f[at:at + 2] = 0
        f[26:30] = 0
        pseudo0, _, _ = closed_form(f, it)
        fixed = _le16_sum(f[U5:U5 + 6]) + (int(f[length - 1]) if (length - U5) % 2 else 0)
        nfree = k - 3
        a = np.arange(0, 2 * 65535 + 1, dtype=np.uint64)
        pstar = (((np.uint64(M32) - np.uint64(pseudo0) - a) & np.uint64(M32)) * np.uint64(inv)) & np.uint64(M32)
        ok = np.flatnonzero((pstar >= fixed + 65535 * nfree // 10) & (pstar <= fixed + 65535 * nfree * 9 // 10))
        if ok.size == 0:
            return None
        j = int(ok[rng.integers(0, ok.size)])
        a0 = int(rng.integers(max(0, j - 65535), min(65535, j) + 1))
        f[26:30] = [a0 & 255, a0 >> 8, (j - a0) & 255, (j - a0) >> 8]
        w = _words_with_sum(rng, nfree, int(pstar[j]) - fixed)
        f[U5 + 8:at + 2] = np.stack([w & 255, w >> 8], axis=1).astype(np.uint8).ravel()
    else:
        f[at:at + 2] = 0
        pseudo, p0, _ = closed_form(f, it)
        w = np.arange(65536, dtype=np.uint64)
        s = (np.uint64(pseudo) + np.uint64(max(it, 0)) * (np.uint64(p0) + w)) & np.uint64(M32)
        hit = np.flatnonzero((s & np.uint64(0xFFFF)) + (s >> np.uint64(16)) == np.uint64(want))
        if hit.size == 0:
            return None
        v = int(hit[rng.integers(0, hit.size)])
        f[at:at + 2] = [v & 255, v >> 8]
    _, _, s = closed_form(f, it)
    assert (s & 0xFFFF) + (s >> 16) == want
    return f


def fold_sweep(seed):
    """Frames at a few lengths per size class (FOLD_LENGTHS), at even and odd
    starts, whose last aligned payload word puts the reference's pre-fold sum s
    = hi << 16 | lo in each class of FOLD_TARGETS under that target's iteration
    count: lo + hi == 0xFFFF (the check is 0x0000), == 0x10000 (the fold's
    carry is dropped: the check is 0xFFFF), == 0x1FFFE (s = 2^32 - 1: the check
    is 0x0001 where a second fold would give 0x0000).  The
    longer frames' sums wrap past 2^32 under 7919 iterations; under -3 (zero
    passes) s is the pseudo-header's sum alone.  Run it under every count of
    FOLD_ITERS; fold_classes says what each frame is under each."""
    rng = np.random.default_rng(seed)
    made, phases = [], []
    for lens in FOLD_LENGTHS.values():
        for length in lens:
            for cls, it in FOLD_TARGETS:
                for parity in (0, 1):
                    f = _fold_frame(rng, length, cls, it)
                    if f is not None:
                        made.append(f)
                        phases.append(parity + 2 * int(rng.integers(0, 8)))
    order = rng.permutation(len(made))
    made, phases = [made[i] for i in order], [phases[i] for i in order]
    lens = np.array([f.size for f in made], dtype=np.int64)
    starts, total = _layout(lens, phases)
    umem = rng.integers(0, 256, size=total, dtype=np.uint8)
    for s, f in zip(starts.tolist(), made):
        umem[s:s + f.size] = f
    return frames.HostBatch(umem, _descs(starts, lens), "unaligned")


def fold_classes(b, iters):
    """Per frame of a fold batch under `iters`, from the inputs: lo + hi of the
    pre-fold sum, whether pseudo + iters P passed 2^32, the start's parity, and
    the frame's size class."""
    start, ln, _, _, _ = geometry(b)
    t = np.zeros(b.n, dtype=np.int64)
    wrapped = np.zeros(b.n, bool)
    for i in range(b.n):
        pseudo, p, s = closed_form(b.umem[start[i]:start[i] + ln[i]], iters)
        t[i] = (s & 0xFFFF) + (s >> 16)
        wrapped[i] = pseudo + max(int(iters), 0) * p > M32
    size = np.array([min(FOLD_LENGTHS, key=lambda c: abs(c - int(x))) for x in ln])
    return t, wrapped, start & 1, size


def written_checks(b, umem_after):
    """The 16-bit check (little-endian, as the reference stores it) each ihl-5
    frame of 42 bytes or more holds in umem_after."""
    start = b.frame_offsets().astype(np.int64)
    return umem_after[start + 40].astype(np.int64) | umem_after[start + 41].astype(np.int64) << 8
