"""What tests/test_staged_cases.py (CPU) and tests/test_gpu_staged_plan.py share:
a model of XSKNF_GPU_PATH_STAGED's copy plan (stage_frames() in
xsknf_amd/csrc/host_path.hip), one named batch per branch and per edge of a
branch, and rounds that rewrite a batch's frames between submissions.

A STAGED piece reaches its kernel one of four ways (the comment at the head of
host_path.hip, include/xsknf_gpu.h):

  runs               the valid frames, in address order, merge into at most
                     kMaxDmaRuns runs (a frame that starts at most kMergeGap
                     bytes past a run's end joins it); one copy per run, the
                     gap bytes included
  2-D                more runs, the sorted frames at one constant stride > 0,
                     width = max len <= stride and
                     o0 + (k - 1) * stride + width <= umem_size; one 2-D copy of
                     width bytes per frame
  mapped (unsorted)  out of address order with more than kSortMax valid frames:
                     nothing is copied, the kernel works in the mapped host UMEM
  mapped (scattered) more runs and no 2-D shape: as above

A wrong plan does not fault: the kernel sums what the device mirror already
holds.  So every check here is made on frames that CHANGE between the batches
of one context (rounds()), and the byte counters of xsknf_gpu_ctx_get_stats are
held to the model's exact values: they are how a test sees which branch ran.

The model is written from that table and shares no code with csrc; the four
constants and the comparisons it restates are read from host_path.hip, and a
pattern the source no longer holds fails (tests/route_cases.py code_match).
"""
import functools

import numpy as np

from oracle import csum_oracle as O
from tests.route_cases import code_constant, code_match
from xsknf_amd import frames

SRC = "host_path.hip"
RUNS, TWO_D, MAPPED_UNSORTED, MAPPED_SCATTERED = "runs", "2-D", "mapped (unsorted)", "mapped (scattered)"
MIRROR = (RUNS, TWO_D)                 # the kernel reads the device mirror; the host writes the checks
# the numbers of the table above as the contract states them today (the model
# itself uses what the source holds: constants())
TABLE = dict(merge_gap=256, max_runs=8, sort_max=4096, piece=65536)
ADDR_MASK = (1 << frames.OFFSET_SHIFT) - 1
MIN_LEN, MAX_LEN = 60, 1500
UMEM_MAX = 16 << 20
# every batch under the same options: REDIRECT from interface 1 of 3, so the
# forward verdict (2) is neither the parse's 0 nor the drop's -1
NIF, INGRESS = 3, 1
FWD = (INGRESS + 1) % NIF


@functools.lru_cache(maxsize=None)
def constants():
    """kMergeGap, kMaxDmaRuns, kSortMax, kPiece (and kSlots) of host_path.hip."""
    return dict(merge_gap=code_constant(SRC, r"constexpr uint64_t kMergeGap = (\d+);"),
                max_runs=code_constant(SRC, r"constexpr size_t kMaxDmaRuns = (\d+);"),
                sort_max=code_constant(SRC, r"constexpr size_t kSortMax = (\d+);"),
                piece=code_constant(SRC, r"constexpr uint32_t kPiece = (\d+);"),
                slots=code_constant(SRC, r"constexpr int kSlots = (\d+);"))


# The comparisons plan() restates, as the source writes them: `<=` turned into
# `<` (or the reverse) must fail here, not quietly move an edge.
COMPARISONS = (
    r"if \(!xsknf_gpu::in_umem\(off, len, c->umem_size\) \|\| len == 0\) continue;",
    r"if \(off < prev\) sorted = false;",
    r"if \(!sorted && s\.order\.size\(\) > kSortMax\) \{",
    r"if \(!s\.runs\.empty\(\) && off <= s\.runs\.back\(\)\.off \+ s\.runs\.back\(\)\.len \+ kMergeGap\) \{",
    r"if \(end > r\.off \+ r\.len\) r\.len = end - r\.off;",
    r"if \(s\.runs\.size\(\) <= kMaxDmaRuns\) \{",
    r"bool uniform = stride > 0;",
    r"uniform = uniform && width <= stride && o0 \+ \(k - 1\) \* stride \+ width <= c->umem_size;",
    r"c->slot_frames = std::min\(max_batch, kPiece\);",
    r"c->stats\.bytes_h2d \+= sizeof\(xsknf_gpu_desc\) \* n;",
    r"c->stats\.bytes_d2h \+= sizeof\(int32_t\) \* s\.n;",
)


def comparisons_hold():
    for p in COMPARISONS:
        code_match(SRC, p)
    code_match("desc_rules.h", r"return off <= size && len <= size - off;")
    return len(COMPARISONS) + 1


# ---- the model ---------------------------------------------------------------------

def offsets(descs):
    """off = (addr & (2^48 - 1)) + (addr >> 48), as Python-sized integers."""
    a = descs["addr"].astype(np.uint64)
    return ((a & np.uint64(ADDR_MASK)) + (a >> np.uint64(frames.OFFSET_SHIFT))).astype(np.int64)


def valid(descs, umem_size):
    """off <= size, len <= size - off and len > 0."""
    off, ln = offsets(descs), descs["len"].astype(np.int64)
    return (off <= umem_size) & (ln <= umem_size - off) & (ln > 0)


def merged_runs(off, ln, gap):
    """[[off, len]] of the frames (sorted by off) merged where a frame starts at
    most `gap` bytes past the run's end."""
    runs = []
    for o, n in zip(off.tolist(), ln.tolist()):
        if runs and o <= runs[-1][0] + runs[-1][1] + gap:
            runs[-1][1] = max(runs[-1][1], o + n - runs[-1][0])
        else:
            runs.append([o, n])
    return runs


def plan_detail(descs, umem_size):
    """One piece: dict(branch, moved, runs = the merged runs or None (unsorted and
    not sorted), k = valid frames, sorted, stride, width)."""
    K = constants()
    v = valid(descs, umem_size)
    off, ln = offsets(descs)[v], descs["len"].astype(np.int64)[v]
    k = int(off.size)
    in_order = bool(k < 2 or (off[1:] >= off[:-1]).all())
    d = dict(k=k, sorted=in_order, runs=None, stride=None, width=None)
    if not in_order and k > K["sort_max"]:
        return dict(d, branch=MAPPED_UNSORTED, moved=int(ln.sum()))
    at = np.argsort(off, kind="stable")
    off, ln = off[at], ln[at]
    runs = merged_runs(off, ln, K["merge_gap"])
    d["runs"] = runs
    if len(runs) <= K["max_runs"]:
        return dict(d, branch=RUNS, moved=sum(r[1] for r in runs))
    stride, width = int(off[1] - off[0]), int(ln.max())
    d.update(stride=stride, width=width)
    if (stride > 0 and bool((off == off[0] + np.arange(k, dtype=np.int64) * stride).all()) and width <= stride
            and int(off[0]) + (k - 1) * stride + width <= umem_size):
        return dict(d, branch=TWO_D, moved=width * k)
    return dict(d, branch=MAPPED_SCATTERED, moved=int(ln.sum()))


def plan(descs, umem_size):
    """(branch, moved) of one piece."""
    d = plan_detail(descs, umem_size)
    return d["branch"], d["moved"]


def pieces(n, max_batch):
    """[(lo, hi)] of a batch of n descriptors under a context of max_batch."""
    step = min(max_batch, constants()["piece"])
    return [(lo, min(n, lo + step)) for lo in range(0, n, step)]


def counters(descs, umem_size, max_batch):
    """(bytes_h2d, bytes_d2h, [each piece's branch]) one batch adds to the
    context's counters: per piece of n > 0 descriptors 16 * n + moved up, 4 * n
    down."""
    h2d = d2h = 0
    branches = []
    for lo, hi in pieces(int(descs.shape[0]), max_batch):
        b, moved = plan(descs[lo:hi], umem_size)
        h2d += 16 * (hi - lo) + moved
        d2h += 4 * (hi - lo)
        branches.append(b)
    return h2d, d2h, branches


# ---- the expectation ---------------------------------------------------------------

def iters_of(checks):
    """As tests/test_gpu_parity.py test_host_path_bit_exact: zero checks under
    three iterations; with one, a NIC's checks mostly stand (with three every
    one of them would change)."""
    return 1 if checks == "nic" else 3


def expected(umem, descs, checks="zero"):
    """(UMEM, verdicts) of oracle.csum_oracle over the batch's valid frames; an
    invalid descriptor's verdict is -1 and no byte of it is touched (the oracle
    itself, as the reference, trusts its descriptors)."""
    v = valid(descs, umem.size)
    u = umem.copy()
    out = np.full(descs.shape[0], -1, dtype=np.int32)
    if v.any():
        out[v] = O.c_process_batch(u, np.ascontiguousarray(descs[v]), ingress=INGRESS, iters=iters_of(checks),
                                   action=O.REDIRECT, nif=NIF)
    return u, out


def check_positions(umem, descs):
    """Byte offset in the UMEM of the check of every frame the oracle sums
    (checksummer_user.c:34-55: Ethernet, IPv4, 34 bytes, UDP, the UDP header
    where the ihl nibble puts it), -1 for the others."""
    v = valid(descs, umem.size)
    off, ln = offsets(descs), descs["len"].astype(np.int64)
    at = np.full(descs.shape[0], -1, dtype=np.int64)
    for i in np.flatnonzero(v & (ln >= 34)):
        o = int(off[i])
        if umem[o + 12] == 0x08 and umem[o + 13] == 0x00 and umem[o + 23] == 17:
            u = 14 + 4 * (int(umem[o + 14]) & 0x0F)
            if u + 8 <= ln[i]:
                at[i] = o + u + 6
    return at


# ---- building batches --------------------------------------------------------------

def _descs(off, ln, split=None):
    """Descriptors at the given offsets; split: the part of each offset carried
    in the address's upper 16 bits (base | off << 48)."""
    d = np.zeros(len(off), dtype=frames.DESC_DTYPE)
    off = np.asarray(off, dtype=np.uint64)
    hi = np.zeros(len(off), dtype=np.uint64) if split is None else np.minimum(np.asarray(split, dtype=np.uint64), off)
    d["addr"] = (off - hi) | (hi << np.uint64(frames.OFFSET_SHIFT))
    d["len"] = np.asarray(ln, dtype=np.uint32)
    return d


def fill(umem, descs, rng):
    """Redraw every byte of `umem` (gap bytes too) in place, then write a
    well-formed Ethernet / IPv4 / UDP header (random flow and ports) at every
    valid frame of `descs`."""
    umem[:] = rng.integers(0, 256, size=umem.size, dtype=np.uint8)
    v = valid(descs, umem.size)
    off, ln = offsets(descs)[v], descs["len"].astype(np.int64)[v]
    if off.size == 0:
        return
    h = frames.headers(ln, rng.integers(0, 256, size=off.size))
    h[:, 34:38] = rng.integers(0, 256, size=(off.size, 4), dtype=np.uint8)
    cols = np.arange(frames.HDR_LEN, dtype=np.int64)
    idx = off[:, None] + cols[None, :]
    mask = cols[None, :] < ln[:, None]
    umem[idx[mask]] = h[mask]


def _lens(rng, n, lo=MIN_LEN, hi=MAX_LEN):
    return rng.integers(lo, hi + 1, size=n).astype(np.int64)


def _packed(rng, n, lo=MIN_LEN, hi=MAX_LEN):
    """n frames back to back from byte 3 on (odd and even starts), addresses as
    base | off << 48; the UMEM ends 5 bytes after the last frame."""
    ln = _lens(rng, n, lo, hi)
    start = 3 + np.cumsum(ln) - ln
    return _descs(start, ln, split=rng.integers(0, 256, size=n)), int(start[-1] + ln[-1]) + 5


def _umem(size, descs, seed):
    assert size <= UMEM_MAX
    u = np.empty(size, dtype=np.uint8)
    fill(u, descs, np.random.default_rng([seed, 0xF111]))
    return u


def one_run():
    """300 frames packed back to back, in order: one run."""
    d, size = _packed(np.random.default_rng(0x0101), 300)
    return _umem(size, d, 0x0101), d, RUNS


def _groups(groups):
    """5 frames a group: inside a group each frame starts exactly kMergeGap
    bytes past the one before's end (joins), each group kMergeGap + 1 past the
    group before (does not).  The first groups are the same frames whatever
    `groups` is, in a UMEM sized for nine."""
    gap = constants()["merge_gap"]
    ln = _lens(np.random.default_rng(0x0202), 45)
    step = np.where(np.arange(45) % 5 == 0, gap + 1, gap)
    start = 17 + np.cumsum(ln + step) - ln
    size = int(start[-1] + ln[-1]) + 33
    return _descs(start[:5 * groups], ln[:5 * groups]), size


def gap_at():
    """40 frames in 8 groups: exactly kMaxDmaRuns runs."""
    d, size = _groups(8)
    return _umem(size, d, 0x0202), d, RUNS


def gap_over():
    """The same with a ninth group: nine runs, no constant stride."""
    d, size = _groups(9)
    return _umem(size, d, 0x0202), d, MAPPED_SCATTERED


def run_extends():
    """One run of 12 frames in shuffled order: a long frame, a short one right
    behind it, one exactly kMergeGap further, then gaps under it -- the sort must
    restore this sequence, and every frame moves the run's end.  (Frames of a
    batch never overlap and have len > 0, so a sorted frame starts at or past
    every earlier end: `end > r.off + r.len` holds for every frame that joins a
    run, and its other arm is outside what the header defines.)"""
    gap = constants()["merge_gap"]
    ln = np.array([1500, 60, 700, 61, 1499, 64, 65, 570, 60, 1500, 333, 77], dtype=np.int64)
    step = np.array([0, 0, gap, 1, gap - 1, 0, 7, gap, 15, 2, gap, 100], dtype=np.int64)
    start = 64 + np.cumsum(ln + step) - ln
    d = _descs(start, ln)[np.random.default_rng(0x0303).permutation(12)].copy()
    return _umem(int(start[-1] + ln[-1]) + 9, d, 0x0303), d, RUNS


TWO_D_FRAMES, TWO_D_STRIDE = 600, 2048


def _two_d():
    """600 frames at a 2048-byte stride in rx order at headroom 256, lengths
    mixed, the longest (1500) in the middle and the last one 60 bytes."""
    ln = _lens(np.random.default_rng(0x0404), TWO_D_FRAMES)
    ln[TWO_D_FRAMES // 2], ln[-1] = MAX_LEN, MIN_LEN
    return _descs(np.arange(TWO_D_FRAMES, dtype=np.int64) * TWO_D_STRIDE + frames.HEADROOM, ln)


def two_d():
    d = _two_d()
    return _umem(TWO_D_FRAMES * TWO_D_STRIDE, d, 0x0404), d, TWO_D


def two_d_width_is_stride():
    """64 frames at a stride of 1536 from byte 7, one of exactly 1536 bytes; the
    others at most 1000, so each is a run of its own.  The UMEM ends with the
    last frame's slot."""
    ln = _lens(np.random.default_rng(0x0505), 64, MIN_LEN, 1000)
    ln[20] = 1536
    d = _descs(7 + np.arange(64, dtype=np.int64) * 1536, ln)
    return _umem(7 + 64 * 1536, d, 0x0505), d, TWO_D


def two_d_off_stride():
    """two_d with frame 300 one byte off the stride."""
    d = _two_d()
    d["addr"][300] += np.uint64(1)
    return _umem(TWO_D_FRAMES * TWO_D_STRIDE, d, 0x0404), d, MAPPED_SCATTERED


def _two_d_end(d):
    return int(offsets(d)[-1])


def two_d_past_end():
    """two_d in a UMEM that ends with the last frame's 60th byte: the 2-D
    rectangle (width 1500) would pass the UMEM's end, so no 2-D copy."""
    d = _two_d()
    return _umem(_two_d_end(d) + MIN_LEN, d, 0x0404), d, MAPPED_SCATTERED


def two_d_fits_exactly():
    """The same frames in a UMEM that ends with the rectangle's last byte."""
    d = _two_d()
    return _umem(_two_d_end(d) + MAX_LEN, d, 0x0404), d, TWO_D


def _reversed(n):
    """Slots 0 .. n - 1 of kSortMax + 1 slots of 2048 bytes, in descending
    address order; the same frames and UMEM whatever n is."""
    m = constants()["sort_max"] + 1
    ln = _lens(np.random.default_rng(0x0606), m)
    d = _descs(np.arange(m, dtype=np.int64) * 2048 + frames.HEADROOM, ln)
    return d[:n][::-1].copy(), m * 2048


def reversed_sortmax():
    d, size = _reversed(constants()["sort_max"])
    return _umem(size, d, 0x0606), d, TWO_D


def reversed_sortmax_plus_1():
    d, size = _reversed(constants()["sort_max"] + 1)
    return _umem(size, d, 0x0606), d, MAPPED_UNSORTED


def shuffled_small():
    """64 frames in 64 of a 16 MiB UMEM's 8192 chunks, in the order the fill ring
    recycled them; eight of them among the first 16 chunks, where the other
    cases' frames lie (alternating())."""
    rng = np.random.default_rng(0x0707)
    slot = np.concatenate([rng.choice(16, size=8, replace=False), 16 + rng.choice(UMEM_MAX // 2048 - 16, size=56,
                                                                                 replace=False)]).astype(np.int64)
    slot = slot[rng.permutation(64)]
    d = _descs(slot * 2048 + frames.HEADROOM, _lens(rng, 64))
    return _umem(UMEM_MAX, d, 0x0707), d, MAPPED_SCATTERED


def shuffled_packed():
    """300 packed frames permuted: sorted, then one run."""
    rng = np.random.default_rng(0x0808)
    d, size = _packed(rng, 300)
    d = d[rng.permutation(300)].copy()
    return _umem(size, d, 0x0808), d, RUNS


INVALID_KINDS = 5


def _invalid(kind, size):
    """(addr, len) no UMEM of `size` bytes holds: past the end by a byte, len 0,
    addr 2^47, len 2^32 - 1, an `off` part that carries the sum over the top.
    Kinds 1 and 3 lie at byte 0, below every frame; the others above."""
    return [(size - 99, 100), (0, 0), (1 << 47, 100), (0, 0xFFFFFFFF),
            ((size - 100) | (0xFFFF << frames.OFFSET_SHIFT), 60)][kind % INVALID_KINDS]


def invalid_between():
    """gap_at with an invalid descriptor after every third frame, each kind in
    turn: counted, the ones at byte 0 would put the batch out of order, and the
    ones past the end would put the frame after them out of order."""
    g, size = _groups(8)
    rows = []
    for i in range(g.shape[0]):
        rows.append((int(g["addr"][i]), int(g["len"][i])))
        if i % 3 == 2:
            rows.append(_invalid(i // 3, size))
    d = np.zeros(len(rows), dtype=frames.DESC_DTYPE)
    d["addr"] = np.array([r[0] for r in rows], dtype=np.uint64)
    d["len"] = np.array([r[1] for r in rows], dtype=np.uint32)
    return _umem(size, d, 0x0202), d, RUNS


def all_invalid():
    """50 invalid descriptors: no run, nothing moves, every verdict -1."""
    size = 4099
    rows = [_invalid(k, size) for k in range(50)]
    d = np.zeros(50, dtype=frames.DESC_DTYPE)
    d["addr"] = np.array([r[0] for r in rows], dtype=np.uint64)
    d["len"] = np.array([r[1] for r in rows], dtype=np.uint32)
    return _umem(size, d, 0x0909), d, RUNS


def edge_frames():
    """300 packed frames as one_run, a fifth of them turned into the parse's edge
    cases each round (frames.inject_edge_cases: short, non-IPv4, non-UDP, ihl
    0..15, all-0xff payloads).  The case fixes the lengths at 60..kMergeGap: an
    edge case may shrink its frame to nothing, and a longer slot left empty
    would cut the run (only two such frames side by side do here)."""
    d, size = _packed(np.random.default_rng(0x0A0A), 300, MIN_LEN, constants()["merge_gap"])
    return _umem(size, d, 0x0A0A), d, RUNS


def piece_cut():
    """kPiece + 1 frames of 64 bytes in 64-byte slots, in order: two pieces under
    max_batch = kPiece + 1, one run each, the second of one frame."""
    n = constants()["piece"] + 1
    d = _descs(np.arange(n, dtype=np.int64) * 64, np.full(n, 64))
    return _umem(n * 64, d, 0x0B0B), d, RUNS


INTERLEAVED_FRAMES, INTERLEAVED_BATCHES = 1200, 4


def interleaved_packed():
    """1,200 packed frames of 60..kMergeGap / 3 - 1 bytes: the frames j, j + 4,
    j + 8, .. lie at most kMergeGap apart, so each of the four interleaved
    batches is ONE run that covers the other three batches' frames."""
    d, size = _packed(np.random.default_rng(0x0C0C), INTERLEAVED_FRAMES, MIN_LEN, constants()["merge_gap"] // 3 - 1)
    return _umem(size, d, 0x0C0C), d, RUNS


CASES = {
    "one-run": one_run, "gap-at": gap_at, "gap-over": gap_over, "run-extends": run_extends, "2d": two_d,
    "2d-width-is-stride": two_d_width_is_stride, "2d-off-stride": two_d_off_stride, "2d-past-end": two_d_past_end,
    "2d-fits-exactly": two_d_fits_exactly, "reversed-sortmax": reversed_sortmax,
    "reversed-sortmax+1": reversed_sortmax_plus_1, "shuffled-small": shuffled_small,
    "shuffled-packed": shuffled_packed, "invalid-between": invalid_between, "all-invalid": all_invalid,
    "edge-frames": edge_frames, "piece-cut": piece_cut, "interleaved-packed": interleaved_packed,
}
# the cases test_each_case_over_three_rounds takes (the other two have tests of their own)
EACH = [c for c in CASES if c not in ("piece-cut", "interleaved-packed")]
# a new length within the slot each round; every other case fixes its geometry
VARY_LEN = ("one-run", "shuffled-small", "shuffled-packed", "edge-frames")
EDGE = {"edge-frames": 0.2}
# the pairs that differ in one quantity, and the byte count that tells them apart
EDGE_PAIRS = (("gap-at", "gap-over"), ("reversed-sortmax", "reversed-sortmax+1"),
              ("2d-fits-exactly", "2d-past-end"), ("2d", "2d-off-stride"))


@functools.lru_cache(maxsize=None)
def case(name):
    umem, descs, branch = CASES[name]()
    umem.setflags(write=False)
    descs.setflags(write=False)
    return umem, descs, branch


def max_batch(name):
    return constants()["piece"] + 1 if name == "piece-cut" else 4200


# ---- rounds ------------------------------------------------------------------------

class Round:
    """One version of a case: the UMEM to hand in, the descriptors, and the
    oracle's UMEM and verdicts for it."""

    def __init__(self, umem, descs, checks):
        self.umem, self.descs, self.checks = umem, descs, checks
        self.want_umem, self.want_verdicts = expected(umem, descs, checks)
        self.check_at = check_positions(umem, descs)
        for a in (self.umem, self.descs, self.want_umem, self.want_verdicts, self.check_at):
            a.setflags(write=False)

    def same_checks_as(self, prev):
        """The summed frames whose check the oracle leaves as the round before
        left those two bytes: a stale mirror would go unseen there."""
        at = self.check_at[self.check_at >= 0]
        return at[(self.want_umem[at] == prev.want_umem[at]) & (self.want_umem[at + 1] == prev.want_umem[at + 1])]


def rewrite(umem, descs0, rng, *, vary=False, edge=0.0, checks="zero"):
    """Rewrite `umem` in place for the slots of `descs0`: every byte redrawn,
    every valid frame a new header (flow, ports) and payload and, with `vary`, a
    new length within its slot (at most kMergeGap / 2 shorter, and no shorter
    than 60: a packed run stays a run); then a NIC's checks (`nic`), then the
    edge cases over a share `edge` of the valid frames.  Returns the round's
    descriptors."""
    descs = descs0.copy()
    v = valid(descs0, umem.size)
    if vary:
        slot = descs0["len"].astype(np.int64)
        cut = rng.integers(0, constants()["merge_gap"] // 2 + 1, size=slot.size)
        descs["len"] = np.where(v, slot - np.minimum(cut, np.maximum(slot - MIN_LEN, 0)), slot).astype(np.uint32)
    fill(umem, descs, rng)
    if checks == "nic" or edge:
        b = frames.HostBatch(umem, descs[v].copy(), "unaligned")
        if checks == "nic":
            frames.offload_checks_host(b)
        if edge:
            frames.inject_edge_cases(b, edge, seed=int(rng.integers(1 << 31)))
        descs["len"][v] = b.descs["len"]
    return descs


def rounds(name, k, seed, checks="zero"):
    """k versions of a case over the same descriptors' slots.  Each round is
    redrawn until the oracle's check of every summed frame differs from the two
    bytes the round before left there (a 16-bit check repeats by chance once in
    65,536 frames), so no stale copy can give the right answer by luck."""
    umem0, descs0, _ = case(name)
    out = []
    for r in range(k):
        for attempt in range(64):
            rng = np.random.default_rng([seed, r, attempt, checks == "nic"])
            umem = np.empty_like(umem0)
            descs = rewrite(umem, descs0, rng, vary=name in VARY_LEN, edge=EDGE.get(name, 0.0), checks=checks)
            rd = Round(umem, descs, checks)
            if not out or rd.same_checks_as(out[-1]).size == 0:
                break
        else:
            raise AssertionError(f"{name}: round {r} keeps repeating a check of round {r - 1}")
        out.append(rd)
    return out


def no_overlap(descs, umem_size):
    """The valid frames of a batch: no offset twice, no two sharing a byte."""
    v = valid(descs, umem_size)
    off, ln = offsets(descs)[v], descs["len"].astype(np.int64)[v]
    at = np.argsort(off, kind="stable")
    off, ln = off[at], ln[at]
    return bool((off[1:] >= off[:-1] + ln[:-1]).all()) and np.unique(off).size == off.size


# ---- one context, branch after branch ----------------------------------------------

ALTERNATE = ("one-run", "2d", "shuffled-small", "gap-at", "reversed-sortmax+1", "2d")


def alternating(seed, checks="zero", order=ALTERNATE):
    """The batches of `order` on ONE 16 MiB UMEM, each over its own case's
    slots (they overlap: every case starts at the UMEM's head), the UMEM
    rewritten before each.  Returns [(UMEM before the batch, descs, intended
    branch, the oracle's UMEM, its verdicts)]; a case's branch in this larger
    UMEM is its own (only the 2-D bound looks at the size, and it is met with
    room to spare)."""
    steps = []
    for j, name in enumerate(order):
        _, descs0, branch = case(name)
        umem = np.empty(UMEM_MAX, dtype=np.uint8)
        descs = rewrite(umem, descs0, np.random.default_rng([seed, j, 0xA17]), vary=name in VARY_LEN, checks=checks)
        wu, wv = expected(umem, descs, checks)
        steps.append((umem, descs, branch, wu, wv))
    return steps
