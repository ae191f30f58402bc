"""What tests/test_forward.py (CPU) and tests/test_gpu_forward.py share: an
independent numpy model of the frame forward (include/xsknf_gpu.h, "forwarding
routed frames"), 16-byte aligned arrays, frame layouts that mix the lengths and
every address mod 16, and the comparison of destination UMEMs with the model --
every byte, the sentinels outside the frames included.  For the batches past
one sweep of the device forward's grid: the sweep read from the code, packed
frames built vectorised, the model as a flat scatter, and the counts a capacity
below the tx total leaves."""
import numpy as np

from tests.route_cases import code_constant, code_match
from xsknf_amd import frames

SENTINEL8 = 0xA5                       # every destination byte before a call
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1500, 9000]
CHUNK = 2048
SHIFT = 48
MASK = (1 << SHIFT) - 1


def aligned_u8(n, fill=None):
    """n uint8 at a 16-byte aligned address (a view into a longer array)."""
    raw = np.empty(n + 16, dtype=np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:n]
    assert a.ctypes.data % 16 == 0
    if fill is not None:
        a[:] = fill
    return a


def aligned_descs(n):
    return aligned_u8(16 * n, 0).view(frames.DESC_DTYPE)


def rx_bytes(size, seed):
    """An rx UMEM in which no byte equals the sentinel."""
    a = aligned_u8(size)
    a[:] = np.random.default_rng(seed).integers(0, 0xA5, size, dtype=np.uint8)
    a.setflags(write=False)
    return a


def offset_of(addr):
    """xsknf_rt.c addr_offset, restated."""
    addr = int(addr)
    return (addr & MASK) + (addr >> SHIFT)


def mixed_frames(n, lens=LENS, unaligned=True):
    """n (addr, len) frames in a UMEM of 2 KiB chunks, and the UMEM's size: the
    lengths in turn (so a 9000-byte frame sits among 1-byte ones in every run of
    13), the address mod 16 stepping through all 16 values against them, each
    frame from a chunk of its own onwards.  unaligned: every other address
    carries part of its offset in bits 48 and up."""
    out, chunk = [], 0
    for f in range(n):
        ln = lens[f % len(lens)]
        r = (f // len(lens) + f % len(lens)) % 16
        off = chunk * CHUNK + 16 * (f % 5) + r
        chunk += (off % CHUNK + ln) // CHUNK + 1
        if unaligned and f % 2 and off >= 300:
            delta = 256 + f % 7
            out.append(((off - delta) | (delta << SHIFT), ln))
        else:
            out.append((off, ln))
    return out, max(chunk, 1) * CHUNK


PACKED_LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 64]
PACKED_LONG, PACKED_EVERY = 4200, 4099     # a frame of more than 64 * kUnroll chunks, every 4099th


def grid_sweep():
    """G: the entries one sweep of forward_frames' persistent grid takes, from
    the code: kMaxBlocks blocks of kThreads / 64 waves, a 64-entry tile each.
    Also holds the code to what the long tests lean on: the grid is capped at
    kMaxBlocks, a wave strides by the whole grid's waves, and PACKED_LONG bytes
    are more chunks than one trip of the chunk loop moves."""
    h = "kernel_forward.h"
    blocks = code_constant(h, r"constexpr uint32_t kMaxBlocks = (\d+);")
    threads = code_constant(h, r"constexpr int kThreads = (\d+);")
    wave = code_constant(h, r"constexpr int kWaves = kThreads / (\d+);")
    tile = code_constant(h, r"const uint64_t e = t \* (\d+) \+ lane;")
    assert wave == 64 and tile == 64
    code_match(h, r"t \+= gridDim\.x \* static_cast<uint64_t>\(kWaves\)")
    code_match("forward_device.hip", r"want < kMaxBlocks \? want : kMaxBlocks")
    unroll = code_constant(h, r"constexpr int kUnroll = (\d+);")
    code_match(h, r"k0 \+= 64ull \* kUnroll")
    assert PACKED_LONG > 64 * unroll * 16
    return blocks * (threads // wave) * tile


def packed_frames(n):
    """(n descriptors, the rx UMEM's size) for the batches past one sweep of the
    forward's grid: the lengths of PACKED_LENS in turn, every PACKED_EVERY-th
    frame PACKED_LONG bytes; frame e + 1 starts e % 3 bytes after frame e's end,
    so neighbours share 16-byte chunks and the starts step through every address
    mod 16; every other address as base | offset << 48.  About 26 bytes a frame."""
    e = np.arange(n, dtype=np.uint64)
    ln = np.array(PACKED_LENS, dtype=np.uint64)[e % np.uint64(len(PACKED_LENS))]
    ln[PACKED_EVERY - 1::PACKED_EVERY] = PACKED_LONG
    step = ln + e % np.uint64(3)
    start = np.cumsum(step, dtype=np.uint64) - step + np.uint64(5)
    delta = np.where((e % np.uint64(2) == 1) & (start >= 300), np.uint64(256) + e % np.uint64(7), np.uint64(0))
    d = aligned_descs(n)
    d["addr"] = (start - delta) | (delta << np.uint64(SHIFT))
    d["len"] = ln.astype(np.uint32)
    d["options"] = 7
    return d, (int((start + ln).max()) + 64 & ~15) if n else 64


def offsets_of(addr):
    """offset_of over an array of addresses."""
    a = np.asarray(addr, dtype=np.uint64)
    return (a & np.uint64(MASK)) + (a >> np.uint64(SHIFT))


def past_sweep(tx, counts, dst_sizes, rx_size, sweep):
    """What a routed batch holds at tx entries of index >= sweep (taken by a
    wave's second or later tile) that the forward copies: (the set of start
    addresses mod 16, the set of lengths, the number of entries)."""
    nif = len(dst_sizes)
    owner = np.repeat(np.arange(nif), counts[:nif])
    lim = np.array([0 if s is None else min(s, rx_size) for s in dst_sizes], dtype=np.uint64)[owner]
    off, ln = offsets_of(tx["addr"][:owner.size]), tx["len"][:owner.size].astype(np.uint64)
    live = (off + ln <= lim) & (lim > 0)
    live[:sweep] = False
    return set((off[live] % np.uint64(16)).tolist()), set(ln[live].tolist()), int(live.sum())


def clip_counts(counts, nif, cap):
    """The per-interface counts of the first `cap` tx entries: what
    xsknf_gpu_forward_frames looks at when its capacity n is below the tx total."""
    out, left = [], int(cap)
    for c in counts[:nif]:
        out.append(min(int(c), left))
        left -= out[-1]
    return out + [0]


def lists(per_if):
    """per_if: one list of (addr, len) per interface -> (tx_descs, counts with
    the drop count 0 after them).  options 0, as the router writes them."""
    flat = [p for l in per_if for p in l]
    tx = aligned_descs(len(flat))
    tx["addr"] = np.array([a for a, _ in flat], dtype=np.uint64)
    tx["len"] = np.array([l for _, l in flat], dtype=np.uint32)
    return tx, [len(l) for l in per_if] + [0]


def deal(frames_, nif):
    """The frames dealt to nif interfaces in turn."""
    return [frames_[i::nif] for i in range(nif)]


def _initial(dst_sizes, init):
    """The destinations before a forward: sentinel-filled, or copies of `init`
    (one array of dst_sizes[i] bytes per interface with a UMEM of its own)."""
    if init is None:
        return [None if s is None else np.full(s, SENTINEL8, dtype=np.uint8) for s in dst_sizes]
    assert all((a is None) == (s is None) and (s is None or a.size == s) for a, s in zip(init, dst_sizes))
    return [None if a is None else np.array(a, dtype=np.uint8) for a in init]


def model(rx, dst_sizes, tx, counts, init=None):
    """The header's contract by per-entry slice assignment.  dst_sizes[i]: the
    size of interface i's own UMEM, or None where it shares the rx UMEM.
    Returns (the destinations -- sentinel-filled, or as `init` gives them --
    with the frames in them, or None; stats)."""
    dsts = _initial(dst_sizes, init)
    st, base = [0, 0, 0], 0
    for i, d in enumerate(dsts):
        c = int(counts[i])
        if d is not None:
            for j in range(base, base + c):
                off, ln = offset_of(tx["addr"][j]), int(tx["len"][j])
                if off <= rx.size and ln <= rx.size - off and off <= d.size and ln <= d.size - off:
                    d[off:off + ln] = rx[off:off + ln]
                    st[0] += 1
                    st[1] += ln
                else:
                    st[2] += 1
        base += c
    return dsts, st


def model_flat(rx, dst_sizes, tx, counts, block=1 << 16, init=None):
    """model() for long lists: the copied entries' bytes by one flat index
    scatter per `block` entries instead of a Python loop per entry.  (model()
    stays the definition; tests/test_forward.py holds this one to it.)"""
    dsts = _initial(dst_sizes, init)
    off, ln = offsets_of(tx["addr"]), tx["len"].astype(np.uint64)      # (off < 2^49, len < 2^32: no wrap below)
    st, base = [0, 0, 0], 0
    for i, d in enumerate(dsts):
        c = int(counts[i])
        if d is not None:
            o, l = off[base:base + c], ln[base:base + c]
            ok = (o + l <= np.uint64(rx.size)) & (o + l <= np.uint64(d.size))
            st[0] += int(ok.sum())
            st[1] += int(l[ok].sum())
            st[2] += c - int(ok.sum())
            o, l = o[ok].astype(np.int64), l[ok].astype(np.int64)
            for s in range(0, o.size, block):
                ob, lb = o[s:s + block], l[s:s + block]
                idx = np.repeat(ob - (np.cumsum(lb) - lb), lb) + np.arange(int(lb.sum()))
                d[idx] = rx[idx]
        base += c
    return dsts, st


def fresh(dst_sizes):
    """Sentinel-filled, aligned destination arrays for forward_host."""
    return [None if s is None else aligned_u8(s, SENTINEL8) for s in dst_sizes]


def same_umems(got, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None
            continue
        bad = np.flatnonzero(np.asarray(g) != w)
        assert bad.size == 0, f"{what}: UMEM of interface {i} differs at {bad[:8]} (of {bad.size})"


def umem_sizes(nif, size):
    """A mix of destinations for nif interfaces over an rx UMEM of `size` bytes:
    own and full-size, shared (None), own and smaller (its far frames are out of
    range), own."""
    small = (size // 2 + 1000) & ~15
    return [(size, None, small, size)[i % 4] for i in range(nif)]
