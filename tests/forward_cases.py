"""What tests/test_forward.py (CPU) and tests/test_gpu_forward.py share: an
independent numpy model of the frame forward (include/xsknf_gpu.h, "forwarding
routed frames"), 16-byte aligned arrays, frame layouts that mix the lengths and
every address mod 16, and the comparison of destination UMEMs with the model --
every byte, the sentinels outside the frames included."""
import numpy as np

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


def model(rx, dst_sizes, tx, counts):
    """The header's contract by per-entry slice assignment.  dst_sizes[i]: the
    size of interface i's own UMEM, or None where it shares the rx UMEM.
    Returns (sentinel-filled destinations with the frames in them, or None;
    stats)."""
    dsts = [None if s is None else np.full(s, SENTINEL8, dtype=np.uint8) for s in dst_sizes]
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
