"""Batches and the model for the macswap NF's tests (tests/test_macswap.py,
tests/test_gpu_macswap.py) and for its fixture's generator
(tests/golden/make_macswap_golden.py).

The model is written from the rules in include/xsknf_gpu.h ("the macswap NF") on
numpy arrays.  It shares no code with xsknf_amd/csrc; the descriptor rules are
restated here on purpose, as in the other *_cases modules.
"""
import os
import re

import numpy as np

from tests import firewall_cases as FC
from xsknf_amd import frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "macswap_golden.npz")
REDIRECT, DROP, PASS = 0, 1, 2
ACTIONS = (REDIRECT, DROP, PASS)
INGRESS = (0, 1, 2, 3, 0x7fffffff, 0xfffffffe, 0xffffffff)


def code_constant(pattern, name="kernel_macswap.h"):
    """A number the kernel's source states, by pattern."""
    src = open(os.path.join(ROOT, "xsknf_amd", "csrc", name)).read()
    return int(re.search(pattern, src).group(1))


# ---- the model ---------------------------------------------------------------

def offsets(descs) -> np.ndarray:
    addr = descs["addr"].astype(np.uint64)
    return (addr & np.uint64((1 << 48) - 1)) + (addr >> np.uint64(48))


def verdict(action, ingress, nif) -> int:
    """Rule 3 in 32-bit unsigned arithmetic, read back as an int32."""
    if action == DROP:
        return -1
    v = ((ingress + 1) & 0xffffffff) % nif
    return v - (1 << 32) if v >= 1 << 31 else v


def model(umem, descs, ingress=0, action=REDIRECT, double=False, nif=1):
    """(UMEM after the batch, verdicts): rules 0-3 frame by frame."""
    out = umem.copy()
    size = int(umem.size)
    v = np.full(descs.shape[0], -1, dtype=np.int32)
    fwd = verdict(action, ingress, nif)
    for i, (off, ln) in enumerate(zip(offsets(descs).tolist(), descs["len"].tolist())):
        if not (off <= size and ln <= size - off):   # rule 0
            continue
        if ln < 14:                                  # rule 1
            continue
        if not double:                               # rule 2 (twice: as it was)
            dst = out[off:off + 6].copy()
            out[off:off + 6] = out[off + 6:off + 12]
            out[off + 6:off + 12] = dst
        v[i] = fwd
    return out, v


# ---- batches -------------------------------------------------------------------

def descs_of(starts, lens, rng=None) -> np.ndarray:
    d = np.zeros(len(starts), dtype=frames.DESC_DTYPE)
    d["addr"] = np.asarray(starts, dtype=np.uint64)
    d["len"] = np.asarray(lens, dtype=np.uint32)
    if rng is not None:
        d["options"] = rng.integers(0, 1 << 32, len(starts), dtype=np.uint64)
    return d


def packed(rng, n, base, lens=(14,), tail=0):
    """n frames back to back from byte `base` on, their lengths cycling through
    `lens`, every byte random; the last frame ends `tail` bytes before the
    UMEM's end.  With 14-byte frames at an odd base, neighbours' swapped bytes
    share aligned words."""
    ln = np.resize(np.asarray(lens, dtype=np.int64), n)
    starts = base + np.concatenate([[0], np.cumsum(ln)[:-1]])
    umem = rng.integers(0, 256, int(base + ln.sum() + tail), dtype=np.uint8)
    return umem, descs_of(starts, ln, rng)


def phase_sweep(rng, lens=(14, 60)):
    """For every off % 128 in 0..127 one frame of each length, each in a 512-byte
    cell of random canary bytes: the 12 swapped bytes straddle every 4-, 16-,
    64- and 128-byte boundary in every way."""
    starts, ln = [], []
    for k, length in enumerate(lens):
        for p in range(128):
            starts.append(512 * (128 * k + p) + 128 + p)
            ln.append(length)
    umem = rng.integers(0, 256, 512 * 128 * len(lens), dtype=np.uint8)
    order = rng.permutation(len(starts))
    return umem, descs_of(np.asarray(starts)[order], np.asarray(ln)[order], rng)


def unaligned_form(descs, rng):
    """The same frames addressed as base | offset << 48 with a random split."""
    d = descs.copy()
    off = offsets(descs)
    o = np.array([int(rng.integers(0, min(int(s), 0xffff) + 1)) for s in off], dtype=np.uint64)
    d["addr"] = (off - o) | (o << np.uint64(48))
    return d


def outside_descs(size):
    """Descriptors outside a UMEM of `size` bytes, in each way rule 0 names:
    past the end by a byte, starting at the end with a length, starting past the
    end, far away, a length that would wrap a 32- or 64-bit sum, an offset part
    that carries past 2^48, and a frame longer than the UMEM."""
    bad = [(size - 10, 11), (size, 1), (size + 1, 0), (1 << 47, 64), ((1 << 48) - 1, 64), (size - 1, 0xffffffff),
           (((1 << 48) - 1) | (0xffff << 48), 64), (0, size + 1), ((size - 13) | (1 << 48), 14)]
    return np.array([(a, ln, 7) for a, ln in bad], dtype=frames.DESC_DTYPE)


def bounds_case(rng, size=4096 + 13):
    """A UMEM of `size` bytes with a frame at offset 0, a 14-byte frame in its
    last 14 bytes, a 0-byte frame at its end, a few frames between and every
    outside descriptor among them."""
    umem = rng.integers(0, 256, size, dtype=np.uint8)
    inside = descs_of([0, 14, 29, 100, 1001, size - 14 - 61, size - 14, size],
                      [14, 15, 64, 13, 1514, 61, 14, 0], rng)
    out = outside_descs(size)
    rows = []
    for i in range(max(inside.shape[0], out.shape[0])):
        if i < out.shape[0]:
            rows.append(out[i])
        if i < inside.shape[0]:
            rows.append(inside[i])
    return umem, np.array(rows, dtype=frames.DESC_DTYPE)


def uniform(rng, n, length=64):
    """n frames of one length back to back from offset 0."""
    umem = rng.integers(0, 256, n * length, dtype=np.uint8)
    return umem, descs_of(np.arange(n, dtype=np.uint64) * np.uint64(length), np.full(n, length))


def mixed(rng, n=257):
    """n frames of lengths 0..80 (a fifth below 14) at random gaps and phases in
    the base | off << 48 layout, with outside descriptors among them."""
    fl = [rng.integers(0, 256, int(rng.integers(0, 14)) if i % 5 == 0 else int(rng.integers(14, 81)),
                       dtype=np.uint8).tobytes() for i in range(n)]
    umem, descs = FC.pack_unaligned(fl, rng, max_gap=9, tail=3)
    out = outside_descs(umem.size)
    descs[3::29][:out.shape[0]] = out[:descs[3::29].shape[0]]
    return umem, descs


# ---- the fixture ---------------------------------------------------------------

def golden_batches(seed=20262):
    """The fixture's inputs (tests/golden/macswap_golden.npz holds them as data
    with what the reference's function left; this is how they were drawn), as
    (umem, descs, ingress, action, double, nif):
      batch 0   every length 0..20 at every start phase 0..15, lengths 59, 60,
                64, 590, 1500, 1514, random gaps, outside descriptors among
                them, the last frame ending on the UMEM's last byte;
      batch 1   96 frames of 14 bytes back to back from offset 1, then lengths
                cycling 14, 15, 17, 13 from an odd offset on;
      2..25     a small packed batch under every action x swap mode x 1..4
                interfaces, the ingress cycling through INGRESS."""
    rng = np.random.default_rng(seed)
    fl, ph = [], []
    for length in range(21):
        for p in range(16):
            fl.append(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
            ph.append(p)
    for length in (59, 60, 64, 590, 1500, 1514):
        fl.append(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        ph.append(int(rng.integers(16)))
    order = rng.permutation(len(fl))
    fl, ph = [fl[i] for i in order], [ph[i] for i in order]
    fl.append(rng.integers(0, 256, 14, dtype=np.uint8).tobytes())
    ph.append(5)
    u0, d0 = FC.pack_unaligned(fl, rng, ph, max_gap=6)
    d0 = FC.with_outside(u0, d0, rng)
    batches = [(u0, d0, 0, REDIRECT, False, 2)]
    ua, da = packed(rng, 96, 1)
    ub, db = packed(rng, 64, 3, lens=(14, 15, 17, 13))
    db["addr"] += np.uint64(ua.size)
    batches.append((np.concatenate([ua, ub]), np.concatenate([da, db]), 0xffffffff, PASS, False, 3))
    k = 0
    for action in ACTIONS:
        for double in (False, True):
            for nif in (1, 2, 3, 4):
                u, d = packed(rng, 12, k % 4, lens=(14, 13, 20, 14, 16))
                batches.append((u, unaligned_form(d, rng), INGRESS[k % len(INGRESS)], action, double, nif))
                k += 1
    return batches
