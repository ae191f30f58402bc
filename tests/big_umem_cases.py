"""One UMEM layout for tests/test_big_umem.py (CPU) and tests/test_gpu_big_umem.py:
a batch whose frames lie around byte 2^32 of a UMEM of S = 2^32 + 8 MiB bytes,
so that a frame offset cut to 32 bits, or taken through a signed 32-bit
intermediate, gives a wrong verdict or a wrong byte instead of passing.

    the decoy   [0, 8 MiB)              for every frame [lo, hi) wholly past 2^32 the bytes
                                        [lo - 2^32, hi - 2^32): another frame of the same length
                                        (ethertype, protocol or one 5-tuple bit flipped, the 12 MAC
                                        bytes a canary).  A truncated offset reads or writes it.
    the window  [2^32 - 8192, 2^32 + W) the batch.  Frames below 2^32 start past 2^31; exactly one
                                        frame, the straddler, starts at 2^32 - k and crosses 2^32.
    the tail    [S - 4096, S)           one frame that ends on the UMEM's last byte: the in-range
                                        neighbours of the descriptors outside the UMEM.
    everything else is zero.

The references are the pure-Python models of the other *_cases modules, run on
`Layout.compact()`: the window and the tail joined into one small array, with the
descriptors rebased onto it (the window starts on a multiple of 4096, so every
address phase is kept; the tail's end is the array's end, so a descriptor is
inside the array exactly when it is inside the UMEM -- which `lay` also checks
against S with Python integers).  This module shares no code with xsknf_amd/csrc.

A descriptor (0, S + 1) does not exist here: a length has 32 bits and S is past
2^32, so every length is inside the UMEM at offset 0.  Its place is taken by
(S + 1 - 0xffffffff, 0xffffffff), the longest frame that ends one byte past S.
"""
import mmap

import numpy as np

from oracle import csum_oracle as O
from tests import firewall_cases as FC
from tests import forward_cases as FWC
from tests import lb_cases as LC
from tests import macswap_cases as MC
from tests import route_cases as RC
from xsknf_amd import frames

B = 1 << 32
S = B + (8 << 20)
HEAD = 8192
WIN = B - HEAD                 # a multiple of 4096
TAIL = 4096
DECOY = S - B                  # the decoy image covers [0, 8 MiB): the window's and the tail's frames - 2^32
MAX_W = 4 << 20
MASK48 = (1 << 48) - 1
CANARY = bytes(range(0xC0, 0xCC))

# ---- the straddler -----------------------------------------------------------
#
# The straddling frame starts at 2^32 - k: byte j of it lies at 2^32 - k + j, so
# 2^32 falls between its bytes k - 1 and k.  A field [a, b) of several bytes is
# crossed when a < k < b; for the one byte 23 both edges are taken (k = 23: the
# byte is the first past 2^32, k = 24: the last before it).  Straddlers have ihl
# 5: the ports word is [34, 38), the UDP check [40, 42), the TCP check [50, 52).
K_FIELDS = [   # (k, the field 2^32 falls in, the straddler's protocol)
    (1, "macs", 17),        # (2^32 - k) % 4 = 3
    (2, "macs", 17),        # 2
    (3, "macs", 17),        # 1
    (4, "macs", 17),        # 0
    (6, "macs", 17),        # between the destination and the source MAC
    (13, "ethertype", 17),
    (23, "proto", 17),
    (24, "proto", 17),
    (25, "ip_check", 17),
    (28, "addresses", 17),  # inside saddr
    (30, "addresses", 17),  # between saddr and daddr
    (32, "addresses", 17),  # inside daddr
    (36, "ports", 17),      # between sport and dport
    (35, "ports", 6),       # inside sport
    (41, "l4_check", 17),
    (51, "l4_check", 6),
]
K_MACS = [k for k, f, _ in K_FIELDS if f == "macs"]
K_COPY = list(range(1, 18))    # the copies: 2^32 at every byte of a frame's first 16-byte chunk and one past it
K_ALL = [(k, p) for k, _, p in K_FIELDS]
K_FEW = [(2, 17), (13, 17), (36, 17), (51, 6)]     # where a second or third run of one NF adds no field
K_CSUM = [41, 1, 16, 17, 33, 69]                   # the UDP check, the first chunk's edges, the payload


def k_ids(ks):
    return [f"k{k}-{'tcp' if p == 6 else 'udp'}" for k, p in ks]


def field_span(f: bytes, name: str):
    """[a, b) of a field within frame f, by the rules' own parse."""
    nxt = 14 + 4 * (f[14] & 15)
    return {"macs": (0, 12), "ethertype": (12, 14), "proto": (23, 24), "ip_check": (24, 26), "addresses": (26, 34),
            "ports": (nxt, nxt + 4), "l4_check": (nxt + 16, nxt + 18) if f[23] == 6 else (nxt + 6, nxt + 8)}[name]


def crossed(k: int, span) -> bool:
    a, b = span
    return k in (a, b) if b - a == 1 else a < k < b


def random_sid(rng, proto):
    return (int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 16)),
            int(rng.integers(1, 1 << 16)), proto)


def straddler(rng, proto=17, sid=None, length=74):
    """A well-formed ihl-5 frame that reaches the map lookups: (frame, its sid)."""
    sid = random_sid(rng, proto) if sid is None else sid
    return LC.frame(rng, sid, length=length, ihl=5), sid


# ---- the layout ----------------------------------------------------------------

def offset_of(addr: int) -> int:
    return (addr & MASK48) + (addr >> 48)


def inside(addr: int, ln: int, size: int = S) -> bool:
    off = offset_of(addr)
    return off <= size and ln <= size - off


def outside_descs():
    """Descriptors outside a UMEM of S bytes, in each way rule 0 names."""
    return [(S - 10, 11), (S, 1), (S + 1, 0), (S - 1, 0xffffffff), (S + 1 - 0xffffffff, 0xffffffff),
            ((S - 13 - 200) | (200 << 48), 14), (1 << 47, 64), (MASK48, 64), (MASK48 | (0xffff << 48), 64)]


def tail_descs(tail_len):
    """Their in-range neighbours: each ends on byte S - 1 (or holds no byte)."""
    return [(S - tail_len, tail_len), (S - 11, 11), (S - 1, 1), (S, 0), ((S - 14 - 200) | (200 << 48), 14)]


def decoy_of(f: bytes, i: int) -> bytes:
    """Another frame of len(f) bytes that a correct parse answers differently."""
    n = len(f)
    if n < 14:      # every rule drops it whatever it holds: only its bytes can differ
        return bytes(b ^ 0xFF for b in f)

    def ethertype(d):
        d[12], d[13] = (0x86, 0xDD) if bytes(d[12:14]) == b"\x08\x00" else (0x08, 0x00)

    def proto(d):
        if n >= 24:
            d[23] = {6: 17, 17: 6}.get(d[23], 6)

    def tuple_bit(d):
        if n >= 34:
            d[26 + i % 8] ^= 1 << (i % 7)

    def long_header(d):
        d[14] |= 15

    flips = [ethertype, proto, tuple_bit]
    flips = flips[i % 3:] + flips[:i % 3]      # the ethertype on some, the protocol on some, a tuple bit on the rest
    tries = [(a,) for a in flips] + [(ethertype, proto), (ethertype, proto, long_header), (proto, long_header)]
    answer = FC.frame_key(f)
    for t in tries:
        d = bytearray(f)
        for flip in t:
            flip(d)
        if FC.frame_key(bytes(d)) != answer:
            break
    else:
        raise AssertionError("no decoy answers differently")
    d[:12] = CANARY
    return bytes(d)


class Layout:
    """win: the window's bytes; tail: the last TAIL bytes; decoy: [0, DECOY);
    descs: the batch; straddler / outside: indices into it."""

    def __init__(self, win, tail, decoy, descs, straddler, outside, k):
        self.win, self.tail, self.decoy, self.descs = win, tail, decoy, descs
        self.straddler, self.outside, self.k = straddler, outside, k

    @property
    def win_end(self):
        return WIN + self.win.size

    def regions(self):
        """(start, bytes) of everything that is not zero."""
        return [(0, self.decoy), (WIN, self.win), (S - TAIL, self.tail)]

    def zero_spans(self):
        return [(DECOY, WIN), (self.win_end, S - TAIL)]

    def rebase(self, descs):
        """The descriptors as plain addresses into compact()'s array."""
        msize = self.win.size + TAIL
        out = np.array(descs, dtype=frames.DESC_DTYPE)
        for i, (addr, ln) in enumerate(zip(descs["addr"].tolist(), descs["len"].tolist())):
            off = offset_of(addr)
            if WIN <= off <= self.win_end and off < S - TAIL:
                new = off - WIN
            elif S - TAIL <= off < S + TAIL:
                new = off - (S - msize)
            else:   # far outside, or so long that it is outside whatever it is rebased to
                assert not inside(addr, ln) and not inside(addr, ln, msize), (hex(addr), ln)
                continue
            assert inside(addr, ln) == inside(new, ln, msize), (hex(addr), ln)
            out["addr"][i] = new
        return out

    def compact(self):
        """(window + tail as one writable array, the batch rebased onto it)."""
        return np.concatenate([self.win, self.tail]), self.rebase(self.descs)

    def split(self, m):
        """compact()'s array after a model ran on it: (window, tail)."""
        return m[:self.win.size], m[self.win.size:]

    def image(self, lo, hi, win=None, tail=None):
        """Bytes [lo, hi) of the UMEM, with the window and the tail as given
        (default: as laid)."""
        out = np.zeros(hi - lo, dtype=np.uint8)
        for at, b in ((0, self.decoy), (WIN, self.win if win is None else win),
                      (S - TAIL, self.tail if tail is None else tail)):
            a, z = max(lo, at), min(hi, at + b.size)
            if a < z:
                out[a - lo:z - lo] = b[a - at:z - at]
        return out

    def other(self, rng):
        """The same places with other bytes: a destination UMEM of the forward."""
        win = rng.integers(0, 256, self.win.size, dtype=np.uint8)
        tail = np.where(self.tail != 0, ~self.tail, 0).astype(np.uint8)
        decoy = np.where(self.decoy != 0, self.decoy ^ 0x5A, 0).astype(np.uint8)
        return Layout(win, tail, decoy, self.descs, self.straddler, self.outside, self.k)


def lay(frame_list, strad: bytes, k: int, rng, *, max_gap=12, phases=None, unaligned=True, tail_frame=None,
        extras=True):
    """frame_list in its order with `strad` put in where 2^32 comes: as many
    frames as fit go below 2^32 - k (random gaps of 0..max_gap bytes, frame i at
    phases[i] mod 16 where given; with max_gap 0 and no phases they end exactly
    at 2^32 - k), then the straddler at 2^32 - k, then the rest.  unaligned:
    addresses as base | offset << 48 with a random split.  extras: the outside
    descriptors and the tail's, spread through the batch."""
    assert 0 < k < len(strad)
    gaps = rng.integers(0, max_gap + 1, len(frame_list)).tolist()

    def walk(items, pos, first):
        starts = []
        for j, f in enumerate(items):
            pos += gaps[first + j]
            if phases is not None:
                pos += (phases[first + j] - pos) % 16
            starts.append(pos)
            pos += len(f)
        return starts, pos

    nb = 0
    while nb < len(frame_list) and walk(frame_list[:nb + 1], 0, 0)[1] <= HEAD - k - 64:
        nb += 1
    rel, used = walk(frame_list[:nb], 0, 0)
    base = B - k - used
    if phases is not None or max_gap:
        base &= ~15
    starts = [base + r for r in rel] + [B - k]
    after, end = walk(frame_list[nb:], B - k + len(strad), nb)
    starts += after
    order = frame_list[:nb] + [strad] + frame_list[nb:]
    wlen = (end - WIN + 64 + 15) & ~15
    assert WIN < starts[0] and wlen - HEAD < MAX_W
    win = rng.integers(0, 256, wlen, dtype=np.uint8)
    decoy = np.zeros(DECOY, dtype=np.uint8)
    rows = []
    for i, (s, f) in enumerate(zip(starts, order)):
        win[s - WIN:s - WIN + len(f)] = np.frombuffer(f, dtype=np.uint8)
        if s >= B:
            decoy[s - B:s - B + len(f)] = np.frombuffer(decoy_of(f, i), dtype=np.uint8)
        o = int(rng.integers(0, 0x10000)) if unaligned else 0
        rows.append(((s - o) | (o << 48), len(f), int(rng.integers(1 << 32))))
    crossing = [i for i, (s, f) in enumerate(zip(starts, order)) if s < B < s + len(f)]
    assert crossing == [nb] and starts[nb] == B - k, "exactly one frame straddles 2^32"
    assert all(s >= 1 << 31 for s in starts)

    tail = np.zeros(TAIL, dtype=np.uint8)
    strad_i, out_i = nb, []
    if extras:
        tf = straddler(rng)[0][:60] if tail_frame is None else tail_frame
        tail[TAIL - len(tf):] = np.frombuffer(tf, dtype=np.uint8)
        decoy[DECOY - len(tf):] = np.frombuffer(decoy_of(tf, 1), dtype=np.uint8)
        decoy[DECOY - 14:DECOY - 2] = np.frombuffer(CANARY, dtype=np.uint8)     # the 14-byte neighbour's
        bad, good = outside_descs(), tail_descs(len(tf))
        assert not any(inside(a, ln) for a, ln in bad) and all(inside(a, ln) for a, ln in good)
        assert all(offset_of(a) + ln == S for a, ln in good)
        extra = [(a, ln, False) for a, ln in bad] + [(a, ln, True) for a, ln in good]
        step = max(1, len(rows) // (len(extra) + 1))
        for j, (a, ln, ok) in enumerate(extra):
            at = min(len(rows), (j + 1) * step + j)
            rows.insert(at, (a, ln, 7))
            strad_i += at <= strad_i
            out_i = [x + (at <= x) for x in out_i]
            if not ok:
                out_i.append(at)
    descs = np.array(rows, dtype=frames.DESC_DTYPE)
    assert descs.shape[0] <= 4096 and offset_of(int(descs["addr"][strad_i])) == B - k
    return Layout(win, tail, decoy, descs, strad_i, np.array(sorted(out_i), dtype=np.int64), k)


# ---- a host UMEM of S bytes ------------------------------------------------------

def host_umem(layout=None):
    """S zero bytes of private anonymous memory (pages are committed only when
    written), with `layout` copied in: (the array, the mapping to close)."""
    mm = mmap.mmap(-1, S, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    u = np.frombuffer(mm, dtype=np.uint8)
    if layout is not None:
        for at, b in layout.regions():
            u[at:at + b.size] = b
    return u, mm


PAGE = mmap.PAGESIZE
RESIDENT_LIMIT = 64 << 20      # the decoy's 8 MiB, the window and the tail, in huge pages at the worst


def resident_pages(u):
    """The indices of the pages of host UMEM u that are in memory (mincore):
    a page that was never written is not."""
    import ctypes
    libc = ctypes.CDLL(None, use_errno=True)
    vec = np.zeros((S + PAGE - 1) // PAGE, dtype=np.uint8)
    rc = libc.mincore(ctypes.c_void_p(u.ctypes.data), ctypes.c_size_t(S), ctypes.c_void_p(vec.ctypes.data))
    assert rc == 0, ctypes.get_errno()
    return np.flatnonzero(vec & 1)


def check_host(u, layout, win, tail, what=""):
    """The three comparisons on a host UMEM: the window (and the tail) equal the
    model's bytes, the decoy is as uploaded, every other byte is zero."""
    wrong = []
    for name, at, want in (("window", WIN, win), ("tail", S - TAIL, tail), ("decoy", 0, layout.decoy)):
        bad = np.flatnonzero(u[at:at + want.size] != want)
        if bad.size:
            wrong.append(f"{bad.size} bytes of the {name} differ, first at {[hex(at + int(x)) for x in bad[:4]]}")
    assert not wrong, f"{what}: " + "; ".join(wrong)
    # every other byte is zero: a page that is not in memory was never written, the others are read
    pages = resident_pages(u)
    assert 0 < pages.size * PAGE < RESIDENT_LIMIT, f"{what}: {pages.size} pages of the UMEM are committed"
    for lo, hi in layout.zero_spans():
        for p in pages[(pages >= lo // PAGE) & (pages <= (hi - 1) // PAGE)].tolist():
            a, b = max(lo, p * PAGE), min(hi, (p + 1) * PAGE)
            assert not u[a:b].any(), f"{what}: a byte was written in [{a:#x}, {b:#x})"


# ---- the batches, shared by the CPU and the GPU tests ------------------------------

def firewall_case(k, proto, seed=0):
    """decision_frames(phases=(3,)) + 300 lookups in the unaligned layout and the
    hit-and-miss ACL over the window's keys; the straddler's key is a hit."""
    rng = np.random.default_rng(7000 + 64 * seed + k)
    fl, ph = FC.decision_frames(rng, phases=(3,))
    look = FC.lookup_frames(rng, 300)
    order = rng.permutation(len(fl) + len(look))
    fl = [(fl + look)[i] for i in order]
    ph = [(ph + [int(rng.integers(16)) for _ in look])[i] for i in order]
    st, sid = straddler(rng, proto)
    L = lay(fl, st, k, rng, phases=ph)
    m, md = L.compact()
    keys = FC.keys_of(m, md)
    assert keys[L.straddler] is not None
    rules = np.concatenate([FC.hit_miss_acl(keys, rng), FC.rules_from_keys([keys[L.straddler]], [31])])
    return L, rules


def session_for(sid, direction, rng, ifaces=4):
    return LC.session(*sid, direction, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)),
                      rng.integers(0, 256, 6).tolist(), int(rng.integers(0, ifaces)))


def lb_case(run, k, proto, seed=0):
    """(layout, backends, (session keys, values)) of one of the three runs:
    "prepopulated": every branch (TCP / UDP, to the backend / the client, ihl 0..15, zero checks)
                    over sessions that were put; the straddler's goes to the client or the backend by k;
    "created":      new flows towards services, the straddler the first frame of one;
    "ordered":      the "existing_b" cause of the ordered path among filler, the straddler prepopulated."""
    rng = np.random.default_rng(8000 + 64 * seed + k + {"prepopulated": 0, "created": 1000, "ordered": 2000}[run])
    if run == "prepopulated":
        fl, _ = LC.sweep_frames(rng, phases=(3,))
        fl = [fl[i] for i in rng.permutation(len(fl))]
        bk = np.zeros(0, dtype=LC.lb.BACKEND_DTYPE)
        ks, vs = LC.sessions_for(fl, rng, every=2)
        st, sid = straddler(rng, proto)
    elif run == "created":
        bk = LC.make_backends(rng)
        fl = LC.flows_batch(rng, bk, flows=150, filler=100)
        ks, vs = np.zeros(0, dtype=LC.lb.KEY_DTYPE), np.zeros(0, dtype=LC.lb.VALUE_DTYPE)
        svc = next(i for i in range(bk.shape[0]) if int(bk[i]["proto"]) == proto)
        st, sid = straddler(rng, proto, LC.service_sid(rng, bk, svc))
    else:
        bk, (ks, vs), fl = LC.ordered_cause(rng, "existing_b")
        fl = fl + [FC.make_frame(rng, int(rng.integers(0, 120)), 5, 1, True) for _ in range(150)]
        st, sid = straddler(rng, proto)
    if run != "created":
        sk, sv = session_for(sid, k % 2, rng)
        ks = np.concatenate([ks, np.array([sk], dtype=LC.lb.KEY_DTYPE)])
        vs = np.concatenate([vs, np.array([sv], dtype=LC.lb.VALUE_DTYPE)])
    L = lay(fl, st, k, rng, max_gap=0)
    return L, bk, (ks, vs)


def gate_for(L, rng):
    """The lbfw gate: a third of the batch's keys with actions cycling through
    FC.ACTIONS, never the straddler's (it is to be rewritten): (rules, dict)."""
    m, md = L.compact()
    keys = FC.keys_of(m, md)
    mine = keys[L.straddler]
    third = [kk for kk in dict.fromkeys(x for x in keys if x is not None) if kk != mine][::3]
    r = FC.rules_from_keys(third, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(third))])
    return r, FC.acl_dict(r)


def macswap_case(k, lens=(14,), n=4000, seed=0):
    """macswap_cases' tight packing: n frames back to back with zero gap, the
    lengths cycling, every byte random; k = 1..4 gives the four bases mod 4."""
    rng = np.random.default_rng(9000 + 64 * seed + 8 * len(lens) + k)
    ln = np.resize(np.asarray(lens, dtype=np.int64), n).tolist()
    fl = [rng.integers(0, 256, x, dtype=np.uint8).tobytes() for x in ln]
    st = rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
    tf = rng.integers(0, 256, 60, dtype=np.uint8).tobytes()
    return lay(fl, st, k, rng, max_gap=0, tail_frame=tf)


def forward_case(k, seed=0):
    """Lengths 0..200 at every start phase mod 16 and three 9000-byte frames, one
    of them the straddler."""
    rng = np.random.default_rng(9500 + 64 * seed + k)
    fl, ph = [], []
    for length in range(201):
        for p in range(16):
            fl.append(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
            ph.append(p)
    for _ in range(2):
        fl.append(rng.integers(0, 256, 9000, dtype=np.uint8).tobytes())
        ph.append(int(rng.integers(16)))
    order = rng.permutation(len(fl))
    fl, ph = [fl[i] for i in order], [ph[i] for i in order]
    st = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    tf = rng.integers(0, 256, 60, dtype=np.uint8).tobytes()
    return lay(fl, st, k, rng, max_gap=5, phases=ph, tail_frame=tf)


def forward_expectation(L, D, nif=2, ingress=1):
    """macswap -> route -> forward by the models on the compact arrays, the
    forward's capacity cutting the window's list in the middle: (rx after,
    verdicts, the route's lists, the capacity, the cut counts, the destination
    after, stats).  L: the rx layout, D: the destination's (L.other)."""
    m, md = L.compact()
    mu, mv = MC.model(m, md, ingress, MC.REDIRECT, False, nif)
    tx, fill, order, counts = RC.model(L.descs, mv, nif)
    live = np.array([WIN <= offset_of(a) < L.win_end for a in tx["addr"].tolist()])
    cap = int(np.flatnonzero(live)[live.sum() // 2])
    cut = FWC.clip_counts(counts, nif, cap)
    dm, _ = D.compact()
    (du, _), stats = FWC.model(mu, [dm.size, None], L.rebase(tx), cut, init=[dm, None])
    assert stats[0] > 1000 and 0 < cap < counts[0]
    return mu, mv, (tx, fill, order, counts), cap, cut, du, stats


def csum_case(seed, k):
    """A small seeded checksummer batch with edge cases, laid around 2^32."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 3000, size=500).astype(np.uint32)
    b = frames.unaligned_batch(500, lens, seed=seed)
    frames.inject_edge_cases(b, 0.1, seed=seed + 1)
    fl = [b.frame(i).tobytes() for i in range(b.n)]
    at = next(i for i in range(8, b.n) if len(fl[i]) >= 1000)
    strad = fl.pop(at)
    return lay(fl, strad, k, rng, max_gap=7)


def oracle_verdicts(L, m, md, **kw):
    """The RFC 1071 oracle in place over the compact array.  It has no rule 0
    (the kernel's rx validation keeps such descriptors from the reference): the
    descriptors outside the UMEM -- judged against S by the layout -- get -1
    and only the others go to it."""
    ok = np.ones(md.shape[0], dtype=bool)
    ok[L.outside] = False
    v = np.full(md.shape[0], -1, dtype=np.int32)
    v[ok] = O.c_process_batch(m, np.ascontiguousarray(md[ok]), **kw)
    return v
