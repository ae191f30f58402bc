"""Frames, ACLs and the model for the firewall NF's tests (tests/test_firewall.py,
tests/test_gpu_firewall.py).

The model is written from the rules in include/xsknf_gpu.h ("the firewall NF"),
with a Python dict as the map: 13 key bytes -> action, the last rule of a key
winning.  It shares no code with xsknf_amd/csrc; the descriptor rules are
restated here on purpose, as in the other *_cases modules.
"""
import os
import re

import numpy as np

from xsknf_amd import firewall, frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "firewall_golden.npz")
ACTIONS = (-1, 0, 1, 2, 31, 0x7fffffff, -7)
LENGTHS = ("0", "13", "14", "33", "34", "n+3", "n+4", "n+7", "n+8", "n+19", "n+20", "n+21")
PROTOS = (6, 17, 1)


def code_constant(pattern, name="kernel_firewall.h"):
    """A number the kernel's source states, by pattern."""
    src = open(os.path.join(ROOT, "xsknf_amd", "csrc", name)).read()
    return int(re.search(pattern, src).group(1))


# ---- the model ---------------------------------------------------------------

def rule_key(r) -> bytes:
    """The 13 key bytes of a RULE_DTYPE record, as they lie in a frame."""
    return (int(r["saddr"]).to_bytes(4, "little") + int(r["daddr"]).to_bytes(4, "little") +
            int(r["sport"]).to_bytes(2, "little") + int(r["dport"]).to_bytes(2, "little") + bytes([int(r["proto"])]))


def acl_dict(rules) -> dict:
    d = {}
    for r in rules:
        d[rule_key(r)] = int(r["action"])
    return d


def rules_dict_fast(rules) -> dict:
    """acl_dict for a million rules: the keys cut from the records' own bytes."""
    raw = np.ascontiguousarray(rules).view(np.uint8).reshape(-1, 20)
    keys = np.ascontiguousarray(raw[:, :13]).tobytes()
    act = rules["action"].tolist()
    return {keys[13 * i:13 * i + 13]: act[i] for i in range(len(act))}


def frame_key(f: bytes):
    """(verdict, None) where rules 1-5 decide, else (None, key)."""
    n = len(f)
    if n < 14:
        return -1, None
    if f[12:14] != b"\x08\x00":
        return 0, None
    if n < 34:
        return -1, None
    nxt = 14 + 4 * (f[14] & 15)
    proto = f[23]
    if proto == 6:
        if nxt + 20 > n:
            return -1, None
    elif proto == 17:
        if nxt + 8 > n:
            return -1, None
    else:
        return 0, None
    return None, bytes(f[26:34]) + bytes(f[nxt:nxt + 4]) + bytes([proto])


def model(umem, descs, acl: dict) -> np.ndarray:
    size = int(umem.size)
    buf = umem.tobytes()
    out = np.empty(descs.shape[0], dtype=np.int32)
    for i, (addr, ln) in enumerate(zip(descs["addr"].tolist(), descs["len"].tolist())):
        off = (addr & ((1 << 48) - 1)) + (addr >> 48)
        if not (off <= size and ln <= size - off):
            out[i] = -1
            continue
        v, key = frame_key(buf[off:off + ln])
        out[i] = acl.get(key, 0) if v is None else v
    return out


def keys_of(umem, descs):
    """The lookup key of every frame that reaches the map (None for the others)."""
    buf = umem.tobytes()
    out = []
    for addr, ln in zip(descs["addr"].tolist(), descs["len"].tolist()):
        off = (addr & ((1 << 48) - 1)) + (addr >> 48)
        out.append(frame_key(buf[off:off + ln])[1] if off + ln <= len(buf) else None)
    return out


def rules_from_keys(keys, actions) -> np.ndarray:
    r = np.zeros(len(keys), dtype=firewall.RULE_DTYPE)
    if len(keys):
        raw = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 13)
        r.view(np.uint8).reshape(-1, 20)[:, :13] = raw
        r["action"] = np.asarray(actions, dtype=np.int64).astype(np.int32)
    return r


def neighbours(key: bytes):
    """The 104 keys one bit away."""
    k = int.from_bytes(key, "little")
    return [(k ^ (1 << b)).to_bytes(13, "little") for b in range(104)]


# ---- frames and batches --------------------------------------------------------

def make_frame(rng, length, ihl=5, proto=17, ipv4=True) -> bytes:
    """`length` random bytes with the fields the rules read set where they exist."""
    f = bytearray(rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    if length >= 14:
        f[12:14] = b"\x08\x00" if ipv4 else (b"\x86\xdd" if rng.integers(2) else b"\x08\x06")
    if length > 14:
        f[14] = (int(rng.integers(16)) << 4) | ihl
    if length > 23:
        f[23] = proto
    return bytes(f)


def length_of(name: str, ihl: int) -> int:
    return int(name) if name[0] != "n" else 14 + 4 * ihl + int(name[2:])


def pack_unaligned(frame_list, rng, phases=None, max_gap=40, tail=0):
    """Frames one after another in the `base | off << 48` layout with random
    gaps; frame i starts at phase phases[i] (mod 16) where given.  tail: bytes
    after the last frame (0: it ends on the UMEM's last byte)."""
    pos, starts = 0, []
    for i, f in enumerate(frame_list):
        pos += int(rng.integers(0, max_gap + 1))
        if phases is not None:
            pos += (phases[i] - pos) % 16
        starts.append(pos)
        pos += len(f)
    umem = rng.integers(0, 256, pos + tail, dtype=np.uint8)
    descs = np.zeros(len(frame_list), dtype=frames.DESC_DTYPE)
    for i, (s, f) in enumerate(zip(starts, frame_list)):
        umem[s:s + len(f)] = np.frombuffer(f, dtype=np.uint8)
        o = int(rng.integers(0, min(s, 0xffff) + 1))
        descs[i] = ((s - o) | (o << 48), len(f), int(rng.integers(1 << 32)))
    return umem, descs


def pack_aligned(frame_list, rng, chunk=2048):
    """The aligned layout: frame i at a random headroom inside chunk i."""
    umem = rng.integers(0, 256, chunk * len(frame_list), dtype=np.uint8)
    descs = np.zeros(len(frame_list), dtype=frames.DESC_DTYPE)
    for i, f in enumerate(frame_list):
        s = chunk * i + int(rng.integers(0, chunk - len(f) + 1))
        umem[s:s + len(f)] = np.frombuffer(f, dtype=np.uint8)
        descs[i] = (s, len(f), 0)
    return umem, descs


def decision_frames(rng, phases=range(16)):
    """ihl x protocol x ethertype x length x phase: (frames, phases)."""
    fl, ph = [], []
    for ihl in range(16):
        for proto in PROTOS:
            for ipv4 in (True, False):
                for ln in LENGTHS:
                    for p in phases:
                        fl.append(make_frame(rng, length_of(ln, ihl), ihl, proto, ipv4))
                        ph.append(p)
    return fl, ph


def with_outside(umem, descs, rng):
    """Descriptors outside the UMEM directly before and after in-range ones:
    past the end by a byte, starting at the end with a length, far away, and
    with a length that would wrap a 32- or 64-bit sum."""
    size = int(umem.size)
    bad = [(size - 10, 11), (size, 1), (size + 1, 0), (1 << 47, 64), ((1 << 48) - 1, 64), (size - 1, 0xffffffff),
           (((1 << 48) - 1) | (0xffff << 48), 64), (0, size + 1)]
    out = []
    k = 0
    for i in range(descs.shape[0]):
        out.append(tuple(descs[i]))
        if i % 3 == 0:
            out.append((bad[k % len(bad)][0], bad[k % len(bad)][1], 7))
            k += 1
    return np.array(out, dtype=frames.DESC_DTYPE)


def lookup_frames(rng, n, lo=54, hi=130):
    """n well-formed TCP / UDP frames that all reach the map (mixed ihl)."""
    fl = []
    for i in range(n):
        ihl = int(rng.choice([5, 5, 5, 6, 15, 0, 3]))
        proto = 6 if i % 2 else 17
        need = 14 + 4 * ihl + (20 if proto == 6 else 8)
        fl.append(make_frame(rng, int(rng.integers(max(lo, need, 34), max(hi, need) + 1)), ihl, proto, True))
    return fl


def hit_miss_acl(keys, rng):
    """The rules of the hits-and-near-misses test over the frames' keys: the
    exact key for frames 0, 3, 6 ... (actions cycling through ACTIONS), the 104
    one-bit neighbours but not the key for frames 1, 4, 7 ..., nothing for the
    rest.  A neighbour that happens to be another frame's key is left out."""
    real = {k for k in keys if k is not None}
    rk, ra = [], []
    j = 0
    for i, k in enumerate(keys):
        if k is None:
            continue
        if i % 3 == 0:
            rk.append(k)
            ra.append(ACTIONS[j % len(ACTIONS)])
            j += 1
        elif i % 3 == 1:
            for nb in neighbours(k):
                if nb not in real:   # (the 8 with another protocol can never match: the builder may drop them)
                    rk.append(nb)
                    ra.append(int(rng.integers(1, 30)))
    return rules_from_keys(rk, ra)


def random_rules(rng, n) -> np.ndarray:
    r = np.zeros(n, dtype=firewall.RULE_DTYPE)
    r["saddr"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["daddr"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["sport"] = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    r["dport"] = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    r["proto"] = np.where(rng.integers(0, 2, n) == 1, 6, 17)
    r["action"] = rng.integers(-1, 32, n)
    return r


def frames_for_rules(rules, rng, flip=False):
    """One 64-byte frame (ihl 5) per rule carrying its key; flip: one random bit
    of saddr / daddr / the ports flipped, so that the key is (almost surely) absent."""
    n = rules.shape[0]
    fr = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    raw = np.ascontiguousarray(rules).view(np.uint8).reshape(-1, 20)
    fr[:, 12], fr[:, 13], fr[:, 14] = 8, 0, 0x45
    fr[:, 23] = raw[:, 12]
    fr[:, 26:34] = raw[:, 0:8]
    fr[:, 34:38] = raw[:, 8:12]
    if flip:
        bit = rng.integers(0, 96, n)
        col = np.where(bit < 64, 26 + bit // 8, 34 + (bit - 64) // 8)
        fr[np.arange(n), col] ^= (1 << (bit % 8)).astype(np.uint8)
    descs = np.zeros(n, dtype=frames.DESC_DTYPE)
    descs["addr"] = np.arange(n, dtype=np.uint64) * 64
    descs["len"] = 64
    return fr.reshape(-1), descs


def million_case(seed=1001, n_rules=1000000, n_look=65536):
    """The 1,000,000-rule ACL with n_look hits and n_look misses: (rules, umem,
    descs, expected verdicts by the dict)."""
    rng = np.random.default_rng(seed)
    rules = random_rules(rng, n_rules)
    d = rules_dict_fast(rules)
    pick = rng.integers(0, n_rules, n_look)
    hu, hd = frames_for_rules(rules[pick], rng)
    mu, md = frames_for_rules(rules[pick], rng, flip=True)
    umem = np.concatenate([hu, mu])
    md = md.copy()
    md["addr"] += hu.size
    descs = np.concatenate([hd, md])
    raw = umem.reshape(-1, 64)
    keys = np.concatenate([raw[:, 26:34], raw[:, 34:38], raw[:, 23:24]], axis=1).tobytes()
    want = np.array([d.get(keys[13 * i:13 * i + 13], 0) for i in range(2 * n_look)], dtype=np.int32)
    return rules, umem, descs, want


def full_table_case(seed=77, slots=1024):
    """slots - 1 distinct rules in `slots` slots, slots - 1 hits and as many misses."""
    rng = np.random.default_rng(seed)
    rules = random_rules(rng, slots - 1)
    assert len(acl_dict(rules)) == slots - 1
    hu, hd = frames_for_rules(rules, rng)
    mu, md = frames_for_rules(rules, rng, flip=True)
    md = md.copy()
    md["addr"] += hu.size
    return rules, np.concatenate([hu, mu]), np.concatenate([hd, md])


def acl_text(rules) -> str:
    """The reference's file format for RULE_DTYPE records."""
    lines = [str(len(rules))]
    for r in rules:
        sa = ".".join(str(b) for b in int(r["saddr"]).to_bytes(4, "little"))
        da = ".".join(str(b) for b in int(r["daddr"]).to_bytes(4, "little"))
        sp = int.from_bytes(int(r["sport"]).to_bytes(2, "little"), "big")
        dp = int.from_bytes(int(r["dport"]).to_bytes(2, "little"), "big")
        act = "DROP" if int(r["action"]) == -1 else str(int(r["action"]))
        lines.append(f"{sa} {da} {sp} {dp} {'TCP' if int(r['proto']) == 6 else 'UDP'} {act}")
    return "\n".join(lines) + "\n"


def golden_inputs(seed=20261):
    """The fixture's frames and ACL (tests/golden/firewall_golden.npz holds
    them as data together with the reference function's verdicts; this is how
    they were drawn): every branch of rules 1-7 at phases 0, 5, 11, 15, and
    lookups of which a third hit, a third have only one-bit neighbours in the
    ACL and a third are absent; actions that fit the file format's 4 characters."""
    rng = np.random.default_rng(seed)
    fl, ph = decision_frames(rng, phases=(3,))
    ph = [int(rng.choice([0, 5, 11, 15])) for _ in fl]
    look = lookup_frames(rng, 1500, hi=110)
    fl += look
    ph += [int(rng.integers(16)) for _ in look]
    umem, descs = pack_unaligned(fl, rng, ph, max_gap=12)
    keys = keys_of(umem, descs)
    real = {k for k in keys if k is not None}
    rk, ra = [], []
    acts = (-1, 0, 1, 2, 31, 9999, -7)
    j = 0
    for i, k in enumerate(keys):
        if k is None:
            continue
        if i % 3 == 0:
            rk.append(k)
            ra.append(acts[j % len(acts)])
            j += 1
        elif i % 3 == 1 and i % 45 == 1:
            for nb in neighbours(k)[:96]:   # (the protocol bits would leave TCP / UDP)
                if nb not in real:
                    rk.append(nb)
                    ra.append(int(rng.integers(1, 30)))
    # duplicates: the first 20 keys again, earlier in the file, with other actions
    dup = rules_from_keys(rk[:20], [5] * 20)
    rules = np.concatenate([dup, rules_from_keys(rk, ra)])
    return umem, descs, rules
