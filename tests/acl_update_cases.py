"""Cases and the model for the ACL update tests (tests/test_acl_update.py,
tests/test_gpu_acl_update.py): xsknf_gpu_acl_update of include/xsknf_gpu.h.

The model is a Python dict {13 key bytes -> action}, as in tests/firewall_cases.py,
with the ops applied in index order.  A case is (name, slots, initial rules,
calls, expected): calls[i] is an OP_DTYPE array (or, for a call that must be
refused, (ops, errno)), expected[i] the dict after it.  Everything is seeded.
The table's hash is restated here on purpose: the chain cases pick, by brute
force, keys whose home slots collide in a 64-slot table.
"""
import collections
import errno

import numpy as np

from tests import firewall_cases as FC
from xsknf_amd import firewall

SLOTS = 64
PUT, DELETE = firewall.PUT, firewall.DELETE
M32 = 0xffffffff

Case = collections.namedtuple("Case", "name slots rules calls expected")


def tombstone_share():
    """slots / this many tombstones at most outlive an update's deletes (acl_table.h)."""
    return FC.code_constant(r"constexpr uint32_t kAclTombstoneShare = (\d+);", "acl_table.h")


# ---- the hash and the keys -------------------------------------------------------

def acl_hash(a, b, c, p):
    """acl_hash of xsknf_amd/csrc/acl_table.h, restated."""
    h = (a * 0x9E3779B1) & M32
    h ^= h >> 15
    h = ((h ^ b) * 0x85EBCA77) & M32
    h ^= h >> 13
    h = ((h ^ c) * 0xC2B2AE3D) & M32
    h ^= h >> 16
    h = ((h ^ p) * 0x27D4EB2F) & M32
    h ^= h >> 15
    return h


def key_words(key: bytes):
    """{saddr, daddr, sport | dport << 16, proto} of 13 key bytes."""
    return (int.from_bytes(key[0:4], "little"), int.from_bytes(key[4:8], "little"),
            int.from_bytes(key[8:12], "little"), key[12])


def home(key: bytes, slots=SLOTS):
    return acl_hash(*key_words(key)) & (slots - 1)


def random_key(rng) -> bytes:
    return rng.integers(0, 256, 12, dtype=np.uint8).tobytes() + bytes([6 if rng.integers(2) else 17])


def keys_at(rng, slot, n, slots=SLOTS, taken=()):
    """n distinct random keys whose probe starts at `slot`."""
    out, seen = [], set(taken)
    while len(out) < n:
        k = random_key(rng)
        if home(k, slots) == slot and k not in seen:
            seen.add(k)
            out.append(k)
    return out


def keys_away(rng, n, avoid, slots=SLOTS, taken=()):
    """n distinct random keys whose probe starts in none of the slots `avoid`."""
    out, seen = [], set(taken)
    while len(out) < n:
        k = random_key(rng)
        if home(k, slots) not in avoid and k not in seen:
            seen.add(k)
            out.append(k)
    return out


# ---- ops and the model -------------------------------------------------------------

def ops_of(items) -> np.ndarray:
    """OP_DTYPE records from (op, key bytes, action) triples."""
    items = list(items)
    ops = np.zeros(len(items), dtype=firewall.OP_DTYPE)
    if items:
        ops["rule"] = FC.rules_from_keys([k for _, k, _ in items], [a for _, _, a in items])
        ops["op"] = [o for o, _, _ in items]
    return ops


def puts(keys, actions):
    return [(PUT, k, a) for k, a in zip(keys, actions)]


def deletes(keys):
    return [(DELETE, k, 0x5a5a) for k in keys]   # (the action of a DELETE is ignored)


def apply(d: dict, ops) -> dict:
    """The dict after the ops in index order; a key whose protocol is neither 6
    nor 17 never enters."""
    d = dict(d)
    for o in ops:
        k = FC.rule_key(o["rule"])
        if k[12] not in (6, 17):
            continue
        if int(o["op"]) == PUT:
            d[k] = int(o["rule"]["action"])
        else:
            d.pop(k, None)
    return d


def sorted_rules(d: dict) -> np.ndarray:
    """The dict as xsknf_gpu_acl_dump orders it."""
    keys = sorted(d, key=key_words)
    return FC.rules_from_keys(keys, [d[k] for k in keys])


def _case(name, slots, initial, calls):
    """calls: lists of (op, key, action), or (such a list, errno) for a refused call."""
    rules = FC.rules_from_keys([k for k, _ in initial], [a for _, a in initial])
    d = FC.acl_dict(rules)
    out_calls, expected = [], []
    for c in calls:
        if isinstance(c, tuple):
            out_calls.append((ops_of(c[0]) if not isinstance(c[0], np.ndarray) else c[0], c[1]))
        else:
            ops = ops_of(c)
            out_calls.append(ops)
            d = apply(d, ops)
        expected.append(dict(d))
    return Case(name, slots, rules, out_calls, expected)


# ---- the cases -----------------------------------------------------------------------

def chain_cases(seed=4101):
    """Chains of colliding keys in 64 slots; the other slots hold a few keys that
    start elsewhere, so the chains lie exactly where the test puts them."""
    rng = np.random.default_rng(seed)
    out = []
    acts = FC.ACTIONS

    def chain(slot, n=5):
        c = keys_at(rng, slot, n)
        span = {(slot + i) % SLOTS for i in range(-1, n + 3)}
        fill = keys_away(rng, 12, span, taken=c)
        # the fillers' own chains may not run into the span either
        fill = [k for k in fill if all((home(k) + i) % SLOTS not in span for i in range(12))]
        return c, fill

    c, fill = chain(10)
    init = [(k, acts[i % 7]) for i, k in enumerate(c + fill)]
    extra = keys_at(rng, 10, 1, taken=c)[0]
    out.append(_case("delete the middle of a chain of 5", SLOTS, init, [
        deletes([c[2]]),                 # the tail c[3], c[4] lies behind the tombstone
        deletes([c[0]]),                 # and behind two
        puts([extra], [9]),              # takes c[0]'s slot, the first tombstone
        puts([c[2]], [11]),              # back, into its old slot
        deletes([c[4], c[3]]),
    ]))

    c, fill = chain(20)
    init = [(k, acts[i % 7]) for i, k in enumerate(c + fill)]
    out.append(_case("delete and re-put the same key", SLOTS, init, [
        deletes([c[1]]) + puts([c[1]], [21]),            # in one call
        deletes([c[3]]),
        puts([c[3]], [22]),                              # across calls
        puts([c[3]], [23]) + deletes([c[3]]),            # and the other way round
        deletes([c[0]]) + puts([c[0]], [24]) + deletes([c[0]]) + puts([c[0]], [25]),
    ]))

    c, fill = chain(33)
    init = [(k, acts[i % 7]) for i, k in enumerate(c + fill)]
    out.append(_case("a tombstone in front of a live copy of the put key", SLOTS, init, [
        deletes([c[1]]),
        puts([c[3]], [31]),              # c[3] lives two slots behind the tombstone: replaced, not stored twice
        puts([c[4]], [32]) + puts([c[2]], [33]),
        deletes([c[0]]),
        puts([c[4]], [34]),              # two tombstones in front of it now
    ]))

    c, fill = chain(62)                  # slots 62, 63, 0, 1, 2
    init = [(k, acts[i % 7]) for i, k in enumerate(c + fill)]
    more = keys_at(rng, 62, 2, taken=c)
    more63 = keys_at(rng, 63, 1)
    out.append(_case("a chain that wraps from slot 63 to slot 0", SLOTS, init, [
        deletes([c[1], c[2]]),           # slots 63 and 0
        puts([more[0]], [41]),           # into 63
        puts([more63[0]], [42]),         # starts at 63, into 0
        deletes([c[0]]),
        puts([more[1]], [43]) + puts([c[4]], [44]),
        deletes([c[3], c[4], more[0]]),
    ]))
    return out


def capacity_cases(seed=4102):
    rng = np.random.default_rng(seed)
    keys = keys_away(rng, SLOTS + 4, ())
    full, spare = keys[:SLOTS - 1], keys[SLOTS - 1:]
    init = [(k, 1 + i) for i, k in enumerate(full)]
    return [_case("slots - 1 live keys", SLOTS, init, [
        (puts([spare[0]], [7]), errno.ENOSPC),                               # one more new key
        puts([full[5]], [-1]),                                               # a replace at full capacity
        (puts([full[6]], [8]) + puts([spare[1]], [7]), errno.ENOSPC),        # nothing of a refused call is kept
        deletes([full[7]]) + puts([spare[0]], [70]),                         # one out, one in
        (puts([spare[1], spare[2]], [7, 7]) + deletes([full[8]]), errno.ENOSPC),
        deletes([full[8], full[9]]) + puts([spare[1], spare[2]], [71, 72]),
        deletes(full[10:40]),
        puts(full[10:40], range(100, 130)),
    ])]


def churn_cases(seed=4103):
    """Disjoint key sets put and deleted on 64 slots.  A call whose deletes alone
    pass slots / kAclTombstoneShare must rebuild: the first case has two such
    calls.  The second lets tombstones pile up a few at a time."""
    rng = np.random.default_rng(seed)
    many = SLOTS // tombstone_share() + 1
    keys = keys_away(rng, 30 + 12 * many, ())
    base, rest = keys[:30], keys[30:]
    sets = [rest[i * many:(i + 1) * many] for i in range(12)]
    init = [(k, i - 1) for i, k in enumerate(base + sets[0])]
    calls = [deletes(sets[0]), puts(sets[1], range(many)), deletes(sets[1]), puts(sets[2], range(many)),
             deletes(sets[2][:3]), deletes(sets[2][3:]) + puts(sets[3], range(many))]
    big = _case("deletes past the tombstone bound", SLOTS, init, calls)
    small = [rest[i * 5:(i + 1) * 5] for i in range(24)]
    init = [(k, i - 1) for i, k in enumerate(base + small[0])]
    calls = []
    for i in range(23):
        calls.append(deletes(small[i]))
        calls.append(puts(small[i + 1], [i] * 5))
    return [big, _case("tombstones five at a time", SLOTS, init, calls)]


def order_cases(seed=4104):
    rng = np.random.default_rng(seed)
    k, other, third = keys_away(rng, 3, ())
    odd = k[:12] + bytes([1])            # a protocol the table never holds
    init = [(other, 5)]
    bad = ops_of(puts([third], [6]) + deletes([other]) + puts([k], [7]))
    bad["op"][-1] = 2
    return [_case("the last op on a key wins", SLOTS, init, [
        [(PUT, k, 1), (PUT, k, 2), (DELETE, k, 0), (PUT, k, 3)],
        [(DELETE, k, 0), (PUT, k, 4), (DELETE, k, 9)],
        deletes([k]),                                    # an absent key: no error
        [(PUT, odd, 8), (PUT, other, 6)],                # the odd protocol is left out
        deletes([odd]),                                  # and its DELETE does nothing
        (bad, errno.EINVAL),                             # a bad op at index n - 1: nothing changes
        [],                                              # n == 0
    ])]


def all_cases():
    return chain_cases() + capacity_cases() + churn_cases() + order_cases()


def must_rebuild(case, i) -> bool:
    """Whether call i of `case` deletes more present keys than may stay tombstones."""
    c = case.calls[i]
    if isinstance(c, tuple):
        return False
    before = case.expected[i - 1] if i else FC.acl_dict(case.rules)
    last = {}
    for o in c:
        last[FC.rule_key(o["rule"])] = int(o["op"])
    gone = sum(1 for k, op in last.items() if op == DELETE and k in before)
    return gone > case.slots // tombstone_share()


# ---- probe frames ------------------------------------------------------------------------

def probe_frames(case, seed=4199):
    """(umem, descs, keys): one 64-byte frame for every key the case ever names
    and for six one-bit neighbours of each (the protocol's bits included)."""
    rng = np.random.default_rng(seed)
    keys = {FC.rule_key(r) for r in case.rules}
    for c in case.calls:
        ops = c[0] if isinstance(c, tuple) else c
        keys |= {FC.rule_key(o["rule"]) for o in ops}
    keys = sorted(keys)
    near = []
    for i, k in enumerate(keys):
        nb = FC.neighbours(k)
        near += [nb[(17 * i + 19 * j) % 104] for j in range(5)] + [nb[96 + i % 8]]
    every = keys + near
    umem, descs = FC.frames_for_rules(FC.rules_from_keys(every, [0] * len(every)), rng)
    return umem, descs, every


def verdicts_of(d: dict, keys) -> np.ndarray:
    """The firewall's verdicts over probe_frames' frames by the dict."""
    return np.array([d.get(k, 0) if k[12] in (6, 17) else 0 for k in keys], dtype=np.int32)


# ---- random ops -----------------------------------------------------------------------------

def random_calls(seed=4105, total=20000, universe=200, max_call=160):
    """`total` seeded ops over `universe` keys in calls of random size: yields
    (ops, dict after the call)."""
    rng = np.random.default_rng(seed)
    keys = [random_key(rng) for _ in range(universe)]
    assert len(set(keys)) == universe
    d, done = {}, 0
    while done < total:
        n = min(int(rng.integers(0, max_call + 1)), total - done)
        pick = rng.integers(0, universe, n)
        what = rng.integers(0, 5, n)     # 2 in 5 delete
        ops = ops_of((DELETE if w < 2 else PUT, keys[p], int(a))
                     for p, w, a in zip(pick.tolist(), what.tolist(), rng.integers(-1, 40, n).tolist()))
        d = apply(d, ops)
        done += n
        yield ops, dict(d)


def distinct_new_rules(n, base=0) -> np.ndarray:
    """n rules with n distinct keys (saddr counts up from base + 1), none of them
    in a table that holds only such rules with a smaller saddr."""
    r = np.zeros(n, dtype=firewall.RULE_DTYPE)
    i = np.arange(n, dtype=np.uint64) + np.uint64(base + 1)
    r["saddr"] = i
    r["daddr"] = (i * np.uint64(2654435761)) & np.uint64(M32)
    r["sport"] = i & np.uint64(0xffff)
    r["dport"] = (i >> np.uint64(3)) & np.uint64(0xffff)
    r["proto"] = np.where(i & np.uint64(1), 6, 17)
    r["action"] = (i % np.uint64(37)).astype(np.int64) - 1
    return r
