"""The model and the case builders for the ACL hit counters' tests
(tests/test_acl_counters.py, tests/test_gpu_acl_counters.py):
xsknf_gpu_acl_counters_* of include/xsknf_gpu.h.

The model is plain Python: the ACL as a dict {13 key bytes -> action}
(tests/firewall_cases.py), a dict {key -> [packets, bytes]} beside it and the
four totals.  A batch goes through firewall_cases.frame_key and the descriptor
rules restated there; an update applies its ops in index order: a PUT of a key
the map holds keeps the key's counters, a DELETE ends them, a PUT of an absent
key starts at 0/0.  A rebuild of the table must change nothing anybody can see:
rebuilt() is the identity.  It shares no code with xsknf_amd/csrc.
"""
import numpy as np

from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from xsknf_amd import firewall, frames

FRAMES, HITS, MISSES, DECIDED = range(4)


class Model:
    def __init__(self, rules):
        self.acl = FC.acl_dict(rules)
        self.ctr = {k: [0, 0] for k in self.acl}
        self.totals = [0, 0, 0, 0]

    def batch(self, umem, descs, verdict_of=None):
        """Counts one batch; returns the firewall's verdicts (verdict_of: None)."""
        size = int(umem.size)
        buf = umem.tobytes()
        out = np.zeros(descs.shape[0], dtype=np.int32)
        for i, (addr, ln) in enumerate(zip(descs["addr"].tolist(), descs["len"].tolist())):
            self.totals[FRAMES] += 1
            off = (addr & ((1 << 48) - 1)) + (addr >> 48)
            if not (off <= size and ln <= size - off):
                self.totals[DECIDED] += 1
                out[i] = -1
                continue
            v, key = FC.frame_key(buf[off:off + ln])
            if key is None:
                self.totals[DECIDED] += 1
                out[i] = v
            elif key in self.acl:
                self.totals[HITS] += 1
                self.ctr[key][0] += 1
                self.ctr[key][1] += ln
                out[i] = self.acl[key]
            else:
                self.totals[MISSES] += 1
        return out

    def update(self, ops):
        for o in ops:
            k = FC.rule_key(o["rule"])
            if k[12] not in (6, 17):
                continue
            if int(o["op"]) == firewall.PUT:
                if k not in self.acl:
                    self.ctr[k] = [0, 0]
                self.acl[k] = int(o["rule"]["action"])
            elif k in self.acl:
                del self.acl[k]
                del self.ctr[k]

    def rebuilt(self):
        """As if the table had been rebuilt: nothing visible changes."""
        return self

    def clear(self):
        for c in self.ctr.values():
            c[0] = c[1] = 0
        self.totals = [0, 0, 0, 0]

    def expected(self):
        """(rules, counters, totals) as Acl.counters returns them."""
        keys = sorted(self.acl, key=UC.key_words)
        c = np.zeros(len(keys), dtype=firewall.COUNTER_DTYPE)
        c["packets"] = [self.ctr[k][0] for k in keys]
        c["bytes"] = [self.ctr[k][1] for k in keys]
        return FC.rules_from_keys(keys, [self.acl[k] for k in keys]), c, np.array(self.totals, dtype=np.uint64)


def check(acl, model, device=False, what=""):
    """One set of acl's counters against the model, and the totals' identities."""
    rules, ctr, totals = acl.counters(device=device)
    wr, wc, wt = model.rebuilt().expected()
    where = f"{what} ({'device' if device else 'host'} set)"
    assert rules.tobytes() == wr.tobytes(), f"{where}: the rules differ"
    bad = np.nonzero((ctr["packets"] != wc["packets"]) | (ctr["bytes"] != wc["bytes"]))[0]
    assert bad.size == 0, f"{where}: {bad.size} counters differ, first {bad[:4]}: {ctr[bad[:4]]} != {wc[bad[:4]]}"
    assert totals.tolist() == wt.tolist(), f"{where}: totals {totals.tolist()} != {wt.tolist()}"
    assert int(totals[FRAMES]) == int(totals[HITS]) + int(totals[MISSES]) + int(totals[DECIDED])
    return rules, ctr, totals


# ---- frames ------------------------------------------------------------------------

def frames_for_keys(keys, rng, stride=128):
    """One ihl-5 frame per key (13 key bytes each, repeats welcome) at `stride`
    bytes from the last, with a random length that holds the TCP header."""
    n = len(keys)
    fr = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    raw = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(-1, 13) if n else np.zeros((0, 13), dtype=np.uint8)
    fr[:, 12], fr[:, 13], fr[:, 14] = 8, 0, 0x45
    fr[:, 23] = raw[:, 12]
    fr[:, 26:38] = raw[:, 0:12]
    descs = np.zeros(n, dtype=frames.DESC_DTYPE)
    descs["addr"] = np.arange(n, dtype=np.uint64) * stride
    descs["len"] = rng.integers(54, stride + 1, n)
    return fr.reshape(-1), descs


def absent_keys(rng, n, taken):
    out, seen = [], set(taken)
    while len(out) < n:
        k = UC.random_key(rng)
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def traffic(rng, keys, n, misses=0.2):
    """n keys drawn from `keys` with a skew (a few rules take most), a share of
    them replaced by keys nobody holds."""
    w = 1.0 / (1 + np.arange(len(keys)))
    pick = rng.choice(len(keys), n, p=w / w.sum())
    out = [keys[i] for i in pick.tolist()]
    gone = absent_keys(rng, int(n * misses), keys)
    for j, k in zip(rng.choice(n, len(gone), replace=False).tolist(), gone):
        out[j] = k
    return out


def interleaved_wave(rng, key, other_keys):
    """64 frames and then 64 more, in the unaligned layout: hits on `key`
    interleaved lane by lane with misses, with frames the parse decides
    (decision_frames) and, through with_outside, with descriptors outside the
    UMEM.  Returns (umem, descs)."""
    dec, _ = FC.decision_frames(rng, phases=(0,))
    dec = [f for f in dec if FC.frame_key(f)[1] is None]
    miss = absent_keys(rng, 64, [key] + list(other_keys))
    fl = []
    for i in range(96):
        if i % 3 == 0:
            u, d = frames_for_keys([key], rng)
            fl.append(u[:int(d["len"][0])].tobytes())
        elif i % 3 == 1:
            fl.append(dec[int(rng.integers(len(dec)))])
        else:
            u, d = frames_for_keys([miss[i % 64]], rng)
            fl.append(u[:int(d["len"][0])].tobytes())
    umem, descs = FC.pack_unaligned(fl, rng, tail=5)
    return umem, FC.with_outside(umem, descs, rng)


# ---- update cases ----------------------------------------------------------------------
# (name, slots, initial keys, steps); a step is ("batch", keys) or ("update", ops
# triples as acl_update_cases.ops_of takes them, must_rebuild).

def update_cases(seed=5101):
    rng = np.random.default_rng(seed)
    S = UC.SLOTS
    out = []
    keys = UC.keys_away(rng, 24, ())
    new = absent_keys(rng, 8, keys)
    init = [(k, i % 5 - 1) for i, k in enumerate(keys)]
    out.append(("replace keeps, delete ends, a new key starts at zero", S, init, [
        ("batch", keys + new), ("batch", keys[:10]),
        ("update", UC.puts(keys[:4], [9] * 4) + UC.deletes(keys[4:8]) + UC.puts(new[:4], [3] * 4), False),
        ("batch", keys + new)]))
    out.append(("delete then put in one call resets, the same slot or not", S, init, [
        ("batch", keys * 2),
        ("update", UC.deletes(keys[:3]) + UC.puts(keys[:3], [7] * 3) +
         UC.puts(keys[3:5], [1] * 2) + UC.deletes(keys[3:5]) + UC.puts(keys[3:5], [2] * 2) +
         UC.deletes(keys[5:6]) + UC.puts(keys[5:6], [4]) + UC.deletes(keys[5:6]), False),
        ("batch", keys)]))
    chain = UC.keys_at(rng, 11, 4)
    late = UC.keys_at(rng, 11, 1, taken=chain)
    init2 = [(k, 5) for k in chain]
    out.append(("a put into a tombstone starts at zero", S, init2, [
        ("batch", chain * 3), ("update", UC.deletes(chain[1:2]), False), ("batch", chain + late),
        ("update", UC.puts(late, [6]), False), ("batch", chain + late + late)]))
    many = S // UC.tombstone_share() + 1
    keys = UC.keys_away(rng, 40, ())
    new = absent_keys(rng, 6, keys)
    init3 = [(k, i) for i, k in enumerate(keys)]
    out.append(("a rebuild past the tombstone bound carries the survivors", S, init3, [
        ("batch", traffic(rng, keys, 200)),
        ("update", UC.deletes(keys[:many]) + UC.puts(new, [8] * 6) + UC.puts(keys[many:many + 3], [-1] * 3) +
         UC.deletes(keys[many + 3:many + 4]) + UC.puts(keys[many + 3:many + 4], [0]), True),
        ("batch", traffic(rng, keys + new, 200))]))
    fill = absent_keys(rng, 24, keys)
    out.append(("a rebuild because no slot would stay empty", S, init3, [
        ("batch", traffic(rng, keys, 200)),
        ("update", UC.deletes(keys[:12]), False), ("batch", keys),
        ("update", UC.puts(fill, range(24)) + UC.puts(keys[12:14], [77] * 2), True),
        ("batch", traffic(rng, keys + fill, 300))]))
    return out


def run_steps(case, make_acl, do_batch, do_update, after):
    """Drive one update case: make_acl(rules, slots) -> acl; do_batch(acl, umem,
    descs); do_update(acl, ops); after(acl, model, step index) when a step is done."""
    name, slots, init, steps = case
    rng = np.random.default_rng(5199)
    rules = FC.rules_from_keys([k for k, _ in init], [a for _, a in init])
    model = Model(rules)
    acl = make_acl(rules, slots)
    acl.counters_enable()
    for i, step in enumerate(steps):
        if step[0] == "batch":
            umem, descs = frames_for_keys(step[1], rng)
            model.batch(umem, descs)
            do_batch(acl, umem, descs)
        else:
            ops = UC.ops_of(step[1])
            gone = len({k for o, k, _ in step[1] if o == firewall.DELETE and k in model.acl}) + acl.info["tombstones"]
            model.update(ops)
            do_update(acl, ops)
            info = acl.info
            if step[2]:   # (its deletes alone would leave tombstones)
                assert gone and info["tombstones"] == 0, f"{name}: step {i} did not rebuild"
            assert info["rules"] == len(model.acl)
        after(acl, model, i)
    return acl, model
