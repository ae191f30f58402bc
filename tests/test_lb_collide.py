"""The load balancer's host model (xsknf_gpu_lb_host, xsknf_gpu_lbfw_host) against
the dict models of tests/lb_cases.py and tests/lbfw_cases.py on keys chosen by
their home slot (tests/lb_collide_cases.py): session tables of the smallest
size the builder accepts, chains hundreds of slots long that wrap from the last
slot to slot 0, every stored key hit, near misses that run to a chain's end,
and the capacity boundary.  The device tests (tests/test_gpu_lb_collide.py)
compare against the host model, and both sides share lb_table.h's probe: only
the dict model sees a fault in it.  Each test asserts its premise with the
chain model.  No GPU."""
import re

import numpy as np

from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lbfw_cases as WC
from xsknf_amd import lb, lbfw
from xsknf_amd.firewall import Acl

I, NIF = CC.INGRESS, CC.NIF


def test_the_probes_start_where_the_search_says():
    """lb::key_hash is acl_hash of the key's four words, and every probe of the
    session table and of the staging table starts at its low bits."""
    csrc = FC.ROOT + "/xsknf_amd/csrc/"
    tsrc = open(csrc + "lb_table.h").read()
    assert re.search(r"uint32_t key_hash\(const Key &k\) \{ return acl_hash\(k\.a, k\.b, k\.c, k\.p\); \}", tsrc)
    for fn in ("find", "put"):
        body = tsrc[tsrc.index(f"XSKNF_HD inline {'uint32_t' if fn == 'find' else 'int'} {fn}("):]
        assert re.search(r"mask = (t\.)?slots - 1;\s*uint32_t s = key_hash\(k\) & mask;", body[:400]), fn
    ksrc = open(csrc + "kernel_lb.h").read()
    for fn, key, size in (("stage", "key", "a.stage_slots"), ("staged", "key", "a.stage_slots"),
                          ("commit_one", "k", "a.t.slots")):
        body = ksrc[ksrc.index(f" {fn}(const Args &a"):]
        body = body[:body.index("\n}\n")]
        assert re.search(rf"mask = {re.escape(size)} - 1", body), fn
        assert re.search(rf"uint32_t s = lb::key_hash\({key}\) & mask;", body), fn
        assert re.search(r"s = \(s \+ 1\) & mask;", body), fn
    # acl_table.h's constants, in the order the restatement applies them
    asrc = open(csrc + "acl_table.h").read()
    body = asrc[asrc.index("inline uint32_t acl_hash("):][:400]
    assert re.findall(r"0x[0-9A-F]{8}u|>> \d+", body) == ["0x9E3779B1u", ">> 15", "0x85EBCA77u", ">> 13", "0xC2B2AE3Du",
                                                        ">> 16", "0x27D4EB2Fu", ">> 15"]


def test_the_restated_hash_is_the_librarys():
    """40 keys that the restated hash sends to one home slot of 2^16 are 40
    rules of one chain in an ACL of 2^16 slots: the builder, which counts the
    home slot as probe 1, reports a longest probe of 40."""
    K, M = 40, 1 << 16
    home, keys = CC.same_home_keys(M, K)
    assert len(set(keys)) == K and {h & (M - 1) for h in CC.hash_keys(keys)} == {home}
    rules = FC.rules_from_keys([CC.sid_bytes((a, b, c & 0xffff, c >> 16, p)) for a, b, c, p in keys], [1] * K)
    with Acl.from_rules(rules, slots=M) as A:
        assert A.info["rules"] == K and A.info["slots"] == M and A.info["max_probe"] == K
    assert CC.chain_of(keys, M).longest == K


def test_the_search_is_deterministic_and_in_its_window():
    bk = CC.one_backend(6)
    for M, w, group in ((64, 4, "both"), (16384, 16, "s"), (16384, 16, "b")):
        fl = CC.flows(bk, M, w, group, 256)
        if M == 64:   # once from scratch: the draws and the hashes are cached per process
            CC._draw.cache_clear()
            CC._hashes.cache_clear()
        assert fl == CC.flows(bk, M, w, group, 256) and len(set(fl)) == 256
        hs = np.array(CC.hash_keys([CC.fwd_key(s) for s in fl]))
        hb = np.array(CC.hash_keys([CC.bwd_key(bk, s) for s in fl]))
        assert CC.in_window(hs, M, w).all() == (group != "b") and CC.in_window(hb, M, w).all() == (group != "s")
        assert CC.in_window(hs, M, w).any() == (group != "b") and CC.in_window(hb, M, w).any() == (group != "s")
        homes = set(((hs if group != "b" else hb) & (M - 1)).tolist())
        assert homes <= set(range(M - w // 2, M)) | set(range(w // 2)) and min(homes) < w // 2 <= M - w // 2 <= max(homes)
        # a window of M slots is a window of every smaller table
        assert CC.in_window(hs if group != "b" else hb, M // 2, w).all()
    # and backward_sid of lb_cases (jhash over one backend) is this module's
    assert all(LC.backward_sid(bk, s) == CC.bwd_sid(bk, s) for s in fl[:8])


def test_the_chain_model():
    c = CC.Chain(8)
    k = CC.flows(CC.one_backend(17), 8, 2, "s", 5)
    homes = [h & 7 for h in CC.hash_keys([CC.fwd_key(s) for s in k])]
    assert set(homes) <= {7, 0}
    got = [c.put(CC.fwd_key(s)) for s in k]
    occupied = sorted(c.slots)
    assert len(occupied) == 5 and c.longest == max(p for p, _ in got) >= 3
    assert [c.find(CC.fwd_key(s))[::2] for s in k] == [(p, True) for p, _ in got]
    assert (7 in homes) == (c.wraps > 0)
    assert CC.stage_slots(0) == CC.stage_slots(16) == 64 and CC.stage_slots(17) == 128 and CC.stage_slots(4096) == 16384


def host_and_model(bk, pre, batches, max_sessions, slots, rules=None, acl_slots=0):
    """Every batch (a CC.Batch) through the host model and the dict model on
    tables that start with `pre`: UMEM bytes, verdicts, counters and the sorted
    session dump agree after each.  Returns the host's (verdicts, stats) per
    batch."""
    acl = None if rules is None else FC.acl_dict(rules)
    m = (LC.Model if rules is None else WC.Model)(bk, max_sessions)
    out = []
    with lb.LoadBalancer.from_backends(bk, max_sessions=max_sessions, slots=slots) as L:
        assert L.info["slots"] == slots and L.info["max_sessions"] == max_sessions
        if pre is not None:
            L.sessions_put(*pre)
            m.sessions_put(*pre)
        A = None if rules is None else Acl.from_rules(rules, slots=acl_slots)
        for b in batches:
            umem, descs = b.arrays()
            u1, u2 = umem.copy(), umem.copy()
            if rules is None:
                v1, s1 = lb.lb_host(u1, descs, L, I, NIF)
                v2, s2 = m.batch(u2, descs, I, NIF)
            else:
                v1, s1 = lbfw.lbfw_host(u1, descs, A, L, I, NIF)
                v2, s2 = m.batch(u2, descs, I, NIF, acl)
            assert np.array_equal(v1, v2), np.nonzero(v1 != v2)[0][:8]
            assert np.array_equal(u1, u2) and np.array_equal(s1, s2), (s1, s2)
            k1, w1 = L.sessions_dump()
            k2, w2 = m.dump()
            assert k1.tobytes() == k2.tobytes() and w1.tobytes() == w2.tobytes()
            assert L.info["host_sessions"] == k1.shape[0]
            out.append((v1, s1))
        if A is not None:
            A.close()
    return out


def stored_keys(pre):
    return [CC.fwd_key((int(k["saddr"]), int(k["daddr"]), int(k["sport"]), int(k["dport"]), int(k["proto"])))
            for k in pre[0]]


def test_deep_chains_across_the_tables_end():
    """slots == 2 * max_sessions; 300 stored sessions in one cluster across the
    table's end, each hit; 150 absent keys of the same homes; 100 new flows
    stored into the cluster."""
    bk, pre, b, stored, absent, new = CC.deep_case()
    c = CC.chain_of(stored_keys(pre), 1024)
    assert c.longest >= 256 and c.wraps > 0
    deep = [c.find(CC.fwd_key(s)) for s in stored]
    assert all(f for _, _, f in deep) and max(p for p, _, _ in deep) >= 256
    miss = [c.find(CC.fwd_key(s)) for s in absent]
    assert not any(f for _, _, f in miss) and min(p for p, _, _ in miss) >= 64 and any(wr for _, wr, _ in miss)
    for s in new:
        assert c.put(CC.fwd_key(s))[0] >= 64
    (v, st), (v2, st2) = host_and_model(bk, pre, [b, b], 512, 1024)
    assert [int(x) for x in st[:6]] == [640, 450, 190, 0, 200, 0]
    assert [int(x) for x in st2[:6]] == [640, 450, 190, 0, 0, 0]


def test_the_grids_batch_on_the_host():
    """3b's batch (tests/test_gpu_lb_collide.py) against the dict model."""
    T = LC.code_constant(r"constexpr int kThreads = (\d+);")
    bk, b, fl = CC.grid_case(T)
    c = CC.chain_of(b.staged_keys(bk), 8192)
    assert c.longest >= 256 and c.wraps > 0
    (v, st), (v2, st2) = host_and_model(bk, None, [b, b], 4096, 8192)
    assert int(st[4]) == 1024 and int(st2[4]) == 0 and int(st[5]) == 0
    want = b.expected_verdicts(bk)
    assert all(int(v[i]) == x for i, x in want.items())
    assert set(want.values()) == {1, CC.INGRESS, CC.PASS_IFACE}


def test_capacity_boundary_on_the_host():
    """P + 2 F == max_sessions fits exactly; the batch again stores nothing;
    one more flow fails its forward insert and skips the backward one; one
    slot less and the last flow's backward insert fails."""
    d = CC.capacity_case()
    bk, pre, exact = d["bk"], d["pre"], d["exact"]
    new_keys = exact.staged_keys(bk)
    assert pre[0].shape[0] + len(new_keys) == d["max_sessions"] == d["slots"] // 2 and len(set(new_keys)) == 200
    c = CC.chain_of(stored_keys(pre) + new_keys, d["slots"])
    assert c.longest >= 64 and c.wraps > 0
    cs = CC.chain_of(new_keys, CC.stage_slots(exact.n))
    assert cs.longest >= 64 and cs.wraps > 0
    frames_of_flows = sum(1 for t in exact.what if t is not None and t[0] == "f")
    assert frames_of_flows > 200   # a count of frames instead of keys would not fit
    res = host_and_model(bk, pre, [exact, exact, d["extra"]], d["max_sessions"], d["slots"])
    assert [int(s[4]) for _, s in res] == [200, 0, 0] and [int(s[5]) for _, s in res] == [0, 0, 1]
    (v, st), = host_and_model(bk, pre, [exact], d["max_sessions"] - 1, d["slots"])
    assert int(st[4]) == 199 and int(st[5]) >= 1
    # lbfw: the gated flows take no room
    (v, st), = host_and_model(bk, pre, [d["gated"]], d["max_sessions"], d["slots"], rules=d["rules"])
    assert int(st[4]) == 200 and int(st[5]) == 0 and int(st[WC.GATED]) == d["gated_frames"]


def test_lbfw_behind_a_clustered_acl_on_the_host():
    bk, rules, ruled, pre, b, new = CC.acl_cluster_case()
    c = CC.chain_of([CC.fwd_key(s) for s in ruled], 1024)
    assert c.longest >= 256 and c.wraps > 0
    with Acl.from_rules(rules, slots=1024) as A:
        assert A.info["max_probe"] == c.longest and A.info["rules"] == 600
    (v, st), = host_and_model(bk, pre, [b], 1024, 2048, rules=rules, acl_slots=1024)
    assert int(st[WC.GATED]) == 600 and int(st[4]) == 240 and int(st[2]) >= 100
