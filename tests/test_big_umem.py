"""The host forms over a UMEM whose frames lie around byte 2^32
(tests/big_umem_cases.py: the layout, the decoy, the straddler's k table):
xsknf_gpu_firewall_host, _lb_host, _lbfw_host, _macswap_host, _forward_host,
xsknf_gpu_shard_plan, _shard_pack_plan and _shard_rebase against the pure-Python
models, on S bytes of private anonymous memory of which only the written pages
are ever committed.  After every run: the window and the tail equal the model's
bytes, the decoy is as it was put, every other byte of the UMEM is zero.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import big_umem_cases as BC
from tests import copy_cases as CC
from tests import firewall_cases as FC
from tests import forward_cases as FWC
from tests import lb_cases as LC
from tests import lbfw_cases as LBC
from tests import macswap_cases as MC
from xsknf_amd import _lib, firewall, lb, lbfw, multi, route
from xsknf_amd.shard import rebase_descs, shard_by_bytes, shard_spans

K_ALL, K_FEW, _ids = BC.K_ALL, BC.K_FEW, BC.k_ids


# ---- the table --------------------------------------------------------------------

def test_every_listed_field_is_crossed():
    """From the model alone: for every (k, field, protocol) of K_FIELDS the
    straddler's field, found by the rules' parse, has 2^32 inside it; the MAC
    rows take every alignment; the copies' k put 2^32 at every byte of the first
    16-byte chunk; the layout puts the straddler there and nothing else across."""
    rng = np.random.default_rng(1)
    want = {"macs", "ethertype", "proto", "ip_check", "addresses", "ports", "l4_check"}
    assert {f for _, f, _ in BC.K_FIELDS} == want
    assert {(f, p) for _, f, p in BC.K_FIELDS} >= {("l4_check", 6), ("l4_check", 17)}
    assert {k for k, f, _ in BC.K_FIELDS if f == "proto"} == {23, 24}
    assert {(BC.B - k) % 4 for k in BC.K_MACS} == {0, 1, 2, 3}
    assert BC.K_COPY == list(range(1, 18))
    for k, field, proto in BC.K_FIELDS:
        st, sid = BC.straddler(rng, proto)
        v, key = FC.frame_key(st)
        assert v is None and key == LBC.sid_key(sid), "the straddler reaches the lookups"
        a, b = BC.field_span(st, field)
        assert BC.crossed(k, (a, b)), (k, field)
        L = BC.lay([FC.make_frame(rng, 60, 5, 17, True) for _ in range(300)], st, k, rng)
        off = BC.offset_of(int(L.descs["addr"][L.straddler]))
        assert off == BC.B - k and off + a < BC.B + (b - a == 1 and k == a) and BC.B <= off + b - (b - a > 1)
        # the model rewrites the straddler on both sides of 2^32 when it has a session
        m, md = L.compact()
        model = LC.Model(np.zeros(0, dtype=lb.BACKEND_DTYPE), 16)
        model.sessions_put(*[np.array([x]) for x in BC.session_for(sid, k % 2, rng)])
        before = m.copy()
        model.batch(m, md, 0, 2)
        changed = np.flatnonzero(m != before) + BC.WIN
        assert changed.min() < BC.B <= changed.max() or k <= 12
    for k in BC.K_COPY:
        L = BC.forward_case(k)
        assert int(L.descs["len"][L.straddler]) == 9000 and (L.descs["len"] == 9000).sum() == 3
        off = np.array([BC.offset_of(a) for a in L.descs["addr"].tolist()])
        ok = np.array([BC.inside(a, ln) for a, ln in zip(L.descs["addr"].tolist(), L.descs["len"].tolist())])
        body = ok & (off < BC.S - BC.TAIL)
        assert {(int(ln), int(o) % 16) for ln, o in zip(L.descs["len"][body], off[body])} >= \
            {(ln, p) for ln in range(201) for p in range(16)}


def test_the_layout_is_what_it_says():
    rng = np.random.default_rng(2)
    L, rules = BC.firewall_case(13, 17)
    assert L.descs.shape[0] <= 4096 and L.win.size - BC.HEAD < BC.MAX_W and BC.WIN % 4096 == 0
    off = [BC.offset_of(a) for a in L.descs["addr"].tolist()]
    ok = [BC.inside(a, ln) for a, ln in zip(L.descs["addr"].tolist(), L.descs["len"].tolist())]
    assert sorted(np.flatnonzero(~np.array(ok)).tolist()) == L.outside.tolist() and len(L.outside) == 9
    below = [o for o, i in zip(off, ok) if i and o < BC.B]
    assert len(below) > 50 and min(below) >= 1 << 31
    # every frame wholly past 2^32 has a decoy that differs from it, 2^32 below
    u, mm = BC.host_umem(L)
    n = 0
    for o, ln, i in zip(off, L.descs["len"].tolist(), ok):
        if i and o >= BC.B and ln and o + ln < BC.S - 14:
            assert not np.array_equal(u[o:o + ln], u[o - BC.B:o - BC.B + ln])
            if ln >= 14:     # (a shorter frame is dropped whatever it holds)
                assert bytes(u[o - BC.B:o - BC.B + 12]) == BC.CANARY
                assert FC.frame_key(bytes(u[o - BC.B:o - BC.B + ln])) != FC.frame_key(bytes(u[o:o + ln]))
                n += 1
    assert n > 1000
    # ... and the model's verdicts over the decoys differ where the ACL tells the two keys apart
    m, md = L.compact()
    acl = FC.acl_dict(rules)
    want = FC.model(m, md, acl)
    dm = m.copy()
    dm[BC.HEAD:L.win.size] = L.decoy[:L.win.size - BC.HEAD]
    dm[L.win.size:] = L.decoy[-BC.TAIL:]
    past = np.array([i and o >= BC.B for o, i in zip(off, ok)])
    other = FC.model(dm, md, acl)
    assert (other[past] != want[past]).sum() > 100
    assert (want[L.outside] == -1).all()
    BC.check_host(u, L, L.win, L.tail, "as put")
    del u
    mm.close()


# ---- the firewall -------------------------------------------------------------------

@pytest.mark.parametrize("k,proto", K_ALL, ids=_ids(K_ALL))
def test_firewall_host(k, proto):
    L, rules = BC.firewall_case(k, proto)
    m, md = L.compact()
    want = FC.model(m, md, FC.acl_dict(rules))
    assert want[L.straddler] == 31 and (want[L.outside] == -1).all() and set(FC.ACTIONS) <= set(want.tolist())
    u, mm = BC.host_umem(L)
    with firewall.Acl.from_rules(rules) as acl:
        got = firewall.firewall_host(u, L.descs, acl)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} verdicts differ, first at {bad[:8]}: {got[bad[:8]]} != {want[bad[:8]]}"
    BC.check_host(u, L, L.win, L.tail, "firewall_host")
    del u
    mm.close()


# ---- the load balancer and lbfw -------------------------------------------------------

def _lb_run(run, k, proto, gated):
    L, bk, (ks, vs) = BC.lb_case(run, k, proto)
    rng = np.random.default_rng(k)
    m, md = L.compact()
    rules, gate = BC.gate_for(L, rng) if gated else (None, None)
    model = (LBC if gated else LC).Model(bk, 4096)
    model.sessions_put(ks, vs)
    before = m.copy()
    if gated:
        wv, ws = model.batch(m, md, 1, 3, acl=gate)
        assert int(ws[LBC.GATED]) > 0
    else:
        wv, ws = model.batch(m, md, 1, 3)
    s = BC.offset_of(int(L.descs["addr"][L.straddler])) - BC.WIN
    assert not np.array_equal(m[s:s + 60], before[s:s + 60]), "the straddler is rewritten"
    assert (wv[L.outside] == -1).all()
    u, mm = BC.host_umem(L)
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096) as lbo:
        lbo.sessions_put(ks, vs)
        if gated:
            with firewall.Acl.from_rules(rules) as acl:
                gv, gs = lbfw.lbfw_host(u, L.descs, acl, lbo, 1, 3)
        else:
            gv, gs = lb.lb_host(u, L.descs, lbo, 1, 3)
        hk, hv = lbo.sessions_dump(lb.HOST_TABLE)
    bad = np.flatnonzero(gv != wv)
    assert bad.size == 0, f"{bad.size} verdicts differ, first at {bad[:8]}: {gv[bad[:8]]} != {wv[bad[:8]]}"
    assert np.array_equal(gs, ws), f"stats {gs} != {ws}"
    wk, wvv = model.dump()
    assert hk.tobytes() == wk.tobytes() and hv.tobytes() == wvv.tobytes(), "the session tables differ"
    BC.check_host(u, L, *L.split(m), what=f"{run} k={k}")
    del u
    mm.close()
    return ws


@pytest.mark.parametrize("k,proto", K_ALL, ids=_ids(K_ALL))
def test_lb_host_prepopulated_sessions(k, proto):
    ws = _lb_run("prepopulated", k, proto, gated=False)
    assert int(ws[1]) >= 32 and int(ws[2]) and int(ws[3]) and not int(ws[4])


@pytest.mark.parametrize("run", ["created", "ordered"])
@pytest.mark.parametrize("k,proto", K_FEW, ids=_ids(K_FEW))
def test_lb_host_sessions_created_and_the_ordered_cause(k, proto, run):
    ws = _lb_run(run, k, proto, gated=False)
    assert int(ws[4]) >= (2 if run == "created" else 1)


@pytest.mark.parametrize("run", ["prepopulated", "created", "ordered"])
@pytest.mark.parametrize("k,proto", K_FEW, ids=_ids(K_FEW))
def test_lbfw_host(k, proto, run):
    _lb_run(run, k, proto, gated=True)


# ---- macswap ------------------------------------------------------------------------

def _macswap_host(u, descs, ingress, action, double, nif):
    """xsknf_gpu_macswap_host in place (macswap.macswap_host copies its UMEM)."""
    d = np.ascontiguousarray(descs)
    v = np.full(d.shape[0], 99, dtype=np.int32)
    o = _lib.MacswapOpts(action, 1 if double else 0, nif, 0)
    rc = _lib.load().xsknf_gpu_macswap_host(u.ctypes.data, BC.S, d.ctypes.data, d.shape[0], ingress, ctypes.byref(o),
                                            v.ctypes.data)
    assert rc == 0
    return v


@pytest.mark.parametrize("double", [False, True], ids=["swap", "double"])
@pytest.mark.parametrize("lens", [(14,), (14, 15, 17, 13)], ids=["14", "cycling"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 6])
def test_macswap_host(k, lens, double):
    L = BC.macswap_case(k, lens)
    m, md = L.compact()
    wu, wv = MC.model(m, md, 1, MC.REDIRECT, double, 3)
    assert (wv[L.outside] == -1).all() and wv[L.straddler] == 2 and np.array_equal(wu, m) == double
    u, mm = BC.host_umem(L)
    gv = _macswap_host(u, L.descs, 1, MC.REDIRECT, double, 3)
    assert np.array_equal(gv, wv)
    BC.check_host(u, L, *L.split(wu), what=f"macswap k={k}")
    del u
    mm.close()


# ---- macswap -> route -> forward ------------------------------------------------------

@pytest.mark.parametrize("k", BC.K_COPY)
def test_forward_host(k):
    L = BC.forward_case(k)
    D = L.other(np.random.default_rng(k))
    mu, mv, (tx, _, _, counts), cap, cut, du, stats = BC.forward_expectation(L, D)
    u, mm = BC.host_umem(L)
    d, dmm = BC.host_umem(D)
    gv = _macswap_host(u, L.descs, 1, MC.REDIRECT, False, 2)
    assert np.array_equal(gv, mv)
    htx, _, _, hcounts = route.route_host(L.descs, gv, 2)
    assert hcounts == counts and np.array_equal(htx[:tx.shape[0]], tx)
    txa = FWC.aligned_descs(htx.shape[0])
    txa[:] = htx
    assert route.forward_host(u, [d, u], txa, cut) == stats
    BC.check_host(u, L, *L.split(mu), what="the rx UMEM")
    BC.check_host(d, D, *D.split(du), what="the destination")
    del u, d
    mm.close()
    dmm.close()


# ---- the planner's host functions ------------------------------------------------------

@pytest.mark.parametrize("nshards", [1, 3, 8])
def test_shard_plans_with_addresses_past_4_gib(nshards):
    """xsknf_gpu_shard_plan, _shard_rebase and _shard_pack_plan on the window's
    descriptors against shard.py and the numpy restatement of the packed layout:
    spans and rebased addresses past 2^32, a shard cut at the straddler."""
    L = BC.forward_case(9)
    d = L.descs
    ranges, spans = multi.shard_plan(d, nshards, BC.S)
    assert ranges == shard_by_bytes(d["len"], nshards)
    assert spans == shard_spans(d, ranges, BC.S)
    assert any(b0 < BC.B <= b1 for b0, b1 in spans) and max(b1 for _, b1 in spans) == BC.S
    for (lo, hi), (b0, _) in zip(ranges, spans):
        got = multi.shard_rebase(d[lo:hi], b0, BC.S)
        assert np.array_equal(got.view(np.uint8), rebase_descs(d[lo:hi], b0, BC.S).view(np.uint8))
    # a cut directly before and after the straddler
    s = L.straddler
    b0 = BC.B - L.k
    for lo, hi in ((s, s + 40), (s + 1, s + 40)):
        sp = shard_spans(d, [(lo, hi)], BC.S)[0]
        got = multi.shard_rebase(d[lo:hi], sp[0], BC.S)
        assert np.array_equal(got.view(np.uint8), rebase_descs(d[lo:hi], sp[0], BC.S).view(np.uint8))
        assert (sp[0] == b0) == (lo == s)
    bounds = [0] + [hi for _, hi in ranges]
    for addr in (0x7f0000000000, 0x7f00fffffff9):
        got, sizes = multi.pack_plan(d, bounds, addr, BC.S)
        want, wsizes = CC.packed_layout(d, bounds, addr, BC.S)
        assert np.array_equal(got["addr"], want) and sizes == wsizes
        assert np.array_equal(got["len"], d["len"]) and np.array_equal(got["options"], d["options"])
