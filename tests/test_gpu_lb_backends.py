"""The services and backends of a live load balancer and the list drain on the
DEVICE (include/xsknf_gpu.h xsknf_gpu_lb_backends_update, _backends_dump,
_drain_backends; xsknf_amd/csrc/lb_backends_device.hip, kernel_lb_backends.h,
kernel_lb_drain_list.h) against the model of tests/lb_backends_cases.py.  The
device calls of a step are enqueued on one stream and the host synchronizes
once, before the dumps.  Batches run through check_batch of
tests/test_gpu_lb.py (device == host, byte for byte) and the dict model."""
import numpy as np
import pytest

from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from tests import lb_backends_cases as BC
from tests.test_gpu_lb import check_batch
from tests.test_lb_backends import V1, V2, b, drain_case
from xsknf_amd import lb, lbfw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ADD, REMOVE, H, D, I, NIF = BC.ADD, BC.REMOVE, BC.H, BC.D, BC.I, BC.NIF
REWRITTEN, PASSED, CREATED, FAILED = 1, 2, 4, 5
T = LC.code_constant(r"constexpr int kThreads = (\d+);", "kernel_lb_remove.h")
G = T * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);", "kernel_lb_remove.h")   # slots per sweep of the largest grid
LDS_SET = LC.code_constant(r"constexpr uint32_t kLdsSetSlots = (\d+);", "kernel_lb_drain_list.h")
REGION = 16 * (2 * lb.MAX_SERVICES + lb.MAX_BACKENDS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def make(recs, max_sessions=2048, slots=4096):
    r = BC.records(recs)
    return lb.LoadBalancer.from_backends(r, max_sessions=max_sessions, slots=slots), BC.Model(r, max_sessions, slots)


def update(L, M, ops):
    """Enqueue on the device copy (the host copy is new at once), apply to the model.  No synchronize."""
    o = BC.op_records(ops)
    L.backends_update(ops=o)
    M.update(o)
    assert BC.same_backends(L, M, H), "the host copy is not the model's"


def agree(L, M):
    torch.cuda.synchronize()
    assert BC.same_backends(L, M, D), "the device copy is not the model's"
    assert BC.same_backends(L, M, H), "the host copy is not the model's"


def batch(dev, L, M, sids, what):
    """One batch on the device, the host and the model: all three agree."""
    umem, descs = RC.fast_frames(sids)
    mu = umem.copy()
    hv, hs = check_batch(dev, L, umem, descs, I, NIF, what)
    mv, ms = M.batch(mu, descs, I, NIF)
    assert np.array_equal(hv, mv) and np.array_equal(hs, ms), f"{what}: the model disagrees: {hs} != {ms}"
    assert RC.same_dump(L, M, D), f"{what}: the device table is not the model's"
    return hv, hs


def drain(L, M, ids):
    i = BC.id_records(ids)
    return L.drain_backends(i), L.drain_backends(i, which=H), M.drain_list(i)


def settled(L, M, *steps):
    """The one synchronize of a step; then the results and both dumps against the model."""
    torch.cuda.synchronize()
    for res, hres, want in steps:
        assert res.cpu().tolist() == want.tolist(), f"device result {res.cpu().tolist()} != {want.tolist()}"
        assert hres.tolist() == want.tolist(), f"host result {hres.tolist()} != {want.tolist()}"
    assert RC.same_dump(L, M, D), "the device table is not the model's"
    assert RC.same_dump(L, M, H), "the host table is not the model's"
    return [w.tolist() for _, _, w in steps]


# ---- the update ---------------------------------------------------------------------

def test_a_sequence_of_updates(dev):
    """Every kind of edit, one update each; after each the device dump, the host
    dump and the model agree, and so do they on a batch of new flows."""
    L, M = make([b(V1, i, ifindex=10 + i) for i in range(5)])
    steps = [("a new service", [(ADD, b(V2, 0))]),
             ("a last backend", [(ADD, b(V1, 5, ifindex=15))]),
             ("mac and ifindex replaced", [(ADD, b(V1, 2, mac=(9,) * 6, ifindex=3))]),
             ("the first goes", [(REMOVE, b(V1, 0))]),
             ("a middle one goes", [(REMOVE, b(V1, 3))]),
             ("the last goes", [(REMOVE, b(V1, 5))]),
             ("add then remove, remove then add", [(ADD, b(V1, 7)), (REMOVE, b(V1, 7)), (REMOVE, b(V1, 1)), (ADD, b(V1, 1))]),
             ("absent", [(REMOVE, b(V1, 9)), (REMOVE, BC.rec(0x0c0c0c0c, 1, 6, 1, 1))]),
             ("the only backend goes", [(REMOVE, b(V2, 0))])]
    with L:
        first = BC.flows_to(*V1, 40, seed=60)
        hv0, _ = batch(dev, L, M, first, "before")
        base = L.info["device_bytes"]
        for j, (what, ops) in enumerate(steps):
            update(L, M, ops)
            agree(L, M)
            hv, hs = batch(dev, L, M, BC.flows_to(*V1, 30, seed=61 + 2 * j) + BC.flows_to(*V2, 10, seed=62 + 2 * j), what)
            assert int(hs[PASSED]) == (0 if BC.svc_key(BC.records([b(V2, 0)])[0]) in M.services else 10), what
        assert L.info["device_bytes"] == base + REGION
        hv1, hs1 = batch(dev, L, M, first, "the flows from before")    # sessions of removed backends still rewrite
        assert int(hs1[CREATED]) == 0 and np.array_equal(hv1, hv0) and (hv0 == 10).any()


def _stream_order(dev, L, M, run, ops, fa, fb):
    """Batch A, the update, batch B on one stream with no synchronize between."""
    (ua, da), (ub, db) = RC.fast_frames(fa), RC.fast_frames(fb)
    ta, tb = torch.from_numpy(ua).to(dev), torch.from_numpy(ub).to(dev)
    dda = torch.from_numpy(da.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    ddb = torch.from_numpy(db.view(np.uint8).reshape(-1, 16).copy()).to(dev)
    wa, wb = (torch.empty(lb.lb_workspace(max(len(fa), len(fb))), dtype=torch.uint8, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    va, sa = run(ta, dda, wa)
    o = BC.op_records(ops)
    L.backends_update(ops=o)
    vb, sb = run(tb, ddb, wb)
    torch.cuda.synchronize()
    mva, msa = M.batch(ua, da, I, NIF)
    M.update(o)
    mvb, msb = M.batch(ub, db, I, NIF)
    assert np.array_equal(va.cpu().numpy(), mva) and np.array_equal(ta.cpu().numpy(), ua), "A is not by the old services"
    assert np.array_equal(vb.cpu().numpy(), mvb) and np.array_equal(tb.cpu().numpy(), ub), "B is not by the new services"
    assert sa.cpu().numpy()[:6].tolist() == msa[:6].tolist() and sb.cpu().numpy()[:6].tolist() == msb[:6].tolist()
    assert RC.same_dump(L, M, D)
    agree(L, M)
    return mva, mvb


def test_stream_order_of_both_nfs(dev):
    L, M = make([b(V1, i, ifindex=10 + i) for i in range(4)])
    with L:
        fl = BC.flows_to(*V1, 1200, seed=70)
        # the load balancer: backend 1 goes between A and B (the first update: the tables move)
        va, vb = _stream_order(dev, L, M, lambda u, d, w: lb.lb_batch(u, d, L, I, NIF, workspace=w),
                               [(REMOVE, b(V1, 1))], fl[:300], fl[300:600])
        assert (va == 11).any() and not (vb == 11).any() and set(vb.tolist()) == {10, 12, 13}
        # lbfw on the same object: a service comes and a backend goes (entries)
        f2 = BC.flows_to(*V2, 100, seed=71)
        va, vb = _stream_order(dev, L, M, lambda u, d, w: lbfw.lbfw_batch(u, d, None, L, I, NIF, workspace=w),
                               [(ADD, b(V2, 0, ifindex=20)), (REMOVE, b(V1, 3))], fl[600:900] + f2[:50], fl[900:] + f2[50:])
        assert (va == 13).any() and (va[300:] == CC.PASS_IFACE).all()
        assert not (vb == 13).any() and (vb[300:] == 20).all()


def test_one_backend_gains_three_hundred(dev):
    """Creation's tables have room for one backend.  Batch A, the update that
    adds 300, batch B, one stream, no wait: A is still right -- it reads the old
    tables, which stay where they are --, B spreads over 301."""
    L, M = make([b(V1, 0, ifindex=0)], max_sessions=8192, slots=16384)
    with L:
        base = L.info["device_bytes"]
        fl = BC.flows_to(*V1, 3000, seed=72)
        more = [(ADD, BC.rec(*V1, 0x0d000001 + i, 0x2000 + i, ifindex=1 + i)) for i in range(300)]
        va, vb = _stream_order(dev, L, M, lambda u, d, w: lb.lb_batch(u, d, L, I, NIF, workspace=w), more, fl[:1500], fl[1500:])
        assert (va == 0).all() and len(set(vb.tolist())) > 250
        assert L.info["device_bytes"] == base + REGION and L.info["backends"] == 301


def test_eight_updates_in_flight(dev):
    """Eight updates enqueued back to back, none waited for: each has a buffer of
    its own while the stream has not passed it."""
    L, M = make([b(V1, i) for i in range(3)])
    with L:
        update(L, M, [(ADD, b(V2, 0))])
        agree(L, M)
        for j in range(8):
            update(L, M, [(ADD, b(V1, 3 + j)), (REMOVE, b(V1, j)), (ADD, b(V2, 1 + j, ifindex=j))])
        agree(L, M)
        assert L.info["backends"] == 3 + 9
        batch(dev, L, M, BC.flows_to(*V1, 40, seed=73) + BC.flows_to(*V2, 40, seed=74), "after eight updates")
        for j in range(8):                                   # and again: the buffers are free and used again
            update(L, M, [(REMOVE, b(V2, j))])
        agree(L, M)
        batch(dev, L, M, BC.flows_to(*V2, 40, seed=75), "after sixteen")


def test_an_update_of_most_entries_and_of_one(dev):
    """3000 backends in one service.  Replacing one record changes one entry;
    removing the first moves every other down by one, which is more entries
    than the tables are long in 32-byte records: they are sent whole."""
    recs = [BC.rec(*V1, 0x0d000001 + i, 0x2000 + (i & 0xfff), ifindex=i & 0xff) for i in range(3000)]
    L, M = make(recs)
    with L:
        update(L, M, [(ADD, recs[2999][:8 - 1] + (7,) + recs[2999][8:])])   # the first update: whole
        agree(L, M)
        one = recs[1234][:6] + ((5, 5, 5, 5, 5, 5), 99, (0, 0))
        update(L, M, [(ADD, one)])
        agree(L, M)
        assert int(L.backends_dump(D)[1234]["ifindex"]) == 99
        batch(dev, L, M, BC.flows_to(*V1, 200, seed=76), "one entry")
        update(L, M, [(REMOVE, recs[0])])
        agree(L, M)
        assert L.info["backends"] == 2999
        batch(dev, L, M, BC.flows_to(*V1, 200, seed=77), "most entries")
        update(L, M, [(ADD, recs[0]), (ADD, b(V2, 0))])                      # and entries again: two and a slot
        agree(L, M)
        batch(dev, L, M, BC.flows_to(*V1, 100, seed=78) + BC.flows_to(*V2, 10, seed=79), "entries again")


# ---- the list drain -----------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 70])
def test_list_drain(dev, n):
    """tests/test_lb_backends.py's host cases on both tables: backends that share
    an address, the same {addr, port} under the other protocol, a duplicate,
    unpaired entries.  A batch after the drain opens the flows anew."""
    recs = drain_case()
    L, M = make(recs)
    with L:
        sids = BC.flows_to(*V1, 300, seed=50) + BC.flows_to(*V2, 300, seed=51)
        batch(dev, L, M, sids, "fill")
        lone = RC.stored([(7, 8, 9, 10, 6), (11, 12, 13, 14, 17)])
        stray = CC.sessions([LC.session(21, 22, 23, 24, 6, lb.TO_BACKEND, 0xc0a80a01, 0x1f90, (1,) * 6, 1),
                             LC.session(0xc0a80a01, 26, 0x1f90, 28, 17, lb.TO_CLIENT, 5, 6, (1,) * 6, 1)])
        for ks, vs in (lone, stray):
            L.sessions_put(ks, vs)
            M.sessions_put(ks, vs)
        ids = BC.backend_ids(recs)
        listed = [ids[0], ids[0]] if n == 2 else (ids[:35] + ids[40:75])[:n]
        count = len(M.sessions)
        (got,) = settled(L, M, drain(L, M, listed))
        assert got[0] == count - len(M.sessions) and (got[0] > 0) == (n > 0)
        assert got[1] == int(got[0] > M.slots // 4)   # (the 70 backends' sessions are more than slots / 4 tombstones)
        assert (CC.sid_bytes((0xc0a80a01, 26, 0x1f90, 28, 17)) in M.sessions) == (n < 70)
        assert CC.sid_bytes((7, 8, 9, 10, 6)) in M.sessions
        hv, hs = batch(dev, L, M, sids, "after the drain")
        assert int(hs[CREATED]) == got[0] - (2 if n == 70 else 1 if n else 0) and int(hs[FAILED]) == 0


@pytest.mark.parametrize("extra", [0, 1])
def test_the_longest_list_in_lds_and_the_shortest_past_it(dev, extra):
    """A set of kLdsSetSlots slots holds a list of half as many: that list is
    probed in LDS, one entry more in global memory.  Ten of the listed backends
    have flows, the others do not exist."""
    n = LDS_SET // 2 + extra
    recs = [b(V1, i) for i in range(20)]
    L, M = make(recs)
    with L:
        sids = BC.flows_to(*V1, 400, seed=80)
        batch(dev, L, M, sids, "fill")
        ids = BC.backend_ids(recs)[5:15] + [(0x0e000001 + i, 0x1f90 + (i & 15), 6 + 11 * (i & 1)) for i in range(n - 10)]
        rng = np.random.default_rng(81)
        ids = [ids[i] for i in rng.permutation(n)]
        want = 2 * sum(1 for s in sids if 5 <= BC.choice(s, 20) < 15)
        assert settled(L, M, drain(L, M, ids)) == [[want, 0]] and want > 100
        hv, hs = batch(dev, L, M, sids, "after the drain")
        assert int(hs[CREATED]) == want


def test_more_slots_than_the_grid_has_lanes(dev):
    """2^20 slots against 2048 x 256 lanes: every lane takes a second slot.  The
    table is sparse; sessions that go and sessions that stay lie in both halves."""
    slots = 2 * G
    assert slots == 1 << 20
    recs = [b(V1, i) for i in range(4)]
    L, M = make(recs, max_sessions=4096, slots=slots)
    with L:
        sids = BC.flows_to(*V1, 1500, seed=82)
        batch(dev, L, M, sids, "fill")
        ids = BC.backend_ids(recs)
        gone = [CC.fwd_key(s) for s in sids if BC.choice(s, 4) in (1, 2)]
        homes = np.array(CC.hash_keys(gone)) & (slots - 1)
        assert (homes >= G).any() and (homes < G).any()
        assert settled(L, M, drain(L, M, [ids[1], ids[2]])) == [[2 * len(gone), 0]]
        left = {rep[1] for rep in M.sessions.values() if rep[0] == lb.TO_BACKEND}
        assert left == {ids[0][0], ids[3][0]}


def test_list_drain_crosses_the_tombstone_bound(dev):
    recs = [b(V1, i) for i in range(6)]
    L, M = make(recs, max_sessions=128, slots=256)
    with L:
        sids = BC.flows_to(*V1, 60, seed=52)
        per = [sum(1 for s in sids if BC.choice(s, 6) == i) for i in range(6)]
        batch(dev, L, M, sids, "fill")
        ids = BC.backend_ids(recs)
        first, k, order = [], 0, sorted(range(6), key=lambda i: per[i])
        while 2 * sum(per[i] for i in first + [order[k]]) <= 64:
            first.append(order[k])
            k += 1
        rest = [i for i in range(6) if i not in first]
        assert first and 2 * sum(per) > 64
        a = drain(L, M, [ids[i] for i in first])            # both in flight: the second crosses slots / 4
        c = drain(L, M, [ids[i] for i in rest])
        assert settled(L, M, a, c) == [[2 * sum(per[i] for i in first), 0], [2 * sum(per[i] for i in rest), 1]]
        assert not M.sessions
        batch(dev, L, M, sids, "after the rebuild")


def test_take_two_of_four_backends_out_of_service(dev):
    """REMOVE two of four, drain the two, the old flows again -- one stream, no
    wait.  Every flow is balanced anew over the two left, as the model says, and
    the table holds no session of the removed ones."""
    recs = [b(V1, i, ifindex=10 + i) for i in range(4)]
    L, M = make(recs)
    with L:
        sids = BC.flows_to(*V1, 400, seed=83)
        hv0, _ = batch(dev, L, M, sids, "four backends")
        out = [recs[1], recs[2]]
        update(L, M, [(REMOVE, r) for r in out])
        step = drain(L, M, BC.backend_ids(out))
        want = 2 * sum(1 for s in sids if BC.choice(s, 4) in (1, 2))
        assert settled(L, M, step) == [[want, 0]]
        agree(L, M)
        hv, hs = batch(dev, L, M, sids, "two backends")
        assert int(hs[CREATED]) == want
        moved = np.isin(hv0, (11, 12))
        assert np.array_equal(hv[~moved], hv0[~moved]) and set(hv[moved].tolist()) == {10, 13}
        assert hv[moved].tolist() == [(10, 13)[BC.choice(s, 2)] for s, m in zip(sids, moved) if m]
        gone = {(int(r[4]), int(r[5])) for r in out}
        for k, rep in M.sessions.items():
            assert (rep[1], rep[2]) not in gone and (LC._u32(k, 0), LC._u16(k, 8)) not in gone
