"""Removing sessions from the load balancer's DEVICE table (include/xsknf_gpu.h
xsknf_gpu_lb_sessions_remove, _drain_backend, _sessions_clear;
xsknf_amd/csrc/lb_remove_device.hip, kernel_lb_remove.h) against the set
semantics of tests/lb_remove_cases.py.  Every call goes to the device table and,
as its _host form, to the host table: after every step both dumps equal the
model and both results are the model's.  The device calls of a step are
enqueued on one stream and the host synchronizes once, before the dump.
Batches before and after a removal run through check_batch of
tests/test_gpu_lb.py (device == host, byte for byte) and the dict model."""
import re

import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lb_remove_cases as RC
from tests.test_gpu_lb import check_batch
from tests.test_gpu_lbfw import check_batch as lbfw_check_batch
from xsknf_amd import _lib, lb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = LC.code_constant(r"constexpr int kThreads = (\d+);", "kernel_lb_remove.h")        # keys per block and step
G = T * LC.code_constant(r"constexpr int kMaxBlocks = (\d+);", "kernel_lb_remove.h")  # keys per sweep of the largest grid
I, NIF = CC.INGRESS, CC.NIF
H, D = lb.HOST_TABLE, lb.DEVICE_TABLE
REWRITTEN, CREATED, FAILED, ORDERED = 1, 4, 5, 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def put(L, M, ks, vs):
    L.sessions_put(ks, vs)
    M.sessions_put(ks, vs)


def remove(L, M, keys, pair=False, model_keys=None):
    """Enqueue on the device table, apply to the host table and the model:
    (device result tensor, host result, expected result).  No synchronize."""
    k = keys if isinstance(keys, np.ndarray) else RC.key_records(keys)
    res = L.sessions_remove(k, pair=pair)
    return res, L.sessions_remove(k, pair=pair, which=H), M.remove(k if model_keys is None else model_keys, pair)


def drain(L, M, addr, port, proto):
    return L.drain_backend(addr, port, proto), L.drain_backend(addr, port, proto, which=H), M.drain(addr, port, proto)


def settled(L, M, *steps):
    """The one synchronize of a step; then the results and both dumps against the model."""
    torch.cuda.synchronize()
    for res, hres, want in steps:
        assert res.cpu().tolist() == want.tolist(), f"device result {res.cpu().tolist()} != {want.tolist()}"
        assert hres.tolist() == want.tolist(), f"host result {hres.tolist()} != {want.tolist()}"
    assert RC.same_dump(L, M, D), "the device table is not the model's"
    assert RC.same_dump(L, M, H), "the host table is not the model's"
    i = L.info
    assert i["device_sessions"] == i["host_sessions"] == len(M.sessions)
    return [w.tolist() for _, _, w in steps]


def batch(dev, L, M, umem, descs, what, ordered=0):
    """One batch on the device, the host and the model: all three agree."""
    mu = umem.copy()
    hv, hs = check_batch(dev, L, umem, descs, I, NIF, what, ordered=ordered)
    mv, ms = M.batch(mu, descs, I, NIF)
    assert np.array_equal(hv, mv) and np.array_equal(hs, ms), f"{what}: the model disagrees: {hs} != {ms}"
    assert RC.same_dump(L, M, D), f"{what}: the device table is not the model's"
    return hv, hs


def test_sizes_are_read_from_the_code():
    src = open(FC.ROOT + "/xsknf_amd/csrc/kernel_lb_remove.h").read()
    assert len(re.findall(r"__launch_bounds__\(kThreads\)", src)) == 5
    assert len(re.findall(r"stride = gridDim\.x \* kThreads", src)) == 5
    dsrc = open(FC.ROOT + "/xsknf_amd/csrc/lb_remove_device.hip").read()
    assert re.search(r"tiles < static_cast<uint32_t>\(lbr::kMaxBlocks\) \? tiles : lbr::kMaxBlocks", dsrc)
    assert T % 64 == 0 and G > T


@pytest.mark.parametrize("kind", ["home", "wrap"])
@pytest.mark.parametrize("where", [0, 5, 11])
def test_removal_from_a_probe_chain(dev, kind, where):
    """Twelve flows whose forward keys form one chain of the 64-slot table (also
    across its end), stored in chain order.  One flow goes, head, middle or
    tail.  The flows further down the chain are still hits; the removed flow's
    frames create it anew, with the same backend."""
    sids = RC.chain_keys(kind)
    bk = RC.chain_service()
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        M = RC.Model(bk, 32, 64)
        fwd = [CC.session_of(bk, s, lb.TO_BACKEND) for s in sids]
        bwd = [CC.session_of(bk, CC.bwd_sid(bk, s), lb.TO_CLIENT, ifindex=I) for s in sids]
        put(L, M, *CC.sessions(fwd + bwd))
        before = dict(M.sessions)
        assert settled(L, M, remove(L, M, [sids[where]], pair=True)) == [[2, 0]]
        rest = sids[where + 1:] + sids[:where]
        if rest:
            hv, hs = batch(dev, L, M, *RC.frames_of(rest), "the rest of the chain")
            assert int(hs[CREATED]) == 0 and int(hs[REWRITTEN]) == len(rest) and (hv == RC.HIT_IFACE).all()
        hv, hs = batch(dev, L, M, *RC.frames_of([sids[where]] * 3), "the removed flow")
        assert int(hs[CREATED]) == 2 and int(hs[FAILED]) == 0 and (hv == RC.HIT_IFACE).all()
        key = CC.sid_bytes(sids[where])
        assert M.sessions[key] == before[key] and len(M.sessions) == 24


def test_list_lengths_around_the_wave_the_block_and_the_grid(dev):
    """n = 1, 63, 64, 65, 257 (two blocks) and one more than the largest grid
    covers in one sweep, where only the LAST key is one the table holds: the
    lane that takes a second key in its loop removes it."""
    rng = np.random.default_rng(21)
    sids = [(int(rng.integers(1, 1 << 32)), 7, int(rng.integers(1, 1 << 16)), 7, 6 + 11 * (i & 1)) for i in range(700)]
    absent = RC.key_records([(s[0], 8, s[2], 8, s[4]) for s in sids[:300]])
    with lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=4096, slots=8192) as L:
        M = RC.Model([], 4096, 8192)
        held = RC.key_records(sids)
        put(L, M, *RC.stored(sids))
        at = 0
        for n in (1, 63, 64, 65, 257):
            pool = np.concatenate([held[at:at + (n + 1) // 2], absent[:n // 2]])   # half held and new, half absent
            at += (n + 1) // 2
            keys = pool[rng.permutation(pool.shape[0])]
            assert keys.shape[0] == n
            assert settled(L, M, remove(L, M, keys, pair=bool(n & 1))) == [[(n + 1) // 2, 0]], f"n = {n}"
        keys = np.tile(absent, (G + 300) // 300)[:G + 1].copy()
        keys[G] = held[at]
        assert keys.shape[0] == G + 1 and G + 1 > T * 2048
        assert settled(L, M, remove(L, M, keys, model_keys=keys[G - 300:])) == [[1, 0]]
        assert CC.sid_bytes(sids[at]) not in M.sessions


def test_every_lane_on_one_slot_and_keys_beside_their_partners(dev):
    """4096 copies of one key: one removal, with `pair` two.  Every key of 100
    flows listed beside its partner, three times over: 200, whatever lane wins."""
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 103, seed=22)
    with lb.LoadBalancer.from_backends(bk, max_sessions=512, slots=2048) as L:
        M = RC.Model(bk, 512, 2048)
        hv, hs = batch(dev, L, M, *RC.fast_frames(sids), "fill")
        assert int(hs[CREATED]) == 206
        one = np.tile(RC.key_records([sids[100]]), 4096)
        assert settled(L, M, remove(L, M, one, model_keys=one[:1])) == [[1, 0]]
        back = CC.bwd_sid(bk, sids[100])
        assert CC.sid_bytes(back) in M.sessions
        assert settled(L, M, remove(L, M, one, pair=True, model_keys=one[:1])) == [[0, 0]]
        one = np.tile(RC.key_records([sids[101]]), 4096)
        assert settled(L, M, remove(L, M, one, pair=True, model_keys=one[:1])) == [[2, 0]]
        one = np.tile(RC.key_records([CC.bwd_sid(bk, sids[102])]), 4096)
        assert settled(L, M, remove(L, M, one, pair=True, model_keys=one[:1])) == [[2, 0]]
        both = RC.key_records([s for f in sids[:100] for s in (f, CC.bwd_sid(bk, f))] * 3)
        rng = np.random.default_rng(23)
        both = both[rng.permutation(both.shape[0])]
        assert settled(L, M, remove(L, M, both, pair=True)) == [[200, 0]]
        assert set(M.sessions) == {CC.sid_bytes(back)}


def test_pair_leaves_strangers(dev):
    """An unpaired sessions_put entry, a partner key that holds a session of the
    same direction, one that holds another service's backward session, and a
    backward session that a second flow replaced: the listed key goes alone."""
    rng = np.random.default_rng(24)
    bk, _, fl = LC.ordered_cause(rng, "shared_b")
    umem, descs = LC.pack_packed(fl, rng)
    keys = [LC.frame_sid(f) for f in fl]
    bsid, s1, s2 = keys[1], keys[2], keys[4]
    one_bk = bk[:1]
    a, b, c = RC.new_flows(one_bk, 3, seed=25)
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        M = RC.Model(bk, 32, 64)
        mu = umem.copy()
        hv, hs = check_batch(dev, L, umem, descs, 0, 2, "two flows, one backward key", ordered=1)
        M.batch(mu, descs, 0, 2)
        assert RC.same_dump(L, M, D) and RC.partner(bsid, M.sessions[bsid]) == s2
        same_dir = LC.session(*CC.bwd_sid(one_bk, b), lb.TO_BACKEND, 1, 2, (0,) * 6, 0)
        stranger = LC.session(*CC.bwd_sid(one_bk, c), lb.TO_CLIENT, int(bk[0]["vaddr"]) + 1, int(bk[0]["vport"]), (0,) * 6, 0)
        put(L, M, *CC.sessions([CC.session_of(one_bk, s, lb.TO_BACKEND) for s in (a, b, c)] + [same_dir, stranger]))

        def rec(kb):
            r = np.zeros(1, dtype=lb.KEY_DTYPE)
            r[0] = (LC._u32(kb, 0), LC._u32(kb, 4), LC._u16(kb, 8), LC._u16(kb, 10), kb[12], (0, 0, 0))
            return r

        listed = np.concatenate([RC.key_records([a, b, c]), rec(s1)])
        assert settled(L, M, remove(L, M, listed, pair=True)) == [[4, 0]]
        assert set(M.sessions) == {bsid, s2, CC.sid_bytes(CC.bwd_sid(one_bk, b)), CC.sid_bytes(CC.bwd_sid(one_bk, c))}
        assert settled(L, M, remove(L, M, rec(s2), pair=True)) == [[2, 0]]


def test_drain_one_backend_of_three(dev):
    """Sixty flows over three backends, created by a batch.  Draining one takes
    both halves of its flows and nothing else; the same batch again creates
    those flows anew and finds every other session."""
    bk = RC.chain_service(backends=3)
    sids = RC.new_flows(bk, 60, seed=26)
    umem, descs = RC.fast_frames(sids + [CC.bwd_sid(bk[i:i + 1], s) for i in range(3) for s in sids[:5]])
    with lb.LoadBalancer.from_backends(bk, max_sessions=256, slots=512) as L:
        M = RC.Model(bk, 256, 512)
        hv, hs = batch(dev, L, M, umem, descs, "fill")
        assert int(hs[CREATED]) == 120
        per = [sum(1 for rep in M.sessions.values() if rep[0] == lb.TO_BACKEND and rep[1] == int(r["addr"])) for r in bk]
        assert min(per) >= 5 and sum(per) == 60
        r = bk[1]
        assert settled(L, M, drain(L, M, int(r["addr"]), int(r["port"]), 6)) == [[2 * per[1], 0]]
        assert settled(L, M, drain(L, M, int(r["addr"]), int(r["port"]), 17)) == [[0, 0]]
        assert not any(rep[1] == int(r["addr"]) for rep in M.sessions.values() if rep[0] == lb.TO_BACKEND)
        hv2, hs2 = batch(dev, L, M, umem, descs, "after the drain")
        assert int(hs2[CREATED]) == 2 * per[1] and int(hs2[FAILED]) == 0 and len(M.sessions) == 120
        assert np.array_equal(hv2[:60], hv[:60])   # the same backend again: the choice is a function of the sid


def test_a_full_table_has_room_again(dev):
    """max_sessions 16384: 8192 flows fill the table.  One further flow sends its
    batch down the ordered path, where its insert fails.  One flow is removed
    with its partner; the same batch then runs the parallel path and both of its
    sessions are stored."""
    bk = CC.one_backend(17, salt=5)
    sids = RC.new_flows(bk, 8193, seed=27)
    with lb.LoadBalancer.from_backends(bk, max_sessions=16384, slots=32768) as L:
        M = RC.Model(bk, 16384, 32768)
        hv, hs = batch(dev, L, M, *RC.fast_frames(sids[:8192]), "fill")
        assert int(hs[CREATED]) == 16384 and L.info["device_sessions"] == 16384
        more = RC.fast_frames([sids[8192], sids[7], sids[8192], sids[9]])
        hv, hs = batch(dev, L, M, *more, "one flow too many", ordered=1)
        assert int(hs[FAILED]) == 2 and int(hs[CREATED]) == 0
        assert settled(L, M, remove(L, M, [sids[3]], pair=True)) == [[2, 0]]
        hv, hs = batch(dev, L, M, *more, "room again", ordered=0)
        assert int(hs[FAILED]) == 0 and int(hs[CREATED]) == 2 and L.info["device_sessions"] == 16384


def test_reuse_fill_remove_and_fill_again(dev):
    """Eight cycles on the 64-slot table (tests/test_lb_remove.py's, on the
    device): fill to max_sessions by a batch, remove four flows a call.  No
    insert fails, no batch leaves the parallel path, the rebuild is reported."""
    bk = CC.one_backend(6)
    flows = RC.new_flows(bk, 8 * 16, seed=15)
    compacted = 0
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        M = RC.Model(bk, 32, 64)
        for cycle in range(8):
            sids = flows[16 * cycle:16 * cycle + 16]
            hv, hs = batch(dev, L, M, *RC.frames_of(sids, seed=cycle), f"cycle {cycle}", ordered=0)
            assert int(hs[FAILED]) == 0 and int(hs[CREATED]) == 32
            steps = [remove(L, M, sids[part:part + 4], pair=True) for part in range(0, 16, 4)]   # four calls in flight
            got = settled(L, M, *steps)
            assert [g[0] for g in got] == [8] * 4 and not M.sessions
            compacted += sum(g[1] for g in got)
        assert compacted >= 8


def test_clear_and_put_after_removals(dev):
    sids = RC.chain_keys("home") + RC.chain_keys("wrap")
    with lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=32, slots=64) as L:
        M = RC.Model([], 32, 64)
        put(L, M, *RC.stored(sids))
        assert settled(L, M, remove(L, M, sids[::2])) == [[12, 0]]
        ks, vs = RC.stored(sids[:6])     # returning keys and replaced values, through the device table's host copy
        vs["port"] += 3
        put(L, M, ks, vs)
        assert settled(L, M, remove(L, M, sids[1:11:2])) == [[5, 1]]   # the 17th tombstone
        L.sessions_clear(D)
        L.sessions_clear(H)
        M.clear()
        settled(L, M)
        put(L, M, *RC.stored(sids))
        hv, hs = batch(dev, L, M, *RC.frames_of(sids), "after the clear")
        assert int(hs[REWRITTEN]) == 24 and int(hs[CREATED]) == 0
        # n == 0: nothing launched, zeros written
        res = torch.full((4,), 7, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        assert _lib.load().xsknf_gpu_lb_sessions_remove(L.handle, None, 0, 1, res.data_ptr(), s) == 0
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [0, 0, 7, 7]
        settled(L, M)


def test_stream_order(dev):
    """Batch A, the removal, batch B on one stream with no synchronize between
    them: A's frames are all hits, B's show exactly the removed sessions."""
    rng = np.random.default_rng(28)
    sids = [(int(rng.integers(1, 1 << 32)), 7, int(rng.integers(1, 1 << 16)), 7, 6) for _ in range(4096)]
    gone = np.zeros(4096, dtype=bool)
    gone[rng.permutation(4096)[:1500]] = True
    umem, descs = RC.fast_frames(sids)
    with lb.LoadBalancer.from_backends(np.zeros(0, dtype=lb.BACKEND_DTYPE), max_sessions=4096, slots=8192) as L:
        M = RC.Model([], 4096, 8192)
        put(L, M, *RC.stored(sids))
        keys = RC.key_records([s for s, g in zip(sids, gone) if g])
        ua, ub = torch.from_numpy(umem).to(dev), torch.from_numpy(umem).to(dev)
        dd = torch.from_numpy(descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        wa, wb = (torch.empty(lb.lb_workspace(4096), dtype=torch.uint8, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        va, sa = lb.lb_batch(ua, dd, L, I, NIF, workspace=wa)
        step = remove(L, M, keys)
        vb, sb = lb.lb_batch(ub, dd, L, I, NIF, workspace=wb)
        settled(L, M, step)
        assert (va.cpu().numpy() == RC.HIT_IFACE).all() and int(sa[REWRITTEN]) == 4096
        assert np.array_equal(vb.cpu().numpy(), np.where(gone, CC.PASS_IFACE, RC.HIT_IFACE))
        assert int(sb[REWRITTEN]) == 4096 - 1500 and int(sb[2]) == 1500


def test_lbfw_on_the_same_object_after_a_removal(dev):
    bk = CC.one_backend(17)
    sids = RC.new_flows(bk, 20, seed=29)
    umem, descs = RC.frames_of(sids)
    with lb.LoadBalancer.from_backends(bk, max_sessions=64, slots=128) as L:
        M = RC.Model(bk, 64, 128)
        batch(dev, L, M, umem, descs, "fill")
        assert settled(L, M, remove(L, M, sids[:7], pair=True)) == [[14, 0]]
        hu, hv, hs = lbfw_check_batch(dev, None, L, umem, descs, I, NIF, "lbfw after the removal", ordered=0)
        assert int(hs[CREATED]) == 14 and int(hs[REWRITTEN]) == 20
