"""The ACL's hit counters on the device (include/xsknf_gpu.h
xsknf_gpu_acl_counters_*; xsknf_amd/csrc/kernel_firewall_count.h,
kernel_acl_count.h, kernel_acl_update.h, kernel_lb.h lb_propose<true>): the
device set against the plain-Python model of tests/acl_counter_cases.py and
against the host set fed the same frames (tests/test_acl_counters.py holds that
one to the model too).  All results are exact integers."""
import numpy as np
import pytest

from tests import acl_counter_cases as CC
from tests import acl_update_cases as UC
from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lbfw_cases as WC
from tests import test_gpu_lbfw as GL
from xsknf_amd import firewall, lb, lbfw
from xsknf_amd.firewall import Acl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = FC.code_constant(r"constexpr int kThreads = (\d+);")        # frames per block and step
G = T * FC.code_constant(r"constexpr int kMaxBlocks = (\d+);")  # frames per sweep of the largest grid
CASES = CC.update_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def _batch(dev, umem, descs, acl, stream=None):
    """Enqueue one xsknf_gpu_firewall_batch; returns the verdict tensor (and keeps the inputs alive with it)."""
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.device(dev), torch.cuda.stream(s):
        du, dd = _to_dev(umem, dev), _to_dev(descs, dev)
        dv = torch.full((descs.shape[0],), 0x5eadbeef, dtype=torch.int32, device=dev)
        firewall.firewall_batch_ptr(du.data_ptr(), umem.size, dd.data_ptr(), descs.shape[0], acl, dv.data_ptr(), s.cuda_stream)
    dv.keep = (du, dd)
    return dv


def _both(dev, A, m, umem, descs, what):
    """One batch on the device and the host, the model beside them: verdicts and both sets."""
    want = m.batch(umem, descs)
    got = _batch(dev, umem, descs, A).cpu().numpy()
    assert np.array_equal(got, want), f"{what}: device verdicts"
    assert np.array_equal(firewall.firewall_host(umem, descs, A), want), f"{what}: host verdicts"
    CC.check(A, m, device=True, what=what)
    return CC.check(A, m, what=what)


def _setup(seed, n=80, slots=0):
    rng = np.random.default_rng(seed)
    keys = UC.keys_away(rng, n, ())
    rules = FC.rules_from_keys(keys, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(n)])
    return rng, keys, rules


def test_the_kernel_is_what_the_sizes_were_read_from():
    src = open(FC.ROOT + "/xsknf_amd/csrc/kernel_firewall_count.h").read()
    assert "__launch_bounds__(kThreads)" in src and '#include "kernel_firewall.h"' in src
    assert T % 64 == 0 and G > T


@pytest.mark.parametrize("shape", ["one rule", "64 rules", "65", "257"])
def test_a_wave_a_partial_wave_a_second_block(dev, shape):
    rng, keys, rules = _setup(5201)
    ks = {"one rule": keys[:1] * 64, "64 rules": keys[:64], "65": (keys[:3] * 22)[:65], "257": (keys * 4)[:257]}[shape]
    assert T == 256
    m = CC.Model(rules)
    umem, descs = CC.frames_for_keys(ks, rng)
    with torch.cuda.device(dev), Acl.from_rules(rules) as A:
        base = A.info["device_bytes"]
        A.counters_enable()
        assert A.info["device_bytes"] == base + 16 * A.info["slots"] + 32
        _, ctr, totals = _both(dev, A, m, umem, descs, shape)
        assert int(totals[CC.HITS]) == len(ks) == int(ctr["packets"].sum())
        if shape == "one rule":
            assert int(ctr["packets"].max()) == 64 and int(ctr["bytes"].max()) == int(descs["len"].sum())


def test_hits_interleaved_with_misses_and_decided_frames(dev):
    """Lane by lane: a hit on one rule, a frame the parse decides, a miss, and
    descriptors outside the UMEM among them -- lanes that left early are in
    nobody's group -- then the same wave's worth again with two rules alternating."""
    rng, keys, rules = _setup(5202)
    m = CC.Model(rules)
    with torch.cuda.device(dev), Acl.from_rules(rules) as A:
        A.counters_enable()
        umem, descs = CC.interleaved_wave(rng, keys[0], keys)
        assert descs.shape[0] == 128
        _, ctr, totals = _both(dev, A, m, umem, descs, "interleaved")
        assert totals.tolist() == [128, 32, 32, 64] and int(ctr["packets"].max()) == 32
        umem, descs = CC.frames_for_keys([keys[1 + i % 2] if i % 4 else CC.absent_keys(rng, 1, keys)[0] for i in range(64)], rng)
        _both(dev, A, m, umem, descs, "two rules alternating")


def test_wrapped_and_colliding_probe_chains(dev):
    """slots - 1 rules in 1024 slots: every hit and as many misses, chains that
    run into one another and wrap."""
    rules, umem, descs = FC.full_table_case(slots=1024)
    m = CC.Model(rules)
    with torch.cuda.device(dev), Acl.from_rules(rules, 1024) as A:
        A.counters_enable()
        assert A.info["max_probe"] > 16
        _, ctr, totals = _both(dev, A, m, umem, descs, "full table")
        assert (ctr["packets"] == 1).all() and (ctr["bytes"] == 64).all() and int(totals[CC.MISSES]) >= 1000


def test_the_grid_stride_loop_twice_with_a_ragged_end(dev):
    """kMaxBlocks x kThreads + 257 frames of 64 bytes over 1,000 rules, a few of
    which take most: the loop's second trip is one block and one lane.  The
    expected counts come from numpy (the model's loop restated on arrays)."""
    rng = np.random.default_rng(5203)
    n = G + 257
    rules = FC.random_rules(rng, 1000)
    assert len(FC.acl_dict(rules)) == 1000
    w = 1.0 / (1 + np.arange(1000))
    pick = rng.choice(1000, n, p=w / w.sum())
    umem, descs = FC.frames_for_rules(rules[pick], rng)
    miss = rng.random(n) < 0.25
    umem.reshape(-1, 64)[miss, 30] ^= 0x40   # a daddr bit: (almost surely) nobody's key
    d = FC.rules_dict_fast(rules)
    raw = umem.reshape(-1, 64)
    kb = np.concatenate([raw[:, 26:38], raw[:, 23:24]], axis=1).tobytes()
    hit = np.array([kb[13 * i:13 * i + 13] in d for i in range(n)])
    assert (hit[~miss]).all() and hit[miss].sum() < 10
    packets = np.bincount(pick[hit], minlength=1000)
    with torch.cuda.device(dev), Acl.from_rules(rules) as A:
        A.counters_enable()
        for rounds in (1, 2):   # two batches in a row
            got = _batch(dev, umem, descs, A).cpu().numpy()
            assert np.array_equal(got, np.where(hit, rules["action"][pick], 0))
            r, ctr, totals = A.counters(device=True)
            assert totals.tolist() == [rounds * n, rounds * int(hit.sum()), rounds * int((~hit).sum()), 0]
            by = {FC.rule_key(x): int(c["packets"]) for x, c in zip(r, ctr)}
            assert [by[FC.rule_key(x)] for x in rules] == (rounds * packets).tolist()
            assert (ctr["bytes"] == 64 * ctr["packets"]).all()


def test_two_streams_count_against_one_acl(dev):
    rng, keys, rules = _setup(5204)
    m = CC.Model(rules)
    ua, da = CC.frames_for_keys(CC.traffic(rng, keys, 20000), rng)
    ub, db = CC.frames_for_keys(CC.traffic(rng, keys[::-1], 20000), rng)
    with torch.cuda.device(dev), Acl.from_rules(rules) as A:
        A.counters_enable()
        torch.cuda.synchronize(dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        va, vb = _batch(dev, ua, da, A, s1), _batch(dev, ub, db, A, s2)
        vc, vd = _batch(dev, ub, db, A, s1), _batch(dev, ua, da, A, s2)
        s1.synchronize()
        s2.synchronize()
        for u, d, v in ((ua, da, va), (ub, db, vb), (ub, db, vc), (ua, da, vd)):
            assert np.array_equal(v.cpu().numpy(), m.batch(u, d))
        CC.check(A, m, device=True, what="two streams")
        A.counters_clear(device=True)
        m.clear()
        CC.check(A, m, device=True, what="cleared")
        assert A.counters()[2].tolist() == [0, 0, 0, 0]   # (the host set never counted)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_updates_in_stream_order(dev, case):
    """Every update case of the CPU file on one non-default stream with no
    synchronize between batch, update and batch: one wait at the very end, then
    the device set is the model's (and the host set, fed the same, too)."""
    with torch.cuda.device(dev):
        s = torch.cuda.Stream(dev)
        keep = []

        def batch(A, u, d):
            keep.append(_batch(dev, u, d, A, s))
            firewall.firewall_host(u, d, A)
        A, m = CC.run_steps(case, lambda r, slots: Acl.from_rules(r, slots), batch,
                            lambda A, ops: A.update(ops=ops, stream=s), lambda A, m, i: None)
        with A:
            s.synchronize()
            CC.check(A, m, device=True, what=case[0])
            CC.check(A, m, what=case[0])
            assert A.dump().tobytes() == A.dump(device=True).tobytes()
            rebuilt = any(st[0] == "update" and st[2] for st in case[3])
            slots = A.info["slots"]
            assert A.info["device_bytes"] == 20 * slots + 16 * slots + 32 + (20 * slots if rebuilt else 0)


def test_a_rebuild_between_batches_checked_at_every_step(dev):
    """The rebuild cases once more with the device set read after every step."""
    for case in CASES[3:]:
        with torch.cuda.device(dev):
            A, m = CC.run_steps(case, lambda r, slots: Acl.from_rules(r, slots), lambda A, u, d: _batch(dev, u, d, A),
                                lambda A, ops: A.update(ops=ops),
                                lambda A, m, i: CC.check(A, m, device=True, what=f"{case[0]}, step {i}"))
            A.close()


def test_lbfw_counts_each_gated_frame_once(dev):
    """xsknf_gpu_lbfw_batch with a counting ACL, the parallel path and a batch
    that takes the ordered path: both sets against the model."""
    rng = np.random.default_rng(5205)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=200, filler=100)
    umem, descs = LC.pack_packed(fl, rng)
    descs = FC.with_outside(umem, descs, rng)
    keys = WC.frame_keys(fl)
    r, d = WC.rules(keys[::3], [(0, -1, 2)[i % 3] for i in range(len(keys[::3]))])
    m = CC.Model(r)
    with torch.cuda.device(dev), lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r) as A:
        A.counters_enable()
        for i in range(2):
            m.batch(umem, descs)
            _, _, hs = GL.check_batch(dev, A, L, umem, descs, 0, 3, f"batch {i}", ordered=0)
            _, _, totals = CC.check(A, m, device=True, what=f"lbfw batch {i}")
            CC.check(A, m, what=f"lbfw batch {i}")
            assert int(totals[CC.HITS]) == (i + 1) * int(hs[WC.GATED]) > 0 and min(totals.tolist()) > 0
    # the ordered path (stats[6] > 0): a cause of it among unrelated gated frames
    rng, bk, ks, vs, fl, r, d = GL._cause_inputs("shared_b", False)
    umem, descs = LC.pack_packed(fl * 3, rng)
    m = CC.Model(r)
    with torch.cuda.device(dev), lb.LoadBalancer.from_backends(bk, max_sessions=64) as L, Acl.from_rules(r) as A:
        A.counters_enable()
        L.sessions_put(ks, vs)
        m.batch(umem, descs)
        _, _, hs = GL.check_batch(dev, A, L, umem, descs, 2, 4, "ordered", ordered=1)
        _, ctr, totals = CC.check(A, m, device=True, what="the ordered path")
        CC.check(A, m, what="the ordered path")
        assert int(totals[CC.HITS]) == int(hs[WC.GATED]) == 12 and (ctr["packets"] == 3).all()


def test_every_branch_of_the_parse_at_every_phase(dev):
    """The counting kernel restates firewall_lookup's rules 0-6: the decision
    sweep (ihl x protocol x ethertype x length) at all 16 start phases, with
    descriptors outside the UMEM among them and an ACL over a third of the keys
    that reach the map -- verdicts by the dict model, both sets by the model."""
    rng = np.random.default_rng(5206)
    fl, ph = FC.decision_frames(rng)
    umem, descs = FC.pack_unaligned(fl, rng, ph, max_gap=12)
    assert set((((descs["addr"] & ((1 << 48) - 1)) + (descs["addr"] >> 48)) % 16).tolist()) == set(range(16))
    descs = FC.with_outside(umem, descs, rng)
    keys = [k for k in FC.keys_of(umem, descs) if k is not None]
    held = list(dict.fromkeys(keys))[::3]
    rules = FC.rules_from_keys(held, [FC.ACTIONS[i % len(FC.ACTIONS)] for i in range(len(held))])
    m = CC.Model(rules)
    with torch.cuda.device(dev), Acl.from_rules(rules) as A:
        A.counters_enable()
        want = FC.model(umem, descs, FC.acl_dict(rules))
        assert np.array_equal(_batch(dev, umem, descs, A).cpu().numpy(), want)
        assert np.array_equal(m.batch(umem, descs), want)
        firewall.firewall_host(umem, descs, A)
        _, _, totals = CC.check(A, m, device=True, what="decision sweep")
        CC.check(A, m, what="decision sweep")
        assert min(totals.tolist()) > 0


def test_lbfw_batches_around_a_rebuild_in_stream_order(dev):
    """lbfw batch -> an update that rebuilds the table (the counters move to the
    other array) -> lbfw batch, on one stream with one wait at the end: the gate
    counts into the array that is current where the batch stands in the stream."""
    rng = np.random.default_rng(5207)
    bk = LC.make_backends(rng)
    fl = LC.flows_batch(rng, bk, flows=120, filler=60)
    umem, descs = LC.pack_packed(fl, rng)
    keys = WC.frame_keys(fl)[:60]
    pad = UC.keys_away(rng, 40 - 20, (), taken=keys)
    held = keys[:20] + pad                      # 40 rules in 64 slots; 20 of them see traffic
    r, _ = WC.rules(held, [(0, -1, 2)[i % 3] for i in range(40)])
    gone = held[10:20] + pad[:8]                # 18 > 64 / 4 deletes: a rebuild
    ops = UC.ops_of(UC.deletes(gone) + UC.puts(keys[20:30], [1] * 10) + UC.puts(held[:3], [2] * 3))
    m = CC.Model(r)
    n = descs.shape[0]
    with torch.cuda.device(dev), lb.LoadBalancer.from_backends(bk, max_sessions=4096) as L, Acl.from_rules(r, 64) as A:
        A.counters_enable()
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            dd = _to_dev(descs, dev)
            ws = torch.zeros(lb.lb_workspace(n), dtype=torch.uint8, device=dev)
            keep = []
            for i in range(2):
                du = _to_dev(umem, dev)
                dv = torch.zeros(n, dtype=torch.int32, device=dev)
                st = torch.zeros(8, dtype=torch.int64, device=dev)
                m.batch(umem, descs)
                lbfw.lbfw_batch_ptr(du.data_ptr(), umem.size, dd.data_ptr(), n, 0, 3, A, L, dv.data_ptr(), ws.data_ptr(),
                                    ws.numel(), st.data_ptr(), s.cuda_stream)
                keep.append((du, dv, st))
                if i == 0:
                    m.update(ops)
                    A.update(ops=ops, stream=s)
                    assert A.info["tombstones"] == 0 and A.info["rules"] == len(m.acl)
        s.synchronize()
        _, ctr, totals = CC.check(A, m, device=True, what="lbfw around a rebuild")
        assert int(keep[0][2][WC.GATED]) + int(keep[1][2][WC.GATED]) == int(totals[CC.HITS]) > 0
        assert int(ctr["packets"].max()) > 0 and A.counters()[2].tolist() == [0, 0, 0, 0]
