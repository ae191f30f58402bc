"""Long mixed runs with ageing, live backends and list drains, host forms: the
two scripts of tests/churn_cases.py -- about 240 batches of both NFs, ACL
updates, removals, drains, list drains, backends updates, clock settings and
expires on one LoadBalancer and one Acl -- through lb_host, lbfw_host,
firewall_host and the HOST_TABLE form of every other call.  After EVERY op the
outputs, the session dump, sessions_ages (keys, ages and the clock, once ageing
is on), the backends dump, the ACL dump and the info counts equal the combined
model.  What the scripts exercise is computed from the model and asserted here,
with the bounds of lb_table.h: live sessions plus tombstones never pass 3/4 of
the slots, tombstones never slots / 4.  tests/test_gpu_churn.py holds the device
tables to the same scripts."""
import pytest

from tests import churn_cases as CH
from tests import life_cases as LF
from xsknf_amd import firewall, lb

NAMES = ["aged", "churn"]


@pytest.mark.parametrize("name", NAMES)
def test_the_script_covers_what_it_is_for(name):
    S = CH.script(name)
    cov = CH.coverage(S)
    print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in sorted(cov.items())))
    assert len(S.ops) >= 240
    assert not CH.coverage_gaps(S, cov), CH.coverage_gaps(S, cov)
    kinds = {op.kind for op in S.ops}
    assert kinds == {"lb_batch", "lbfw_batch", "firewall_batch", "acl_update", "sessions_remove", "drain_backend",
                     "sessions_clear", "sessions_put", "clock", "expire", "backends_update", "drain_backends"} | \
        ({"aging_enable"} if name == "churn" else set())
    assert S.enable_first == (name == "aged")
    assert {op.gate for op in S.ops if op.kind == "lbfw_batch"} == {True, False}
    sizes = [op.descs.shape[0] for op in S.ops if op.kind in CH.BATCHES]
    assert min(sizes) < 256 < max(sizes)       # both sides of the 256-lane tile
    assert all(len(seg) >= 32 for seg, _ in CH.segments(S))
    # the bounds of lb_table.h, from the model's counts after every op
    assert cov["max_live_plus_tombstones"] <= 3 * S.shape.slots // 4
    assert cov["max_tombstones"] <= S.shape.slots // 4
    for op in S.ops:
        assert op.want.n_sessions <= S.shape.max_sessions and op.want.tombstones <= S.shape.slots // 4, CH.describe(op)


@pytest.mark.parametrize("name", NAMES)
def test_host_forms_follow_the_model_op_by_op(name):
    S = CH.script(name)
    H = lb.HOST_TABLE
    with lb.LoadBalancer.from_backends(S.backends, S.shape.max_sessions, S.shape.slots) as L, \
            firewall.Acl.from_rules(S.rules, S.shape.acl_slots) as A:
        assert A.info["rules"] == S.shape.acl_initial and A.info["tombstones"] == 0
        if S.enable_first:
            L.aging_enable()
        for op in S.ops:
            w, what = op.want, CH.describe(op)
            got = CH.run_host(op, L, A)
            if op.kind in CH.BATCHES:
                bad = LF.same_batch(op, *got, w.host_stats)
                assert not bad, f"{what}: {bad}"
            elif op.kind == "firewall_batch":
                assert got.tolist() == w.verdicts.tolist(), f"{what}: the verdicts differ"
            elif op.kind in CH.REMOVALS:
                assert got.tolist() == w.result.tolist(), f"{what}: result {got.tolist()} != {w.result.tolist()}"
            bad = CH.same_tables(op, L, A, H, A.dump())
            assert not bad, f"{what}: {bad}"
            li, ai = L.info, A.info
            assert li["host_sessions"] == w.n_sessions, f"{what}: host_sessions {li['host_sessions']} != {w.n_sessions}"
            assert (li["services"], li["backends"]) == (w.n_services, w.n_backends), \
                f"{what}: the info {li} != {w.n_services} services, {w.n_backends} backends"
            assert (ai["rules"], ai["tombstones"]) == (w.acl_rules.shape[0], w.acl_tombstones), \
                f"{what}: the ACL's info {ai} != {w.acl_rules.shape[0]} rules, {w.acl_tombstones} tombstones"
            assert w.n_sessions + w.tombstones <= 3 * S.shape.slots // 4, what
