"""A long mixed run on live tables, host forms: the two scripts of
tests/life_cases.py -- about 200 batches, ACL updates, removals, drains, a clear
and puts on one LoadBalancer and one Acl -- through lb_host, lbfw_host,
firewall_host, Acl.update's host table and the _host removals.  After EVERY op
the outputs, both dumps and the counts equal the combined model.  The scripts'
coverage (compactions, rebuilds, stand-downs over tombstones, keys created
again, ...) is computed from the model and asserted here, and so is the bound
lb_table.h states: live sessions plus tombstones never pass 3/4 of the slots.
tests/test_gpu_life.py holds the device tables to the same scripts."""
import pytest

from tests import life_cases as LF
from xsknf_amd import firewall, lb


@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_script_covers_what_it_is_for(name):
    S = LF.script(name)
    cov = LF.coverage(S)
    print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in sorted(cov.items())))
    assert len(S.ops) >= 200
    assert not LF.coverage_gaps(S, cov), LF.coverage_gaps(S, cov)
    kinds = {op.kind for op in S.ops}
    assert kinds == {"lb_batch", "lbfw_batch", "firewall_batch", "acl_update", "sessions_remove", "drain_backend",
                     "sessions_clear", "sessions_put"}
    assert {op.gate for op in S.ops if op.kind == "lbfw_batch"} == {True, False}
    sizes = [op.descs.shape[0] for op in S.ops if op.kind in LF.BATCHES]
    assert min(sizes) < 256 < max(sizes)       # both sides of the 256-lane tile
    # the bound of lb_table.h, from the model's counts after every op
    assert cov["max_live_plus_tombstones"] <= 3 * S.shape.slots // 4
    for op in S.ops:
        assert op.want.n_sessions <= S.shape.max_sessions and op.want.tombstones <= S.shape.slots // 4, LF.describe(op)


@pytest.mark.parametrize("name", ["small", "wide"])
def test_host_forms_follow_the_model_op_by_op(name):
    S = LF.script(name)
    with lb.LoadBalancer.from_backends(S.backends, S.shape.max_sessions, S.shape.slots) as L, \
            firewall.Acl.from_rules(S.rules, S.shape.acl_slots) as A:
        assert A.info["rules"] == S.shape.acl_initial and A.info["tombstones"] == 0
        for op in S.ops:
            w, what = op.want, LF.describe(op)
            got = LF.run_host(op, L, A)
            if op.kind in LF.BATCHES:
                bad = LF.same_batch(op, *got, w.host_stats)
                assert not bad, f"{what}: {bad}"
            elif op.kind == "firewall_batch":
                assert got.tolist() == w.verdicts.tolist(), f"{what}: the verdicts differ"
            elif op.kind in LF.REMOVALS:
                assert got.tolist() == w.result.tolist(), f"{what}: result {got.tolist()} != {w.result.tolist()}"
            bad = LF.same_tables(op, L.sessions_dump(lb.HOST_TABLE), A.dump())
            assert not bad, f"{what}: {bad}"
            li, ai = L.info, A.info
            assert li["host_sessions"] == w.n_sessions, f"{what}: host_sessions {li['host_sessions']} != {w.n_sessions}"
            assert (ai["rules"], ai["tombstones"]) == (w.acl_rules.shape[0], w.acl_tombstones), \
                f"{what}: the ACL's info {ai} != {w.acl_rules.shape[0]} rules, {w.acl_tombstones} tombstones"
            assert w.n_sessions + w.tombstones <= 3 * S.shape.slots // 4, what
