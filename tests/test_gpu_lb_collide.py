"""The load balancer's and lbfw's device kernels (xsknf_amd/csrc/kernel_lb.h) on
keys chosen by their home slot (tests/lb_collide_cases.py), against the host
model through check_batch of tests/test_gpu_lb.py and tests/test_gpu_lbfw.py
(every UMEM byte, verdict and counter, the session dump, the sentinels past n,
the descriptors, a garbage workspace; tests/test_lb_collide.py holds the host
model to the dict model on the same batches).  What random keys never reach:
staging chains in which lanes of every block lose their compare-and-swap to
other keys and walk on, probes that wrap from the last slot to slot 0 in stage,
staged, commit_one and lb::find, staged() lookups deep in a chain, many lanes
claiming slots of one session-table cluster, and the parallel path's boundary
sessions + new_keys == max_sessions.  Each test asserts its premise with the
chain model."""
import numpy as np
import pytest

from tests import firewall_cases as FC
from tests import lb_cases as LC
from tests import lb_collide_cases as CC
from tests import lbfw_cases as WC
from tests.test_gpu_lb import check_batch
from tests.test_gpu_lbfw import check_batch as lbfw_check_batch
from xsknf_amd import lb
from xsknf_amd.firewall import Acl

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T = LC.code_constant(r"constexpr int kThreads = (\d+);")   # frames per block and step
I, NIF = CC.INGRESS, CC.NIF
CREATED, FAILED = lb.LB_STATS.index("sessions_created"), lb.LB_STATS.index("inserts_failed")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def backward_macs(L, bk):
    """{client (saddr, sport): the MAC its backward session carries} from the device table."""
    k, v = L.sessions_dump(lb.DEVICE_TABLE)
    back = v["dir"] == lb.TO_CLIENT
    assert (k["saddr"][back] == int(bk[0]["addr"])).all()
    return {(int(a), int(p)): m.tolist() for a, p, m in zip(k["daddr"][back], k["dport"][back], v["mac"][back])}


def check_flows(b, bk, hv, L, known=()):
    """The verdicts say which backward frames passed and which were rewritten,
    and every backward session carries the MAC of its flow's lowest-index frame."""
    want = b.expected_verdicts(bk, known)
    bad = [i for i, x in want.items() if int(hv[i]) != x]
    assert not bad, f"verdicts at {bad[:8]}"
    macs = backward_macs(L, bk)
    first = b.creators()
    assert len(macs) >= len(first)
    wrong = [sid for sid, i in first.items() if macs[(sid[0], sid[2])] != b.mac[i]]
    assert not wrong, f"{len(wrong)} backward sessions carry a later frame's MAC"


@pytest.mark.parametrize("variant", ["two_frames", "backward"])
def test_smallest_staging_table(dev, variant):
    """Sixteen frames, 64 staging slots, 16 keys homed in slots 62, 63, 0, 1: one
    chain of 16 slots that wraps, also in the session table of 64 slots."""
    bk, b = CC.small_case(variant)
    keys = b.staged_keys(bk)
    assert b.n <= 16 and CC.stage_slots(b.n) == 64 and len(set(keys)) == 16
    assert {h & 63 for h in CC.hash_keys(keys)} <= {62, 63, 0, 1}
    c = CC.chain_of(keys, 64)
    assert c.wraps >= 1 and c.longest >= 8
    umem, descs = b.arrays()
    with lb.LoadBalancer.from_backends(bk, max_sessions=32, slots=64) as L:
        hv, hs = check_batch(dev, L, umem, descs, I, NIF, variant, ordered=0)
        assert int(hs[CREATED]) == 16 and L.info["device_sessions"] == 16
        check_flows(b, bk, hv, L)
        if variant == "backward":
            want = b.expected_verdicts(bk)
            assert sorted(want[i] for i, t in enumerate(b.what) if t[0] == "b") == [I, I, CC.PASS_IFACE, CC.PASS_IFACE]
        hv2, hs2 = check_batch(dev, L, umem, descs, I, NIF, variant + " again", ordered=0)
        assert int(hs2[CREATED]) == 0 and int(hs2[1]) == 16


@pytest.mark.parametrize("reverse", [False, True])
def test_one_cluster_claimed_from_every_block(dev, reverse):
    """Sixteen blocks stage 512 keys of one 16-slot window across the staging
    table's end (and 512 scattered ones); lb_commit stores them into one cluster
    across the end of the session table.  Backward frames ahead of their
    creator pass, those after it are rewritten from the staged record deep in
    the chain.  The same batch again finds every session.  reverse: the same
    frames in the opposite order, so that each flow's last frame is its creator."""
    bk, b, fl = CC.grid_case(T, reverse)
    n, first = b.n, b.creators()
    assert n == 16 * T and len(first) == 512
    blocks = [{i // T for i, t in enumerate(b.what) if t == ("f", sid)} for sid in fl]
    assert all(2 <= len(x) <= 3 for x in blocks)   # every frame of a flow in a block of its own
    assert len({i // T for i in first.values()}) >= 15 and set().union(*blocks) == set(range(16))
    keys = b.staged_keys(bk)
    M = CC.stage_slots(n)
    assert int(CC.in_window(np.array(CC.hash_keys(keys)), M, 16).sum()) == 512
    c = CC.chain_of(keys, M)
    assert c.wraps >= 1 and c.longest >= 256
    cs = CC.chain_of(keys, 8192)
    assert cs.wraps >= 1 and cs.longest >= 256
    want = b.expected_verdicts(bk)
    back = [want[i] for i, t in enumerate(b.what) if t is not None and t[0] == "b"]
    assert back.count(CC.PASS_IFACE) >= 64 and back.count(I) >= 200
    # backward frames that follow their creator and whose key lies deep in the staging chain
    deep = [i for i, t in enumerate(b.what) if t is not None and t[0] == "b" and want[i] == I
            and c.find(CC.bwd_key(bk, t[1]))[0] >= 64]
    assert len(deep) >= 50
    umem, descs = b.arrays()
    with lb.LoadBalancer.from_backends(bk, max_sessions=4096, slots=8192) as L:
        hv, hs = check_batch(dev, L, umem, descs, I, NIF, "first batch", ordered=0)
        assert int(hs[CREATED]) == 1024 and int(hs[FAILED]) == 0
        check_flows(b, bk, hv, L)
        hv2, hs2 = check_batch(dev, L, umem, descs, I, NIF, "second batch", ordered=0)
        assert int(hs2[CREATED]) == 0 and int(hs2[1]) == len(want) and int(hs2[2]) == n - len(want)
        check_flows(b, bk, hv2, L, known=set(first))


def test_deep_session_table_chains(dev):
    """lb_propose's lb::find over a cluster of 300 stored sessions across the
    end of a 1024-slot table: every stored key hit, absent keys of the same
    homes run to the chain's end, and 100 new flows are committed into it."""
    bk, pre, b, stored, absent, new = CC.deep_case()
    pk = [CC.fwd_key(s) for s in stored]
    c = CC.chain_of(pk, 1024)
    assert c.longest >= 256 and c.wraps >= 1
    assert min(c.find(CC.fwd_key(s))[0] for s in absent + new) >= 64
    umem, descs = b.arrays()
    with lb.LoadBalancer.from_backends(bk, max_sessions=512, slots=1024) as L:
        L.sessions_put(*pre)
        hv, hs = check_batch(dev, L, umem, descs, I, NIF, "deep", ordered=0)
        assert [int(x) for x in hs[:6]] == [640, 450, 190, 0, 200, 0] and L.info["device_sessions"] == 500
        hv2, hs2 = check_batch(dev, L, umem, descs, I, NIF, "deep again", ordered=0)
        assert [int(x) for x in hs2[:6]] == [640, 450, 190, 0, 0, 0]


@pytest.fixture(scope="module")
def capacity():
    d = CC.capacity_case()
    new_keys = d["exact"].staged_keys(d["bk"])
    assert d["pre"][0].shape[0] + len(new_keys) == d["max_sessions"] and len(set(new_keys)) == len(new_keys) == 200
    assert sum(1 for t in d["exact"].what if t is not None and t[0] == "f") > 200   # more frames than keys
    c = CC.chain_of(new_keys, CC.stage_slots(d["exact"].n))
    assert c.longest >= 64 and c.wraps >= 1
    return d


def test_exact_fit_stays_parallel_and_one_more_key_stands_down(dev, capacity):
    """sessions + new_keys == max_sessions runs the parallel path; the full
    table then takes the same batch (no new key) on the parallel path too; one
    further flow stands down, fails its forward insert and skips the backward
    one."""
    d = capacity
    with lb.LoadBalancer.from_backends(d["bk"], max_sessions=d["max_sessions"], slots=d["slots"]) as L:
        L.sessions_put(*d["pre"])
        umem, descs = d["exact"].arrays()
        hv, hs = check_batch(dev, L, umem, descs, I, NIF, "exact fit", ordered=0)
        assert int(hs[CREATED]) == 200 and int(hs[FAILED]) == 0
        assert L.info["device_sessions"] == d["max_sessions"]
        hv, hs = check_batch(dev, L, umem, descs, I, NIF, "exact fit again", ordered=0)
        assert int(hs[CREATED]) == 0 and int(hs[FAILED]) == 0
        assert d["extra"].n <= 4096
        hv, hs = check_batch(dev, L, *d["extra"].arrays(), I, NIF, "one more flow", ordered=1)
        assert int(hs[CREATED]) == 0 and int(hs[FAILED]) == 1
        assert L.info["device_sessions"] == d["max_sessions"]


def test_one_slot_short_stands_down(dev, capacity):
    d = capacity
    with lb.LoadBalancer.from_backends(d["bk"], max_sessions=d["max_sessions"] - 1, slots=d["slots"]) as L:
        L.sessions_put(*d["pre"])
        hv, hs = check_batch(dev, L, *d["exact"].arrays(), I, NIF, "one short", ordered=1)
        assert int(hs[CREATED]) == 199 and int(hs[FAILED]) >= 1
        assert L.info["device_sessions"] == d["max_sessions"] - 1


def test_gated_flows_take_no_room(dev, capacity):
    """lbfw: the exact-fit batch with 20 further new flows of the same staging
    window that the ACL holds.  They stage nothing: the batch still fits."""
    d = capacity
    with lb.LoadBalancer.from_backends(d["bk"], max_sessions=d["max_sessions"], slots=d["slots"]) as L, \
            Acl.from_rules(d["rules"]) as A:
        L.sessions_put(*d["pre"])
        hu, hv, hs = lbfw_check_batch(dev, A, L, *d["gated"].arrays(), I, NIF, "gated", ordered=0)
        assert int(hs[WC.GATED]) == d["gated_frames"] and int(hs[CREATED]) == 200 and int(hs[FAILED]) == 0
        assert L.info["device_sessions"] == d["max_sessions"]


def test_lbfw_through_a_clustered_acl(dev):
    """600 rules of one 16-slot window across the end of a 1024-slot ACL: the
    gate's probe runs hundreds of slots and wraps, for the rules' frames and
    for near misses that go on to the load balancer.  Against the host and the
    dict model."""
    bk, rules, ruled, pre, b, new = CC.acl_cluster_case()
    c = CC.chain_of([CC.fwd_key(s) for s in ruled], 1024)
    assert c.longest >= 256 and c.wraps >= 1 and 0 in rules["action"].tolist()
    umem, descs = b.arrays()
    m = WC.Model(bk, 1024)
    m.sessions_put(*pre)
    mu = umem.copy()
    mv, ms = m.batch(mu, descs, I, NIF, FC.acl_dict(rules))
    with lb.LoadBalancer.from_backends(bk, max_sessions=1024, slots=2048) as L, Acl.from_rules(rules, slots=1024) as A:
        assert A.info["max_probe"] == c.longest
        L.sessions_put(*pre)
        hu, hv, hs = lbfw_check_batch(dev, A, L, umem, descs, I, NIF, "clustered ACL", ordered=0)
        assert np.array_equal(hv, mv) and np.array_equal(hu, mu) and np.array_equal(hs, ms)
        assert int(hs[WC.GATED]) == 600 and int(hs[CREATED]) == 240
        k, v = L.sessions_dump(lb.DEVICE_TABLE)
        mk, mw = m.dump()
        assert k.tobytes() == mk.tobytes() and v.tobytes() == mw.tobytes()
