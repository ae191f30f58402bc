"""Long mixed runs with ageing, live backends and list drains in flight, on the
device: the two scripts of tests/churn_cases.py against the combined model,
whose expectations every op carries (tests/test_churn.py holds the host forms to
them).  The three forms are tests/test_gpu_life.py's, and so are its upload, its
enqueue of the older op kinds and its check of their outputs.

Stepwise: one synchronize after every op, then the op's outputs, the device
session dump, the device sessions_ages (keys, ages, clock) once ageing is on,
the device backends dump, the device ACL dump and the counts against the model.
A failure names the op.

Pipelined: every input is uploaded first and every op has its own workspace,
verdicts, stats and result words.  A whole segment -- batches of both NFs, ACL
updates, removals, drains, list drains, backends updates, clock settings and
expires -- is enqueued on one non-default stream behind a few milliseconds of
unrelated work, with no wait and no readback.  One synchronize ends the
segment; then every op's outputs and the four device dumps must be the model's.
A segment ends only at an op that has no stream argument (sessions_put,
aging_enable).  The device ops leave the host copies alone where the header
says so: the host session table holds what the puts stored and nothing else, at
clock 0; the host copy of the backends is the newest at once.  The churn script
runs once more with the ops alternating between two streams, each op ordered
behind the one before it by an event."""
import numpy as np
import pytest

from tests import churn_cases as CH
from tests import test_gpu_life as GL
from xsknf_amd import firewall, lb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D, H = lb.DEVICE_TABLE, lb.HOST_TABLE
MIN_SEGMENT = GL.MIN_SEGMENT
NAMES = ["aged", "churn"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def objects(S, dev):
    L, A = GL.objects(S, dev)
    if S.enable_first:
        L.aging_enable()
    return L, A


def enqueue(op, b, L, A, stream):
    """The op on the device tables, on `stream`; nothing waits.  Returns its output tensors."""
    if op.kind == "clock":
        return L.clock(op.now, which=D, stream=stream)
    if op.kind == "backends_update":
        return L.backends_update(ops=op.ops, stream=stream)
    with torch.cuda.stream(stream):
        if op.kind == "expire":
            return L.expire(op.max_idle, stream=stream)
        if op.kind == "drain_backends":
            return L.drain_backends(op.ids, stream=stream)
    return GL.enqueue(op, b, L, A, stream)


def check_outputs(op, b, out, mode):
    """After a synchronize: what the op wrote against the model."""
    if op.kind in ("expire", "drain_backends"):
        w = op.want
        assert out.cpu().tolist() == w.result.tolist(), \
            f"{mode}: {CH.describe(op)}: result {out.cpu().tolist()} != {w.result.tolist()}"
    elif op.kind not in ("clock", "backends_update"):
        GL.check_outputs(op, b, out, mode)


def check_tables(op, L, A, mode):
    """The device tables after `op` (the dumps wait for the device)."""
    what = f"{mode}: {CH.describe(op)}"
    bad = CH.same_tables(op, L, A, D, A.dump(device=True))
    assert not bad, f"{what}: {bad}"
    i = L.info
    assert i["device_sessions"] == op.want.n_sessions, f"{what}: device_sessions {i['device_sessions']}"
    assert (i["services"], i["backends"]) == (op.want.n_services, op.want.n_backends), f"{what}: {i}"


class HostSide:
    """What the host copies hold while only device ops run: the sessions the puts
    stored, at clock 0 (sessions_put writes both tables, aging_enable gives both
    their stamps, and no device op touches the host table or its clock)."""

    def __init__(self, S):
        self.M = CH.Sessions(S.backends, S.shape.max_sessions, S.shape.slots)
        self.aging = S.enable_first

    def segment_end(self, op):
        if op.kind == "sessions_put":
            self.M.sessions_put(op.keys, op.values)
        else:
            self.aging = True

    def check(self, op, L, A, mode):
        what = f"{mode}: after {CH.describe(op)}: the host"
        k, v = L.sessions_dump(H)
        mk, mv = self.M.dump()
        assert k.tobytes() == mk.tobytes() and v.tobytes() == mv.tobytes(), f"{what} session table changed"
        if self.aging:
            k, a, clock = L.sessions_ages(H)
            assert clock == 0 and k.tobytes() == mk.tobytes() and not a.any(), f"{what} table's clock or stamps changed"
        assert L.backends_dump(H).tobytes() == op.want.backends, f"{what} copy of the backends is not the newest"
        assert A.dump().tobytes() == op.want.acl_rules.tobytes(), f"{what} copy of the ACL is not the newest"


@pytest.mark.parametrize("name", NAMES)
def test_stepwise(dev, name):
    S = CH.script(name)
    L, A = objects(S, dev)
    with L, A:
        stream = torch.cuda.Stream(dev)
        for op in S.ops:
            if op.kind == "sessions_put":
                L.sessions_put(op.keys, op.values)
            elif op.kind == "aging_enable":
                L.aging_enable()
            else:
                b = GL.upload(op, dev)
                torch.cuda.synchronize()
                out = enqueue(op, b, L, A, stream)
                torch.cuda.synchronize()
                check_outputs(op, b, out, "stepwise")
            check_tables(op, L, A, "stepwise")
            if op.kind == "acl_update":
                assert A.info["tombstones"] == op.want.acl_tombstones, CH.describe(op)


def pipelined(S, dev, streams, mode):
    L, A = objects(S, dev)
    host = HostSide(S)
    with L, A:
        bufs = [GL.upload(op, dev) for op in S.ops]
        ballast = torch.zeros(1 << 26, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for ops, end in CH.segments(S):
            assert len(ops) >= MIN_SEGMENT
            with torch.cuda.stream(streams[0]):
                for _ in range(160):                   # unrelated work the segment queues up behind
                    ballast.add_(1)
            outs, last = [], streams[0]
            for i, op in enumerate(ops):
                s = streams[i % len(streams)]
                if s is not last:                      # ordered behind the op before it, on the device alone
                    done = torch.cuda.Event()
                    done.record(last)
                    s.wait_event(done)
                outs.append(enqueue(op, bufs[op.index], L, A, s))
                last = s
            torch.cuda.synchronize()                   # the segment's one wait
            for op, out in zip(ops, outs):
                check_outputs(op, bufs[op.index], out, mode)
            check_tables(ops[-1], L, A, mode)
            host.check(ops[-1], L, A, mode)
            if end is not None:
                if end.kind == "sessions_put":
                    L.sessions_put(end.keys, end.values)
                else:
                    L.aging_enable()
                host.segment_end(end)
                check_tables(end, L, A, mode)
                host.check(end, L, A, mode)
        assert A.info["tombstones"] == S.ops[-1].want.acl_tombstones


@pytest.mark.parametrize("name", NAMES)
def test_pipelined_on_one_stream(dev, name):
    pipelined(CH.script(name), dev, [torch.cuda.Stream(dev)], "pipelined")


def test_pipelined_across_two_streams(dev):
    pipelined(CH.script("churn"), dev, [torch.cuda.Stream(dev), torch.cuda.Stream(dev)], "two streams")
