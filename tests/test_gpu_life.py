"""A long mixed run on live tables, on the device: the two scripts of
tests/life_cases.py -- about 200 batches, ACL updates, removals, drains, a clear
and puts on one LoadBalancer and one Acl -- against the combined model, whose
expectations every op carries (tests/test_life.py holds the host forms to them).

Stepwise: one synchronize after every op, then the op's outputs, both device
dumps and the session count against the model.  A failure names the op.

Pipelined: every UMEM and descriptor array is uploaded first and every op has
its own workspace, verdicts, stats and result words.  A whole segment of ops is
enqueued on one non-default stream with no wait and no readback; the stream
starts behind a few milliseconds of unrelated work, so the queue is dozens of
calls deep while the host picks its stages (acl_stage_acquire, stage_acquire).
One synchronize ends the segment; then every op's outputs and the dumps must be
the model's.  A segment ends only at an op that has no stream argument
(sessions_put).  The wide script runs once more with the ops alternating
between two streams, each op ordered behind the one before it by an event:
the ordering kernel_lb_remove.h's compaction asks for."""
import types

import numpy as np
import pytest

from tests import life_cases as LF
from xsknf_amd import firewall, lb, lbfw

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D = lb.DEVICE_TABLE
MIN_SEGMENT = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def objects(S, dev):
    return (lb.LoadBalancer.from_backends(S.backends, S.shape.max_sessions, S.shape.slots, device=dev),
            firewall.Acl.from_rules(S.rules, S.shape.acl_slots, device=dev))


def upload(op, dev):
    """The op's inputs on the device, and a workspace of its own."""
    b = types.SimpleNamespace()
    if hasattr(op, "umem"):
        b.umem = torch.from_numpy(op.umem).to(dev)      # (a copy: the script's arrays stay as they are)
        b.descs = torch.from_numpy(op.descs.view(np.uint8).reshape(-1, 16).copy()).to(dev)
        if op.kind in LF.BATCHES:
            b.ws = torch.empty(lb.lb_workspace(op.descs.shape[0]), dtype=torch.uint8, device=dev)
    return b


def enqueue(op, b, L, A, stream):
    """The op on the device tables, on `stream`; nothing waits.  Returns its output tensors."""
    with torch.cuda.stream(stream):
        if op.kind == "lb_batch":
            return lb.lb_batch(b.umem, b.descs, L, op.ingress, op.nif, workspace=b.ws)
        if op.kind == "lbfw_batch":
            return lbfw.lbfw_batch(b.umem, b.descs, A if op.gate else None, L, op.ingress, op.nif, workspace=b.ws)
        if op.kind == "firewall_batch":
            return firewall.firewall_batch(b.umem, b.descs, A)
        if op.kind == "acl_update":
            return A.update(ops=op.ops, stream=stream)
        if op.kind == "sessions_remove":
            return L.sessions_remove(op.keys, pair=op.pair, stream=stream)
        if op.kind == "drain_backend":
            return L.drain_backend(op.addr, op.port, op.proto, stream=stream)
        if op.kind == "sessions_clear":
            return L.sessions_clear(D, stream=stream)
    raise ValueError(op.kind)


def check_outputs(op, b, out, mode):
    """After a synchronize: what the op wrote against the model."""
    w, what = op.want, f"{mode}: {LF.describe(op)}"
    if op.kind in LF.BATCHES:
        bad = LF.same_batch(op, out[0].cpu().numpy(), b.umem.cpu().numpy(), out[1].cpu().tolist(), w.stats)
        assert not bad, f"{what}: {bad}"
    elif op.kind == "firewall_batch":
        assert out.cpu().tolist() == w.verdicts.tolist(), f"{what}: the verdicts differ"
        assert np.array_equal(b.umem.cpu().numpy(), op.umem), f"{what}: the firewall wrote to the UMEM"
    elif op.kind in LF.REMOVALS:
        assert out.cpu().tolist() == w.result.tolist(), f"{what}: result {out.cpu().tolist()} != {w.result.tolist()}"


def check_tables(op, L, A, mode):
    """The device tables after `op` (the dumps wait for the device)."""
    what = f"{mode}: {LF.describe(op)}"
    bad = LF.same_tables(op, L.sessions_dump(D), A.dump(device=True))
    assert not bad, f"{what}: {bad}"
    n = L.info["device_sessions"]
    assert n == op.want.n_sessions, f"{what}: device_sessions {n} != {op.want.n_sessions}"


@pytest.mark.parametrize("name", ["small", "wide"])
def test_stepwise(dev, name):
    S = LF.script(name)
    L, A = objects(S, dev)
    with L, A:
        stream = torch.cuda.Stream(dev)
        for op in S.ops:
            if op.kind == "sessions_put":
                L.sessions_put(op.keys, op.values)
            else:
                b = upload(op, dev)
                torch.cuda.synchronize()
                out = enqueue(op, b, L, A, stream)
                torch.cuda.synchronize()
                check_outputs(op, b, out, "stepwise")
            check_tables(op, L, A, "stepwise")
            if op.kind == "acl_update":
                assert A.info["tombstones"] == op.want.acl_tombstones, LF.describe(op)


def segments(S):
    """The script cut at its ops without a stream argument: [(ops, the put that ends them or None)]."""
    out, cur = [], []
    for op in S.ops:
        if op.kind == "sessions_put":
            out.append((cur, op))
            cur = []
        else:
            cur.append(op)
    out.append((cur, None))
    return out


def pipelined(S, dev, streams, mode):
    L, A = objects(S, dev)
    with L, A:
        bufs = [upload(op, dev) for op in S.ops]
        ballast = torch.zeros(1 << 26, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for ops, put in segments(S):
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
            if put is not None:
                L.sessions_put(put.keys, put.values)
                check_tables(put, L, A, mode)
        assert A.info["tombstones"] == S.ops[-1].want.acl_tombstones


@pytest.mark.parametrize("name", ["small", "wide"])
def test_pipelined_on_one_stream(dev, name):
    pipelined(LF.script(name), dev, [torch.cuda.Stream(dev)], "pipelined")


def test_pipelined_across_two_streams(dev):
    pipelined(LF.script("wide"), dev, [torch.cuda.Stream(dev), torch.cuda.Stream(dev)], "two streams")
