"""Every branch of XSKNF_GPU_PATH_STAGED's copy plan (stage_frames(),
xsknf_amd/csrc/host_path.hip) on frames that change between the batches of one
context.

The STAGED kernel reads a device mirror that the plan fills piece by piece; a
copy the plan forgot makes no fault, the kernel sums what the mirror held.  So
each test here keeps ONE context, rewrites the UMEM between its batches
(tests/staged_cases.py rounds(): every summed frame's check differs from the
round before) and compares, bit for bit, the verdicts and every UMEM byte with
the oracle, and the bytes_h2d / bytes_d2h the call added to the context's
counters with the plan model's: the counters are how a test sees which branch
ran.  tests/test_staged_cases.py holds the cases to their branches on the CPU.
"""
import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import staged_cases as SC
from xsknf_amd import Checksummer, ChecksummerOptions, HostPath, frames

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x57A6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def checksummer(checks):
    return Checksummer(ChecksummerOptions(action=O.REDIRECT, csum_iterations=SC.iters_of(checks)),
                       num_interfaces=SC.NIF, frame_len_hint=1500)


def same(got_v, got_u, want_v, want_u, what):
    bad = np.flatnonzero(got_v != want_v)
    assert bad.size == 0, (f"{what}: {bad.size} verdicts differ, first at {bad[:8]}: {got_v[bad[:8]]} != "
                           f"{want_v[bad[:8]]}")
    bad = np.flatnonzero(got_u != want_u)
    assert bad.size == 0, (f"{what}: {bad.size} UMEM bytes differ, first at {bad[:8]}: {got_u[bad[:8]]} != "
                           f"{want_u[bad[:8]]}")


def moved(before, after, descs, umem_size, max_batch, what):
    """The counters the call moved against the model's, exactly."""
    h2d, d2h, branches = SC.counters(descs, umem_size, max_batch)
    got = (after["bytes_h2d"] - before["bytes_h2d"], after["bytes_d2h"] - before["bytes_d2h"])
    assert got == (h2d, d2h), f"{what}: bytes_h2d / bytes_d2h moved by {got}, the plan {branches} moves {(h2d, d2h)}"
    assert after["frames"] - before["frames"] == descs.shape[0]
    assert after["batches"] - before["batches"] == len(branches)


def run_rounds(name, rs, path, checks, umem, n_max):
    _, _, branch = SC.case(name)
    with HostPath(checksummer(checks), umem, path=path, max_batch=n_max) as hp:
        for r, rd in enumerate(rs):
            what = f"{name} {checks} {path} round {r}"
            umem[:] = rd.umem
            before = hp.stats()
            v = hp.process_batch(rd.descs, ingress_ifindex=SC.INGRESS, verdicts=np.full(rd.descs.shape[0], 7,
                                                                                         dtype=np.int32))
            after = hp.stats()
            same(v, umem, rd.want_verdicts, rd.want_umem, what)
            if path == "staged":
                assert SC.plan(rd.descs, umem.size)[0] == branch, what
                moved(before, after, rd.descs, umem.size, n_max, what)


@pytest.mark.parametrize("name", SC.EACH)
def test_each_case_over_three_rounds(dev, name):
    """One STAGED context per case and kind of checks, three batches over the
    same slots with the frames rewritten in between: zero checks under three
    iterations, then a NIC's checks under one.  A ZEROCOPY context takes the
    same rounds first, as a control on the expectations (its byte counters
    follow no plan)."""
    umem0, _, branch = SC.case(name)
    assert SC.plan(SC.case(name)[1], umem0.size)[0] == branch          # (2d-past-end: before any launch)
    umem = np.empty_like(umem0)
    for checks in ("zero", "nic"):
        rs = SC.rounds(name, 3, SEED, checks)
        for path in ("zerocopy", "staged"):
            run_rounds(name, rs, path, checks, umem, SC.max_batch(name))


def test_branches_alternate_on_one_context(dev):
    """One 16 MiB UMEM, one context, branch after branch over overlapping slots:
    a mapped piece leaves its checks in host memory alone, so the mirror-backed
    piece after it must copy those frames afresh, and the mapped piece after a
    mirror-backed one must not read the mirror."""
    for checks in ("zero", "nic"):
        steps = SC.alternating(SEED, checks)
        umem = np.empty(SC.UMEM_MAX, dtype=np.uint8)
        with HostPath(checksummer(checks), umem, path="staged", max_batch=4200) as hp:
            for j, (u, descs, branch, wu, wv) in enumerate(steps):
                what = f"{checks} step {j} ({SC.ALTERNATE[j]}, {branch})"
                umem[:] = u
                assert SC.plan(descs, umem.size)[0] == branch
                before = hp.stats()
                v = hp.process_batch(descs, ingress_ifindex=SC.INGRESS)
                moved(before, hp.stats(), descs, umem.size, 4200, what)
                same(v, umem, wv, wu, what)


def test_interleaved_batches_in_flight(dev):
    """1,200 packed frames, batch j = frames j, j + 4, ..: four batches submitted
    back to back and waited for once.  Each batch is one run that covers the
    other three batches' frames while those are in flight; three rounds with the
    frames rewritten."""
    nb = SC.INTERLEAVED_BATCHES
    assert nb < SC.constants()["slots"]
    rs = SC.rounds("interleaved-packed", 3, SEED)
    umem = np.empty_like(rs[0].umem)
    with HostPath(checksummer("zero"), umem, path="staged", max_batch=4200) as hp:
        for r, rd in enumerate(rs):
            umem[:] = rd.umem
            subs = [np.ascontiguousarray(rd.descs[j::nb]) for j in range(nb)]
            outs = [np.full(s.shape[0], 7, dtype=np.int32) for s in subs]
            before = hp.stats()
            tickets = [hp.submit(s, o, ingress_ifindex=SC.INGRESS) for s, o in zip(subs, outs)]
            hp.wait(tickets[-1])
            after = hp.stats()
            v = np.empty(rd.descs.shape[0], dtype=np.int32)
            for j, o in enumerate(outs):
                v[j::nb] = o
            same(v, umem, rd.want_verdicts, rd.want_umem, f"interleaved round {r}")
            want = [SC.counters(s, umem.size, 4200) for s in subs]
            assert all(w[2] == [SC.RUNS] for w in want)
            got = (after["bytes_h2d"] - before["bytes_h2d"], after["bytes_d2h"] - before["bytes_d2h"])
            plan = (sum(w[0] for w in want), sum(w[1] for w in want))
            assert got == plan, (f"interleaved round {r}: bytes_h2d / bytes_d2h moved by {got}, four single runs "
                                 f"move {plan}")
            assert after["batches"] - before["batches"] == nb


def test_piece_cut(dev):
    """kPiece + 1 frames under max_batch = kPiece + 1: two pieces, one run each,
    the second of one frame; one round through process_batch, one through
    submit / wait."""
    n = SC.constants()["piece"] + 1
    rs = SC.rounds("piece-cut", 2, SEED)
    assert rs[0].descs.shape[0] == n and SC.counters(rs[0].descs, rs[0].umem.size, n)[2] == [SC.RUNS, SC.RUNS]
    umem = np.empty_like(rs[0].umem)
    with HostPath(checksummer("zero"), umem, path="staged", max_batch=n) as hp:
        for r, rd in enumerate(rs):
            umem[:] = rd.umem
            v = np.full(n, 7, dtype=np.int32)
            before = hp.stats()
            if r == 0:
                hp.process_batch(rd.descs, ingress_ifindex=SC.INGRESS, verdicts=v)
            else:
                hp.wait(hp.submit(rd.descs, v, ingress_ifindex=SC.INGRESS))
            moved(before, hp.stats(), rd.descs, umem.size, n, f"piece-cut round {r}")
            same(v, umem, rd.want_verdicts, rd.want_umem, f"piece-cut round {r}")


def test_empty_batch_changes_nothing(dev):
    """n = 0 on a used context: the call returns, and no counter and no byte moves."""
    rd = SC.rounds("one-run", 1, SEED)[0]
    umem = rd.umem.copy()
    none = np.zeros(0, dtype=frames.DESC_DTYPE)
    with HostPath(checksummer("zero"), umem, path="staged", max_batch=4200) as hp:
        v = hp.process_batch(rd.descs, ingress_ifindex=SC.INGRESS)
        same(v, umem, rd.want_verdicts, rd.want_umem, "one-run")
        before = hp.stats()
        assert hp.process_batch(none, ingress_ifindex=SC.INGRESS).shape[0] == 0
        out = np.full(4, 7, dtype=np.int32)
        hp.wait(hp.submit(none, out, ingress_ifindex=SC.INGRESS))
        assert hp.stats() == before
        assert (out == 7).all() and np.array_equal(umem, rd.want_umem)
