"""tests/option_cases.py on the CPU: the option cycle meets its requirements, and
on the very batches tests/test_gpu_batch_options.py launches, every batch
distinguishes its own options from every other member of the cycle -- in a
verdict, and in a UMEM byte where the payload multiples differ.  Without that a
kernel or host path that processed a batch with another batch's values could
still equal the oracle."""
import numpy as np
import pytest

from oracle import csum_oracle as O
from tests import option_cases as OC
from xsknf_amd import frames


def test_cycle_meets_its_requirements():
    OC.cycle_holds()
    c = OC.OPTION_CYCLE
    assert len(c) >= 6
    # neighbours differ, also across the wrap, and at every offset a context or thread starts from
    for off in range(len(c)):
        f = [OC.fwd(o) for o in OC.cycled(2 * len(c), off)]
        assert all(a != b for a, b in zip(f[:-1], f[1:]))
    assert sorted(OC.fwd(o) for o in c) == [-1, 0, 1, 2, 3, 4]
    assert sorted(OC.mult(o) for o in c) == [0, 1, 1, 2, 3, 7919]
    assert set(OC.CHEAP_CYCLE) < set(c) and len(set(OC.fwd(o) for o in OC.CHEAP_CYCLE)) >= OC.STREAM_LAUNCHES + 1
    o = OC.csum_opts(c[4])
    assert (o.csum_iterations, o.action, o.num_interfaces) == (-3, O.REDIRECT, 3) and OC.kw(c[4])["ingress"] == 1


@pytest.mark.parametrize("bad", [
    OC.OPTION_CYCLE[:3] + ((0, 4, 1, O.REDIRECT),) + OC.OPTION_CYCLE[3:],     # verdict 1 twice
    tuple(o for o in OC.OPTION_CYCLE if o[3] != O.DROP),                       # one action only
    tuple(o for o in OC.OPTION_CYCLE if o[2] >= 0),                            # no zero-pass count
], ids=["shared-verdict", "one-action", "no-negative-count"])
def test_a_weaker_cycle_fails(bad):
    with pytest.raises(AssertionError):
        OC.cycle_holds(bad)


def test_the_condition_is_not_vacuous():
    """Batches that could hide a leak fail it: one whose first frames never reach
    the check (their verdict does not depend on the options), one whose UDP
    bytes sum to zero (nothing for the payload multiple to multiply), and a
    plan that gives a batch options outside the cycle."""
    cuts = [0, 40, 80]
    b = OC.traffic(80, cuts, seed=7)
    OC.Case(b, cuts, OC.cycled(2)).leak_is_visible()
    arp = b.copy()
    for i in range(OC.PROBE):
        o = int(arp.frame_offsets()[40 + i])
        arp.umem[o + 12:o + 14] = [0x08, 0x06]
    with pytest.raises(AssertionError, match="batch 1: verdicts"):
        OC.Case(arp, cuts, OC.cycled(2)).leak_is_visible()
    flat = b.copy()
    for i in range(OC.PROBE):      # an all-zero UDP header and payload: a sum of zero, whatever multiplies it
        o = int(flat.frame_offsets()[i])
        flat.umem[o + 34:o + int(flat.descs["len"][i])] = 0
    with pytest.raises(AssertionError, match="batch 0: UMEM"):
        OC.Case(flat, cuts, OC.cycled(2)).leak_is_visible()
    with pytest.raises(AssertionError):
        OC.leak_is_visible(b.umem, [(b.descs[:40], (0, 7, 1, O.REDIRECT))])


def test_traffic_keeps_what_the_condition_needs():
    cuts = OC.cuts_of(600, [1, 2, 7, 8, 9, 100, 300])
    assert cuts == [0, 1, 3, 10, 18, 27, 127, 427, 600]
    plain = frames.unaligned_batch(600, "imix", seed=11)
    b = OC.traffic(600, cuts, seed=11, edge=0.2, ihl=0.1)
    changed = np.array([not np.array_equal(plain.frame(i), b.frame(i)) for i in range(600)])
    assert changed[10:].sum() > 100 and not changed[:10].any()          # batches under 8 frames stay whole
    assert not changed[cuts[:-1]].any()                                 # every batch's first frame
    assert all(OC.well_formed(b, lo) for lo in cuts[:-1])
    ihl = np.array([b.frame(i)[14] & 15 for i in range(600) if b.descs["len"][i] >= 34])
    assert (ihl == 2).sum() > 5 and (ihl == 3).sum() > 5
    # ihl 2 / 3: a second pass changes the frame again (a batch processed twice shows)
    once = b.copy()
    O.c_process_batch(once.umem, once.descs, **OC.kw(OC.OPTION_CYCLE[0]))
    twice = once.copy()
    O.c_process_batch(twice.umem, twice.descs, **OC.kw(OC.OPTION_CYCLE[0]))
    assert not np.array_equal(once.umem, twice.umem)


@pytest.mark.parametrize("checks", ["zero", "nic"])
def test_one_context_batches(checks):
    """The cuts reach every mechanism: the named sizes, a batch of several ring
    entries, more batches than slots and than ring entries (so both are reused
    by a batch with other options), and every member of the cycle lands on each
    slot and each ring entry."""
    k = OC.constants()
    c = OC.one_context(checks)
    sizes = [hi - lo for lo, hi, _ in c.batches()]
    assert sizes[:6] == list(OC.ONE_CONTEXT_FIXED) and sum(sizes) == OC.ONE_CONTEXT_FRAMES == c.b.n
    assert max(sizes) == OC.ONE_CONTEXT_MAX_BATCH and OC.entries(700, k["entry_frames"]) == 3
    assert 1 <= min(sizes[6:]) and max(sizes[6:-1]) <= 300 and len(set(sizes)) > 20
    assert {1, k["block_frames"], k["block_frames"] + 1, k["entry_frames"], k["entry_frames"] + 1} <= set(sizes)
    assert len(sizes) > 4 * k["entries"] > 4 * k["slots"]
    assert [o for _, _, o in c.batches()] == OC.cycled(len(sizes))
    slot_opts = {(j % k["slots"], o) for j, (_, _, o) in enumerate(c.batches())}
    assert len(slot_opts) == k["slots"] * len(OC.OPTION_CYCLE)
    e, entry_opts = 0, set()
    for lo, hi, o in c.batches():
        for _ in range(OC.entries(hi - lo, k["entry_frames"])):
            entry_opts.add((e % k["entries"], o))
            e += 1
    assert len(entry_opts) >= 3 * k["entries"]          # every entry holds at least three different headers
    assert c.leak_is_visible() == len(sizes) * (len(OC.OPTION_CYCLE) - 1)
    if checks == "nic":
        # the write elision next to batches that rewrite everything: under -i 1 an
        # offloaded check is found in place (all but the few whose fold loses a
        # carry, and the mutated frames), under any other count it changes
        u, _ = c.want()
        offs, lens = c.b.frame_offsets(), c.b.descs["len"]
        moved = np.array([not np.array_equal(u[int(o):int(o + n)], c.b.umem[int(o):int(o + n)])
                          for o, n in zip(offs, lens)])
        one = np.concatenate([np.full(hi - lo, o[2] == 1) for lo, hi, o in c.batches()])
        print("frames changed: -i 1", moved[one].mean(), "other counts", moved[~one].mean())
        assert one.sum() > 1000 and moved[one].mean() < 0.1 and moved[~one].mean() > 0.8


@pytest.mark.parametrize("n_ctx,max_batch,batch", OC.SHARED_SHAPES, ids=[f"{s[0]}x{s[2]}" for s in OC.SHARED_SHAPES])
def test_shared_kernel_batches(n_ctx, max_batch, batch):
    cases = OC.shared_kernel(n_ctx, max_batch, batch)
    assert len(cases) == n_ctx and all(hi - lo <= max_batch for c in cases for lo, hi, _ in c.batches())
    # at every step neighbouring rings hold different options, and so do a ring's consecutive entries
    for a, b in zip(cases[:-1], cases[1:]):
        assert all(OC.fwd(x) != OC.fwd(y) for x, y in zip(a.opts, b.opts))
    assert OC.all_leaks_visible(cases) == sum(len(c.opts) for c in cases) * (len(OC.OPTION_CYCLE) - 1)


def test_join_leave_batches():
    cases = OC.join_leave()
    steps = OC.join_leave_steps()
    assert [s for s in steps if s[0] != "feed"] == [("open", 0, 256), ("open", 1, 64), ("open", 2, 256), ("leave", 1),
                                                    ("open", 3, 1500)]
    assert [c.n for c in cases] == [1500, 7 * 64, 1500, 1500]
    assert all(c.b.n == OC.JOIN_LEAVE_FRAMES for c in cases)
    assert sum(s[2] for s in steps if s[0] == "feed") == sum(c.n for c in cases)
    assert OC.all_leaks_visible(cases) > 0


def test_worker_thread_batches():
    cases = OC.worker_threads()
    assert len(cases) == len(OC.WORKER_PATHS) == 6
    assert all(c.opts[:6] == OC.cycled(6, k) for k, c in enumerate(cases))
    assert OC.all_leaks_visible(cases) == sum(len(c.opts) for c in cases) * (len(OC.OPTION_CYCLE) - 1)


def test_stream_batches():
    jobs = OC.streams()
    assert len(jobs) == OC.STREAMS and all(j.b.n == OC.STREAM_FRAMES for j in jobs)
    for j in jobs:
        f = [OC.fwd(o) for o in j.opts]
        assert len(j.opts) == OC.STREAM_LAUNCHES and len(set(f)) == len(f)
    assert any(o[2] == 7919 for j in jobs for o in j.opts) and any(o[2] < 0 for j in jobs for o in j.opts)
    assert OC.all_leaks_visible(jobs) == OC.STREAMS * OC.STREAM_LAUNCHES * (len(OC.OPTION_CYCLE) - 1)
