"""Per-batch options under concurrency: the inputs and the oracle of
tests/test_gpu_batch_options.py, and the condition that makes a leak visible
(tests/test_option_cases.py checks it on the CPU; every GPU test asserts it
again on the very inputs it launches).

`ingress_ifindex` and struct xsknf_csum_opts are arguments of a BATCH.  Two
values are derived from them -- the forward verdict and the payload multiple
max(iterations, 0) -- and each host path carries them its own way: launch
arguments (ZEROCOPY), the slot (STAGED, applied on the host after the event),
the ring entry's header (RESIDENT, read by the one kernel every ring shares).
A test whose batches all ask for the same thing cannot tell whose values a
batch was processed with, so here consecutive batches step through
OPTION_CYCLE, whose members all differ in the forward verdict.

The oracle is oracle.csum_oracle.c_process_batch applied to each batch with its
own options, in submission order, on one UMEM copy.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import csum_oracle as O
from xsknf_amd import _lib, frames

# (ingress, num_interfaces, iterations, action)
OPTION_CYCLE = (
    (0, 2, 1, O.REDIRECT),
    (1, 2, 3, O.REDIRECT),
    (2, 4, 2, O.REDIRECT),
    (0, 1, 1, O.DROP),
    (1, 3, -3, O.REDIRECT),     # a negative count: zero passes over the payload
    (3, 5, 7919, O.REDIRECT),
)
REQUIRED_ITERATIONS = (1, 2, 3, -3, 7919)
# The literal per-word oracle needs ~3 ms per 1500 B frame at 7919 iterations:
# the 4,096-frame device batches of 1500 B and IMIX frames step through the
# members below it, the 64 B ones (11 words a frame) through the whole cycle.
CHEAP_CYCLE = tuple(o for o in OPTION_CYCLE if o[2] < 1000)
PROBE = 8     # frames of a batch the alternatives are evaluated on (leak_is_visible)


def fwd(opt):
    """The forward verdict (checksummer_user.c:110-111)."""
    ingress, nif, _, action = opt
    return (ingress + 1) % nif if action == O.REDIRECT else -1


def mult(opt):
    """How often the payload counts in the sum (checksummer_user.c:92-103)."""
    return max(opt[2], 0)


def kw(opt):
    ingress, nif, iters, action = opt
    return dict(ingress=ingress, nif=nif, iters=iters, action=action)


def csum_opts(opt):
    return _lib.CsumOpts(opt[2], opt[3], opt[1], 0)


def cycle_holds(cycle=OPTION_CYCLE):
    f = [fwd(o) for o in cycle]
    assert len(set(f)) == len(f), f"two members share a forward verdict: {f}"
    assert {o[3] for o in cycle} == {O.REDIRECT, O.DROP}
    assert set(REQUIRED_ITERATIONS) <= {o[2] for o in cycle}
    assert all(o[0] < o[1] for o in cycle)          # an ingress the worker has


def cuts_of(n, sizes):
    """Cut points of n frames into consecutive batches of the given sizes; the
    last batch takes what is left (sizes past n are not used)."""
    cuts = [0]
    for k in sizes:
        if cuts[-1] + int(k) >= n:
            break
        cuts.append(cuts[-1] + int(k))
    cuts.append(n)
    return cuts


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def pool_map(fn, items):
    """The C oracle releases the GIL: independent contexts on up to 16 CPUs."""
    items = list(items)
    with ThreadPoolExecutor(max_workers=_threads()) as ex:
        return list(ex.map(fn, items))


# ---- the oracle and the condition ------------------------------------------------

def expected(umem, plan):
    """plan: [(descs, opt)] in submission order.  Returns (the UMEM afterwards,
    [each batch's verdicts])."""
    u = umem.copy()
    return u, [O.c_process_batch(u, d, **kw(opt)) for d, opt in plan]


def _span(descs):
    a = descs["addr"]
    off = (a & np.uint64((1 << frames.OFFSET_SHIFT) - 1)) + (a >> np.uint64(frames.OFFSET_SHIFT))
    return int(off.min()), int((off + descs["len"]).max())


def leak_is_visible(umem, plan, cycle=OPTION_CYCLE, probe=PROBE):
    """Asserted on the oracle alone: for every batch of the plan and every other
    member o of the cycle, the batch processed under o differs from the batch
    processed under its own options in at least one verdict, and, where the two
    payload multiples differ, in at least one UMEM byte -- each from the UMEM
    state the batches before it leave.  A batch's frames never overlap (packed
    or chunked layouts) and a frame's result depends on its own bytes only, so
    a witness among the batch's first `probe` frames is a witness in the batch:
    the alternatives run on those (the 7919-iteration member costs the literal
    oracle milliseconds per frame).  Returns the number of comparisons made."""
    cur = umem.copy()
    done = 0
    for j, (descs, opt) in enumerate(plan):
        assert opt in cycle and descs.shape[0] > 0
        d = descs[:probe]
        lo, hi = _span(d)
        pre = cur[lo:hi].copy()
        v_own = O.c_process_batch(cur, d, **kw(opt))
        own = cur[lo:hi].copy()
        for o in cycle:
            if o == opt:
                continue
            cur[lo:hi] = pre
            v = O.c_process_batch(cur, d, **kw(o))
            assert (v != v_own).any(), f"batch {j}: verdicts under {o} equal those under its own {opt}"
            if mult(o) != mult(opt):
                assert (cur[lo:hi] != own).any(), f"batch {j}: UMEM under {o} equals that under its own {opt}"
            done += 1
        cur[lo:hi] = pre
        O.c_process_batch(cur, descs, **kw(opt))
    return done


# ---- traffic ---------------------------------------------------------------------

def well_formed(b, i):
    """Frame i is Ethernet / IPv4 (ihl 5) / UDP with a payload: it reaches
    checksummer_user.c:108, so its verdict is the forward verdict and its
    check depends on the payload multiple."""
    f = b.frame(i)
    return (f.shape[0] > frames.HDR_LEN and f[12] == 0x08 and f[13] == 0x00 and f[14] == 0x45 and f[23] == 17)


def traffic(n, cuts, *, seed, layout="unaligned", length="imix", checks="zero", edge=0.05, ihl=0.04):
    """n frames cut at `cuts`: frames.inject_edge_cases over a share `edge`, and
    ihl 2 / 3 over a share `ihl` (their check lands in the addresses the
    pseudo-header sums: processing one twice, or under another batch's
    multiple and then its own, shows), of the frames that may change: every
    batch's first frame stays a well-formed UDP frame with a payload, and
    batches under 8 frames stay whole."""
    b = (frames.unaligned_batch(n, length, seed=seed) if layout == "unaligned"
         else frames.aligned_batch(n, length, chunk=2048, seed=seed))
    if checks == "nic":
        frames.offload_checks_host(b)
    free = np.zeros(n, dtype=bool)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi - lo >= 8:
            free[lo + 1:hi] = True
    idx = np.flatnonzero(free)
    sub = frames.HostBatch(b.umem, b.descs[idx].copy(), b.layout)      # (the UMEM is shared, the lengths copied)
    frames.inject_edge_cases(sub, edge, seed=seed + 1)
    b.descs["len"][idx] = sub.descs["len"]
    rng = np.random.default_rng(seed + 2)
    offs = b.frame_offsets()
    for i in rng.choice(idx, size=int(round(idx.size * ihl)), replace=False):
        if b.descs["len"][i] >= 34:
            o = int(offs[i])
            b.umem[o + 14] = (b.umem[o + 14] & 0xF0) | (2 + int(rng.integers(0, 2)))
    for lo in cuts[:-1]:
        assert well_formed(b, lo), lo
    return b


class Case:
    """One context's traffic: the batch, its cut points and each batch's options."""

    def __init__(self, b, cuts, opts):
        assert len(opts) == len(cuts) - 1 and cuts[0] == 0 and all(a < c for a, c in zip(cuts[:-1], cuts[1:]))
        self.b, self.cuts, self.opts = b, list(cuts), list(opts)
        self.n = cuts[-1]           # frames submitted (a context that leaves early submits fewer than b.n)
        b.umem.setflags(write=False)
        self._want = None

    def batches(self):
        return [(lo, hi, o) for lo, hi, o in zip(self.cuts[:-1], self.cuts[1:], self.opts)]

    def plan(self):
        return [(self.b.descs[lo:hi], o) for lo, hi, o in self.batches()]

    def leak_is_visible(self):
        return leak_is_visible(self.b.umem, self.plan())

    def want(self):
        """(the oracle's UMEM, its verdicts for the n frames), computed once."""
        if self._want is None:
            u, v = expected(self.b.umem, self.plan())
            u.setflags(write=False)
            self._want = (u, np.concatenate(v))
        return self._want


def cycled(n_batches, offset=0, cycle=OPTION_CYCLE):
    return [cycle[(offset + k) % len(cycle)] for k in range(n_batches)]


def make_case(n, cuts, *, seed, offset=0, **kw_traffic):
    return Case(traffic(n, cuts, seed=seed, **kw_traffic), cuts, cycled(len(cuts) - 1, offset))


def want_all(cases):
    return pool_map(lambda c: c.want(), cases)


def all_leaks_visible(cases):
    return sum(pool_map(lambda c: c.leak_is_visible(), cases))


# ---- the cases of tests/test_gpu_batch_options.py --------------------------------

def constants():
    """What decides the sizes, from the code: a launched context's slots, the
    ring's entries, an entry's frames, the frames one block of its group takes
    and the blocks of a group."""
    from tests.route_cases import code_constant
    h = "checksummer_internal.h"
    return dict(slots=code_constant("host_path.hip", r"constexpr int kSlots = (\d+);"),
                entries=code_constant(h, r"#define XSKNF_RES_SLOTS (\d+)"),
                entry_frames=code_constant(h, r"#define XSKNF_RES_FRAMES (\d+)"),
                block_frames=code_constant(h, r"constexpr uint32_t kResBlockFrames = (\d+);"),
                group=code_constant(h, r"#define XSKNF_RES_GROUP (\d+)"))


def entries(n, entry_frames=256):
    """Ring entries a batch of n frames takes (host_path.hip submit())."""
    return -(-n // entry_frames)


ONE_CONTEXT_FRAMES = 6000
ONE_CONTEXT_FIXED = (1, 64, 65, 256, 257, 700)
ONE_CONTEXT_MAX_BATCH = 700


@functools.lru_cache(maxsize=None)
def one_context(checks):
    """~6,000 unaligned IMIX frames in batches of 1, 64, 65, 256, 257, 700 and
    random sizes 1..300, batch k under OPTION_CYCLE[k % len]."""
    rng = np.random.default_rng(0x0C7)
    cuts = cuts_of(ONE_CONTEXT_FRAMES, list(ONE_CONTEXT_FIXED) + [int(k) for k in rng.integers(1, 301, size=200)])
    return make_case(ONE_CONTEXT_FRAMES, cuts, seed=0x0C70 + (checks == "nic"), checks=checks)


SHARED_SHAPES = [(8, 2000, 100), (8, 64, 50), (40, 300, 257)]     # test_resident_contexts_share_one_kernel's


def shared_kernel(n_ctx, max_batch, batch):
    """Context c steps the cycle from offset c: at any moment neighbouring
    rings, and neighbouring entries of one ring, hold different headers."""
    total = 1200 if n_ctx > 8 else 2000
    cuts = list(range(0, total, batch)) + [total]
    return pool_map(lambda c: make_case(total, cuts, seed=0x5A00 + 16 * c, offset=c, layout="aligned"),
                    range(n_ctx))


# what test_resident_rings_join_and_leave_under_traffic does, as a schedule:
# ("open", ctx, max_batch) / ("feed", ctx, frames) / ("leave", ctx: wait, close) / ("drain", ctxs, frames)
JOIN_LEAVE_FRAMES = 1500
JOIN_LEAVE = ([("open", 0, 256), ("open", 1, 64)] + [("feed", 0, 200), ("feed", 1, 64)] * 4 +
              [("open", 2, 256)] + [("feed", 0, 200), ("feed", 1, 64), ("feed", 2, 256)] * 3 +
              [("leave", 1), ("open", 3, 1500), ("drain", (0, 2, 3), 150)])


def join_leave_steps():
    """JOIN_LEAVE with the drain unrolled: feeds of at most the frames left."""
    pos = {}
    steps = []
    for s in JOIN_LEAVE:
        if s[0] == "open":
            pos[s[1]] = 0
            steps.append(s)
        elif s[0] == "feed":
            k = min(s[2], JOIN_LEAVE_FRAMES - pos[s[1]])
            if k:
                steps.append(("feed", s[1], k))
                pos[s[1]] += k
        elif s[0] == "leave":
            steps.append(s)
        else:
            while any(pos[c] < JOIN_LEAVE_FRAMES for c in s[1]):
                for c in s[1]:
                    k = min(s[2], JOIN_LEAVE_FRAMES - pos[c])
                    if k:
                        steps.append(("feed", c, k))
                        pos[c] += k
    return steps


def join_leave():
    """Four contexts; context c steps the cycle from offset c.  Context 1 leaves
    after its feeds: the rest of its frames is never submitted (Case.n)."""
    sizes = {c: [] for c in range(4)}
    for s in join_leave_steps():
        if s[0] == "feed":
            sizes[s[1]].append(s[2])
    cases = []
    for c in range(4):
        cuts = [0] + [int(x) for x in np.cumsum(sizes[c])]
        # (traffic for all 1500 frames, as the neighbouring test builds it; the cuts end where the feeds end)
        tcuts = cuts if cuts[-1] == JOIN_LEAVE_FRAMES else cuts + [JOIN_LEAVE_FRAMES]
        b = traffic(JOIN_LEAVE_FRAMES, tcuts, seed=0x7100 + 16 * c, edge=0.1)
        cases.append(Case(b, cuts, cycled(len(cuts) - 1, c)))
    return cases


WORKER_PATHS = ["resident", "zerocopy", "staged"] * 2
WORKER_FRAMES, WORKER_BATCH, WORKER_OUT = 3000, 64, 4


def worker_threads():
    cuts = list(range(0, WORKER_FRAMES, WORKER_BATCH)) + [WORKER_FRAMES]
    return pool_map(lambda k: make_case(WORKER_FRAMES, cuts, seed=0x3D00 + 16 * k, offset=k),
                    range(len(WORKER_PATHS)))


STREAMS, STREAM_LAUNCHES, STREAM_FRAMES = 24, 4, 4096
STREAM_LENGTHS = (1500, "imix", 64)


class StreamJob:
    """A device-resident batch launched STREAM_LAUNCHES times on its stream,
    each launch under its own options: the oracle applied as often, in order."""

    def __init__(self, i):
        self.length = STREAM_LENGTHS[i % 3]
        members = OPTION_CYCLE if self.length == 64 else CHEAP_CYCLE
        self.opts = cycled(STREAM_LAUNCHES, i, members)
        self.b = traffic(STREAM_FRAMES, [0, STREAM_FRAMES], seed=0x57A0 + 16 * i, layout="aligned",
                         length=self.length)
        self.b.umem.setflags(write=False)
        self._want = None

    def plan(self):
        return [(self.b.descs, o) for o in self.opts]

    def leak_is_visible(self):
        return leak_is_visible(self.b.umem, self.plan())

    def want(self):
        """(the UMEM after the last launch, each launch's verdicts)."""
        if self._want is None:
            self._want = expected(self.b.umem, self.plan())
        return self._want


def streams():
    return pool_map(StreamJob, range(STREAMS))
