"""The STAGED copy plan's cases (tests/staged_cases.py) on the CPU: every
generator lands in the branch it is meant for under the model, the edge pairs
differ in one quantity only, no batch holds overlapping frames, the model's
constants and comparisons are the source's, and every round's expectation
differs from the round before in every summed frame's check.  Nothing here
needs a GPU: tests/test_gpu_staged_plan.py runs the same cases through
stage_frames() and holds its byte counters to this model.
"""
import numpy as np
import pytest

from tests import staged_cases as SC

SEED = 0x57A6
ROUNDS = 3


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_lands_in_its_branch(name):
    umem, descs, branch = SC.case(name)
    assert umem.size <= SC.UMEM_MAX
    assert descs.shape[0] <= (4200 if name != "piece-cut" else SC.constants()["piece"] + 1)
    assert SC.no_overlap(descs, umem.size)
    _, _, branches = SC.counters(descs, umem.size, SC.max_batch(name))
    assert branches == [branch] * len(branches), name
    v = SC.valid(descs, umem.size)
    ln = descs["len"][v]
    assert ln.size == 0 or (ln.min() >= SC.MIN_LEN and ln.max() <= max(SC.MAX_LEN, 1536))


def test_2d_past_end_takes_no_2d_copy():
    """Asserted before any GPU run uses the case: a 2-D copy of these frames
    would read past the registered UMEM."""
    umem, descs, branch = SC.case("2d-past-end")
    d = SC.plan_detail(descs, umem.size)
    off = np.sort(SC.offsets(descs))
    assert branch == d["branch"] == SC.MAPPED_SCATTERED
    assert d["width"] == SC.MAX_LEN and d["stride"] == SC.TWO_D_STRIDE and len(d["runs"]) > SC.constants()["max_runs"]
    assert int(off[-1]) + SC.MIN_LEN == umem.size                        # the last frame ends on the last byte
    assert int(off[0]) + (d["k"] - 1) * d["stride"] + d["width"] > umem.size
    assert SC.valid(descs, umem.size).all()


def test_constants_and_comparisons_are_the_sources():
    K = SC.constants()
    assert {k: K[k] for k in SC.TABLE} == SC.TABLE
    assert K["slots"] > SC.INTERLEAVED_BATCHES           # four batches in flight, none completed by a submit
    assert SC.comparisons_hold() == len(SC.COMPARISONS) + 1


def test_a_pattern_the_source_lost_fails():
    with pytest.raises(AssertionError, match="no longer matches"):
        SC.code_constant(SC.SRC, r"constexpr uint64_t kMergeGap = (\d+)u;")


def _same_frames(a, b, n):
    return np.array_equal(a["addr"][:n], b["addr"][:n]) and np.array_equal(a["len"][:n], b["len"][:n])


def test_gap_pair_differs_in_the_ninth_group():
    K = SC.constants()
    (ua, da, _), (ub, db, _) = SC.case("gap-at"), SC.case("gap-over")
    assert ua.size == ub.size and da.shape[0] == 40 and db.shape[0] == 45 and _same_frames(da, db, 40)
    a, b = SC.plan_detail(da, ua.size), SC.plan_detail(db, ub.size)
    assert len(a["runs"]) == K["max_runs"] and len(b["runs"]) == K["max_runs"] + 1
    assert (a["branch"], b["branch"]) == (SC.RUNS, SC.MAPPED_SCATTERED)
    # the steps between the frames: kMergeGap inside a group, kMergeGap + 1 between groups
    off, ln = SC.offsets(db), db["len"].astype(np.int64)
    step = off[1:] - (off[:-1] + ln[:-1])
    assert set(step[np.arange(1, 45) % 5 != 0]) == {K["merge_gap"]}
    assert set(step[np.arange(1, 45) % 5 == 0]) == {K["merge_gap"] + 1}
    # runs move their gap bytes too: 4 gaps a group
    assert a["moved"] == int(da["len"].sum()) + 8 * 4 * K["merge_gap"]
    assert b["moved"] == int(db["len"].sum())
    assert np.unique(np.diff(off)).size > 1                                  # no constant stride


def test_sortmax_pair_differs_in_one_frame():
    K = SC.constants()
    (ua, da, _), (ub, db, _) = SC.case("reversed-sortmax"), SC.case("reversed-sortmax+1")
    assert ua.size == ub.size and da.shape[0] == K["sort_max"] and db.shape[0] == K["sort_max"] + 1
    assert _same_frames(da, db[1:], K["sort_max"])                           # the extra frame is the highest slot
    for d in (da, db):
        assert (np.diff(SC.offsets(d)) == -2048).all()
    a, b = SC.plan_detail(da, ua.size), SC.plan_detail(db, ub.size)
    assert not a["sorted"] and not b["sorted"]
    assert (a["branch"], b["branch"]) == (SC.TWO_D, SC.MAPPED_UNSORTED)
    assert a["moved"] == int(da["len"].max()) * K["sort_max"] and b["moved"] == int(db["len"].sum())
    assert a["moved"] != int(da["len"].sum())


def test_2d_end_pair_differs_in_the_umem_size():
    (ua, da, _), (ub, db, _) = SC.case("2d-fits-exactly"), SC.case("2d-past-end")
    assert _same_frames(da, db, da.shape[0]) and da.shape[0] == db.shape[0] == SC.TWO_D_FRAMES
    a, b = SC.plan_detail(da, ua.size), SC.plan_detail(db, ub.size)
    assert ua.size == int(SC.offsets(da)[0]) + (a["k"] - 1) * a["stride"] + a["width"]
    assert ua.size - ub.size == SC.MAX_LEN - SC.MIN_LEN
    assert (a["branch"], b["branch"]) == (SC.TWO_D, SC.MAPPED_SCATTERED)
    assert a["moved"] == SC.MAX_LEN * SC.TWO_D_FRAMES and b["moved"] == int(db["len"].sum()) != a["moved"]
    # one byte less than exactly: no 2-D copy either
    assert SC.plan(da, ua.size - 1)[0] == SC.MAPPED_SCATTERED


def test_2d_stride_pair_differs_in_one_byte_of_one_address():
    (ua, da, _), (ub, db, _) = SC.case("2d"), SC.case("2d-off-stride")
    assert ua.size == ub.size and np.array_equal(da["len"], db["len"])
    diff = np.flatnonzero(da["addr"] != db["addr"])
    assert diff.tolist() == [300] and int(db["addr"][300]) - int(da["addr"][300]) == 1
    a, b = SC.plan(da, ua.size), SC.plan(db, ub.size)
    assert a == (SC.TWO_D, int(da["len"].max()) * SC.TWO_D_FRAMES)
    assert b == (SC.MAPPED_SCATTERED, int(db["len"].sum()))
    # rx order, one headroom, mixed lengths
    assert SC.plan_detail(da, ua.size)["sorted"] and np.unique(da["len"]).size > 100
    assert (SC.offsets(da) % SC.TWO_D_STRIDE == 256).all()


def test_width_may_equal_the_stride():
    umem, descs, _ = SC.case("2d-width-is-stride")
    d = SC.plan_detail(descs, umem.size)
    assert d["branch"] == SC.TWO_D and d["width"] == d["stride"] == 1536 == int(descs["len"].max())
    assert (descs["len"] == 1536).sum() == 1 and d["moved"] == 1536 * 64
    assert umem.size == int(SC.offsets(descs)[0]) + 63 * 1536 + 1536


def test_runs_cases_are_the_runs_they_name():
    K = SC.constants()
    for name, n in (("one-run", 300), ("shuffled-packed", 300), ("run-extends", 12)):
        umem, descs, _ = SC.case(name)
        d = SC.plan_detail(descs, umem.size)
        off, ln = SC.offsets(descs), descs["len"].astype(np.int64)
        assert d["k"] == n and len(d["runs"]) == 1, name
        assert d["moved"] == int((off + ln).max() - off.min())
        assert d["sorted"] == (name == "one-run")
    _, descs, _ = SC.case("one-run")
    assert (descs["addr"] >> np.uint64(48)).max() > 0 and (SC.offsets(descs) % 2).min() == 0 < (SC.offsets(
        descs) % 2).max()
    # run-extends: sorted, the steps hold 0, kMergeGap and values between
    umem, descs, _ = SC.case("run-extends")
    at = np.argsort(SC.offsets(descs))
    off, ln = SC.offsets(descs)[at], descs["len"].astype(np.int64)[at]
    step = off[1:] - (off[:-1] + ln[:-1])
    assert step.min() == 0 and step.max() == K["merge_gap"] and (ln[0], ln[1]) == (1500, 60)
    # shuffled-small: the whole 16 MiB, out of order, no stride
    umem, descs, _ = SC.case("shuffled-small")
    d = SC.plan_detail(descs, umem.size)
    assert umem.size == 16 << 20 and d["k"] == 64 and not d["sorted"] and len(d["runs"]) > K["max_runs"]
    assert int(SC.offsets(descs).max()) - int(SC.offsets(descs).min()) > 8 << 20


def test_invalid_descriptors_do_not_count():
    K = SC.constants()
    (ug, dg, _), (ui, di, _) = SC.case("gap-at"), SC.case("invalid-between")
    v = SC.valid(di, ui.size)
    assert ug.size == ui.size and _same_frames(dg, di[v], 40) and int((~v).sum()) == 13
    assert SC.plan(di, ui.size) == SC.plan(dg, ug.size)
    # each kind is there, and each invalid one would break the address order if it counted
    off = SC.offsets(di)
    kinds = {(int(di["len"][i]) == 0, int(di["len"][i]) == 0xFFFFFFFF, int(di["addr"][i]) == 1 << 47,
              int(di["addr"][i]) >> 48 == 0xFFFF) for i in np.flatnonzero(~v)}
    assert len(kinds) == SC.INVALID_KINDS
    for i in np.flatnonzero(~v):
        assert v[i - 1] and v[i + 1] and not off[i - 1] <= off[i] <= off[i + 1]
    past = [i for i in np.flatnonzero(~v) if int(di["len"][i]) == 100 and int(di["addr"][i]) < 1 << 47]
    assert past and all(int(off[i]) + 100 == ui.size + 1 for i in past)       # past the end by one byte
    # all-invalid: no run, nothing moves
    ua, da, _ = SC.case("all-invalid")
    d = SC.plan_detail(da, ua.size)
    assert d["k"] == 0 and d["runs"] == [] and (d["branch"], d["moved"]) == (SC.RUNS, 0)
    assert SC.counters(da, ua.size, 4200)[:2] == (16 * 50, 4 * 50)
    wu, wv = SC.expected(ua, da)
    assert (wv == -1).all() and np.array_equal(wu, ua)


def test_piece_cut_is_two_pieces():
    K = SC.constants()
    umem, descs, _ = SC.case("piece-cut")
    n = K["piece"] + 1
    assert SC.pieces(n, n) == [(0, K["piece"]), (K["piece"], n)]
    assert SC.counters(descs, umem.size, n) == (16 * n + 64 * n, 4 * n, [SC.RUNS, SC.RUNS])
    assert SC.pieces(n, 4096)[:2] == [(0, 4096), (4096, 8192)] and SC.pieces(0, n) == []


def test_interleaved_batches_are_one_run_each():
    umem, descs, _ = SC.case("interleaved-packed")
    off, ln = SC.offsets(descs), descs["len"].astype(np.int64)
    for j in range(SC.INTERLEAVED_BATCHES):
        sub = descs[j::SC.INTERLEAVED_BATCHES]
        d = SC.plan_detail(sub, umem.size)
        assert d["branch"] == SC.RUNS and len(d["runs"]) == 1 and d["k"] == 300
        lo, hi = d["runs"][0][0], d["runs"][0][0] + d["runs"][0][1]
        others = np.ones(descs.shape[0], bool)
        others[j::SC.INTERLEAVED_BATCHES] = False
        inside = others & (off >= lo) & (off + ln <= hi)
        assert inside.sum() >= 3 * 299                  # the run covers the other batches' frames between its own


def _rounds_hold(name, checks):
    rs = SC.rounds(name, ROUNDS, SEED, checks)
    _, descs0, branch = SC.case(name)
    summed = 0
    for r, rd in enumerate(rs):
        assert np.array_equal(rd.descs["addr"], descs0["addr"]) and (rd.descs["len"] <= descs0["len"]).all()
        assert SC.no_overlap(rd.descs, rd.umem.size)
        assert SC.counters(rd.descs, rd.umem.size, SC.max_batch(name))[2][0] == branch, (name, r)
        at = rd.check_at[rd.check_at >= 0]
        summed += at.size
        # the summed frames are those the oracle gives the forward verdict, and it wrote their checks
        assert np.array_equal(rd.check_at >= 0, rd.want_verdicts == SC.FWD)
        changed = np.flatnonzero(rd.want_umem != rd.umem)
        assert np.isin(changed, np.concatenate([at, at + 1])).all()
        if r:
            assert rd.same_checks_as(rs[r - 1]).size == 0, (name, r)
            assert not np.array_equal(rd.umem, rs[r - 1].umem)
    return summed, rs


# (test_piece_cut runs with zero checks only)
@pytest.mark.parametrize("name,checks", [(n, c) for n in SC.CASES for c in ("zero", "nic")
                                         if (n, c) != ("piece-cut", "nic")])
def test_every_round_changes_every_summed_check(name, checks):
    summed, rs = _rounds_hold(name, checks)
    v = SC.valid(rs[0].descs, rs[0].umem.size)
    if name == "all-invalid":
        assert summed == 0
    elif name == "edge-frames":
        # the parse decides some verdicts, and some checks lie where ihl < 5 puts them
        wv = np.concatenate([rd.want_verdicts for rd in rs])
        assert {-1, 0, SC.FWD} <= set(wv.tolist())
        off = SC.offsets(rs[0].descs)
        rel = np.concatenate([(rd.check_at - off)[rd.check_at >= 0] for rd in rs])
        assert (rel < 40).any() and (rel > 40).any() and (rel == 40).sum() > 400
    else:
        assert summed == ROUNDS * int(v.sum())
    if name in SC.VARY_LEN:
        assert not np.array_equal(rs[0].descs["len"], rs[1].descs["len"])
    if checks == "nic" and name not in ("all-invalid", "edge-frames"):
        # most of a NIC's checks stand under one iteration: few bytes change
        changed = sum(int((rd.want_umem != rd.umem).sum()) for rd in rs)
        assert changed < 0.2 * summed


def test_alternating_steps_keep_their_branches():
    steps = SC.alternating(SEED)
    assert [s[2] for s in steps] == [SC.case(n)[2] for n in SC.ALTERNATE]
    for (umem, descs, branch, wu, wv), name in zip(steps, SC.ALTERNATE):
        assert umem.size == SC.UMEM_MAX and SC.plan(descs, umem.size)[0] == branch, name
        assert (wv == SC.FWD).all() and not np.array_equal(wu, umem)
    # the batches share slots: each one's frames hold bytes of the frames of the one before
    masks = []
    for s in steps:
        m = np.zeros(SC.UMEM_MAX, dtype=bool)
        for o, n in zip(SC.offsets(s[1]).tolist(), s[1]["len"].tolist()):
            m[o:o + n] = True
        masks.append(m)
    for a, b in zip(masks[:-1], masks[1:]):
        assert (a & b).sum() > 1000
    assert {SC.RUNS, SC.TWO_D, SC.MAPPED_SCATTERED, SC.MAPPED_UNSORTED} == {s[2] for s in steps}
