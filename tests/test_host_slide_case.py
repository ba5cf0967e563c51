"""tests/slide_case.py, held to what it claims, without a device: the shift set reaches the placements that
tests/test_gpu_query_slide.py and tests/test_gpu_hit_track_slide.py are there for (asserted from the positions alone, on the set
those tests import), what is assembled per shift - the lead's own record, then the cargo's fixed records - equals every
reference run on the whole shifted batch, and the cargo holds the shapes it was built for."""
import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref
import hit_track_ref as htr
import read_depth_ref as rd
import repair_ref as rr
import screen_ref as sr
import slide_case as sc

PASS, TILE = sc.PASS, sc.TILE


@pytest.fixture(scope="module", params=sc.KS)
def case(request):
    return sc.case(request.param)


def _spread(c, n=20):
    """n shifts spread over the set, its first (the empty lead) and its last (all of L) among them"""
    shifts = c.shifts()
    return sorted({shifts[i * (len(shifts) - 1) // (n - 1)] for i in range(n)} | {c.k - 1, c.k})


# ---- 1. the shift set reaches what it claims -------------------------------------------------------------------------------------
def test_the_shift_set_reaches_every_placement(case):
    c, k = case, case.k
    shifts = c.shifts()
    assert shifts == sorted(set(shifts)) and shifts[0] == 0 and shifts[-1] <= sc.LEAD and set(range(130)) <= set(shifts)
    assert len(shifts) <= 700 and max(c.total(s) for s in shifts) <= 5100  # the run time's budget: calls, and bases per call
    at = np.array(shifts)
    for name, side, b0 in c.boundaries():
        where = at + b0
        for m in (4, 16, 32, 64):
            assert set(where % m) == set(range(m)), (name, side, m)
        assert any(all(e + d in where for d in range(-(k + 2), 3)) for e in (PASS, 2 * PASS)), (name, side)
        assert any(all(e + d in where for d in range(-2, 3)) for e in range(TILE, 5 * TILE, TILE)), (name, side)
    totals = {c.total(s) % PASS for s in shifts}
    assert {PASS - 1, 0, 1} <= totals
    # the k-base sequence: its bases [a, a + k) inside one bitmap word with both edge masks at work; at k = 32 no word holds 32
    # bases off its edge, and it is the range of its window starts, [a, a + 1), that is held to that
    a0 = c.starts0[c.index["k"]]
    span = k if k < 32 else 1
    assert any((s + a0) // 32 == (s + a0 + span - 1) // 32 and (s + a0) % 32 and (s + a0 + span) % 32 for s in shifts)
    assert any((s + a0) % PASS == PASS - 1 for s in shifts)  # it begins on the last position of a pass ...
    held = c.cargo_counters[c.index["k"]]
    assert len(held) == 1 and held[0] >= 2 and (k < 21 or held == [255])  # ... and its one window is held: at k = 32 that window needs the last base of the halo
    assert any((s + a0 + c.lengths[c.index["k"]]) % 32 == 0 for s in shifts)  # and it ends on the last bit of a word
    for name in sc.NAMES[1:]:  # a separator at the first position of a pass: behind every sequence
        assert any((s + c.ends0[c.index[name]]) % PASS == 0 for s in shifts), name
    # a broken stretch of the 400 bases straddles a multiple of 1024: every stretch of two windows or more does
    a400 = c.starts0[c.index["edited400"]]
    assert c.broken400
    for f, l in c.broken400:
        if l > f:
            assert any((s + a400 + f) // TILE < (s + a400 + l) // TILE for s in shifts), (f, l)


def test_thinning_keeps_what_the_assertions_need(case):
    c, k = case, case.k
    thin, full = c.shifts(thin=True), c.shifts()
    assert set(range(130)) <= set(thin) <= set(full)
    at = np.array(thin)
    for name, side, b0 in c.boundaries():
        lo = -(k + 2) if name in ("k", "w33", "long") else -2
        assert any(all(e + d in at + b0 for d in range(lo, 3)) for e in (PASS, 2 * PASS)), (name, side)
    assert {PASS - 1, 0, 1} <= {c.total(s) % PASS for s in thin}


# ---- 2. the references do not depend on position ---------------------------------------------------------------------------------
def test_the_assembled_answers_are_the_references_on_the_whole_batch(case):
    c, k = case, case.k
    cargo_tally = c.cargo_tally()
    for s in _spread(c):
        batch = c.batch(s)
        bases, offsets = c.packed(s)
        assert (bases.tobytes(), offsets.tolist()) == (sc.pack(batch)[0].tobytes(), sc.pack(batch)[1].tolist())
        assert c.total(s) == sum(len(x) + 1 for x in batch)
        per_read, counts = ref.Tally(c.db).add(batch, k, 3)
        want = c.want_add(s, 3)
        assert np.array_equal(want[0], per_read) and np.array_equal(want[1], counts), s
        per_read, counts = c.tally().add(bases, offsets, k, 3)
        assert np.array_equal(want[0], per_read) and np.array_equal(want[1], counts), s
        for window in sc.TRACK_WINDOWS:
            bins, prefix = c.want_track(s, cargo_tally, window)
            whole = ctr.track_np(cargo_tally, bases, offsets, k, window, sc.PEAK)
            assert ctr.equal(bins, whole[0]) and np.array_equal(prefix, whole[1]), (s, window)
        for min_count, min_support in sc.REPAIR_PARAMS:
            whole = rr.as_array(rr.repairs(c.db, batch, k, min_count, min_support))
            assert c.want_repairs(s, min_count, min_support).tobytes() == whole.tobytes(), (s, min_count, min_support)
        for min_count, max_count in sc.EVIDENCE_PARAMS:
            whole = sr.as_array(sr.evidence(c.db, batch, k, min_count, max_count))
            assert c.want_evidence(s, min_count, max_count).tobytes() == whole.tobytes(), (s, min_count, max_count)
        for min_count in sc.DEPTH_PARAMS:
            whole = rd.as_array(rd.read_depth(c.db, batch, k, min_count))
            assert c.want_read_depth(s, min_count).tobytes() == whole.tobytes(), (s, min_count)
        for ignore_case in (False, True):
            marks, runs, sums = c.want_track_marks(s, ignore_case)
            whole = htr.marks(bases, offsets, c.keys_a, c.keys_b, k, ignore_case)
            assert np.array_equal(marks, whole), (s, ignore_case)
            assert np.array_equal(runs, htr.runs(whole, offsets)) and np.array_equal(sums, htr.counts_of(whole, offsets)), (s, ignore_case)


@pytest.mark.parametrize("k", sc.KS)
def test_the_same_against_an_empty_database(k):
    c = sc.case(k, empty=True)
    full = sc.case(k)
    assert c.cargo == full.cargo and c.L == full.L and not c.db and np.array_equal(c.keys_a, full.keys_a)
    for s in (0, k - 1, k, k + 1, sc.SMALL[-1]):
        batch = c.batch(s)
        for min_count, min_support in sc.REPAIR_PARAMS:
            whole = rr.as_array(rr.repairs({}, batch, k, min_count, min_support))
            assert c.want_repairs(s, min_count, min_support).tobytes() == whole.tobytes(), (s, min_count, min_support)
            assert set(whole["kind"].tolist()) <= {rr.NONE, rr.LONG}
        assert c.want_evidence(s, 1, 255).tobytes() == sr.as_array(sr.evidence({}, batch, k)).tobytes()
        assert c.want_read_depth(s, 1).tobytes() == rd.as_array(rd.read_depth({}, batch, k)).tobytes()
        per_read, counts = c.want_add(s)
        assert not per_read[:, 1].any() and not counts.any() and int(per_read[0, 0]) == max(s - k + 1, 0)
        bins, prefix = c.want_track(s, c.cargo_tally(), 64)
        assert np.array_equal(bins["clean"], bins["absent"]) and int(bins["clean"].sum()) == int(per_read[:, 0].sum())


# ---- 3. the cargo is not vacuous -------------------------------------------------------------------------------------------------
def test_the_cargo_holds_the_shapes_it_was_built_for(case):
    c, k, at = case, case.k, case.index
    assert [len(x) for x in c.cargo] == [0, 1, k - 1, k, k + 1, k + 30, k + 31, k + 32, 160, 397, 2100 + k]
    assert c.cargo[at["n160"]].count("N") == 1 and any(ch.islower() for ch in c.cargo[at["n160"]])
    assert set(c.db.values()) == set(sc.COUNTERS)
    lead = set(ref.window_kmers(c.L, k))
    assert lead <= set(c.db) and all(c.db[km] >= 3 for km in lead) and len({c.db[km] for km in lead}) == 5
    long = c.cargo_counters[at["long"]]
    assert len(long) == 2101 and min(long) >= 3 and sum(x != y for x, y in zip(long, long[1:])) > 1500  # it changes from window to window
    # first and last windows are mixed, and neighbours meet held to held and absent to absent
    ends = {name: (bool(c.cargo_counters[at[name]][0]), bool(c.cargo_counters[at[name]][-1])) for name in sc.NAMES[3:]}
    if k >= 21:  # (below that a random window is in the database as often as not, and the reference alone says what is where)
        assert ends == {"k": (True, True), "k+1": (False, True), "w31": (True, False), "w32": (False, True), "w33": (True, True),
                        "n160": (True, False), "edited400": (False, False), "long": (True, True)}
    assert len(set(ends.values())) >= 3
    # repairs: every kind; stretches of 1, k - 1, k and k + 1 windows in the 400 bases
    kinds = set()
    for min_count, min_support in sc.REPAIR_PARAMS:
        kinds |= set(c.want_repairs(0, min_count, min_support)["kind"].tolist())
    assert kinds == {rr.NONE, rr.SUB, rr.DEL, rr.INS, rr.LONG}, kinds
    widths = {l - f + 1 for f, l in c.broken400}
    assert {1, k + 1} <= widths and (k < 21 or {1, 2, k - 1, k, k + 1} <= widths), widths
    mine = c.want_repairs(0, 3, 1)
    assert c.want_repairs(0, 2, 1).size < mine.size and not (mine["read"] == 0).any()  # counter 2 is broken from 3 on; the lead has none
    # evidence: several stretches in one sequence; depth: five distinct quantiles
    assert int(c.want_evidence(0, 1, 255)["stretches"].max()) >= 2 and int(c.want_evidence(0, 10, 20)["stretches"].max()) >= 2
    assert c.want_evidence(0, 1, 255).tobytes() != c.want_evidence(0, 10, 20).tobytes()
    depth = c.want_read_depth(0, 1)
    assert any(len({int(r[f]) for f in ("lowest", "q1", "median", "q3", "highest")}) == 5 for r in depth)
    assert depth.tobytes() != c.want_read_depth(0, 20).tobytes()
    # the track: collapsed, expanded and saturated windows at both window sizes; the tracker: both haplotypes in one sequence
    tally = c.cargo_tally()
    for window in sc.TRACK_WINDOWS:
        bins, prefix = c.want_track(0, tally, window)
        assert all(int(bins[f].sum()) > 0 for f in ("absent", "saturated", "collapsed", "expanded")), window
        assert int(prefix[1]) == 0 and int(prefix[-1]) == bins.size
    bins, _ = c.want_track(200, tally, 64)
    assert k < 21 or not bins["copies"][:2].any()  # the lead's k-mers were never added: a = 0
    marks, runs, sums = c.want_track_marks(0)
    assert c.in_both >= 3 and c.keys_a.size >= 3 and c.keys_b.size >= 3
    assert any({0, 1} <= set(runs["hap"][runs["read"] == r].tolist()) for r in range(1, len(c.cargo) + 1))
    assert not np.array_equal(marks, c.want_track_marks(0, True)[0])  # the lower-case stretch


def test_the_leads_evidence_walk_is_screen_refs_record(case):
    c, k = case, case.k
    for min_count, max_count in sc.EVIDENCE_PARAMS:
        for s in (0, 1, k - 1, k, k + 1, 2 * k, 100, 777, sc.LEAD):
            want = sr.record(c.lead_counters[:max(s - k + 1, 0)], s, k, sr.threshold(min_count), max_count)
            assert tuple(int(v) for v in c.want_evidence(s, min_count, max_count)[0]) == want, (s, min_count, max_count)
