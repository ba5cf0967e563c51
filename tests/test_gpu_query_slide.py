"""Fixed sequences slid through every stream offset of the count-database query kernels (csrc/tbk_query.hip, tbk_depth.hip,
tbk_repair.hip, tbk_screen.hip, tbk_read_depth.hip, and the one lookup they share, tbk_lookup.h).

tests/slide_case.py builds, per k, a cargo of sequences - 0, 1, k - 1, k, k + 1 bases, 31, 32 and 33 windows, 160 bases with an N
and lower case, 400 bases with planted edits, one sequence longer than a pass - behind a lead L[:s].  Shift s moves every
boundary of the cargo by s stream positions, so over the shift set every boundary meets every residue of the 4-byte counter
words, the 16-base chunks, the 32-bit bitmap words and the 64-base lanes, every place from k + 2 before to 2 behind a pass edge,
and the tile edges of the compactions; `total` ends one before, on and one past a pass.  The cargo's records do not depend on s:
they are the references' answers for the cargo alone, computed once (tests/test_host_slide_case.py holds that to the references
run on whole shifted batches, and the shift set to what it reaches).  Everything is integers and every comparison is exact.  A
failure names the shift, the sequence, the first field that differs and where the sequence's ends lie modulo 4, 32 and 2048.

The shift set has 352, 541 and 646 shifts at k = 5, 21 and 32, and a batch at most 5037 bases.  Run times on an MI355X, the slowest
k (32) of each test, references included: add 0.44 s, track 0.45 s, repairs 0.91 s, evidence 0.11 s, read_depth 0.22 s; a case
of the two small-set tests 0.53 s (repairs with one wave slot) or less, most of them 0.01 s; the 46 tests of this file and the
12 of tests/test_gpu_hit_track_slide.py (marks and runs over the whole set: 0.53 s) together 8.0 s.  Nothing had to be thinned
(slide_case.shifts(thin=True) is what would be).

Held once against scratch mutants, each a change of one mask or stored value in a copy of the sources, built by itself, run once
on an MI355X and never committed.  "whole set": the test_*_at_every_stream_offset of that call; every mutant also failed
test_one_wave_slot_carries_from_pass_to_pass and, but for the two byte masks, test_an_empty_database_at_the_small_offsets.
  mutant                                              the slide tests that failed            the earlier tests that failed
  range_word_mask: last word shifted by 30u - ...     whole set: add, evidence, read_depth   copy_track 14, db_query 15, read_depth 10,
                                                      at k 5, 21; track at k 5, 21, 32       screen_evidence 8 cases
  LaneWindows::load: halo staged by lane < 1 only     whole set: all five calls and the      copy_track 5, db_query 24, read_depth 12,
                                                      tracker at k 21, 32                    repairs 7, screen_evidence 6, hit_track 53
  LaneWindows::roll: bad_hi << 30                     whole set: all five calls and the      copy_track 10, db_query 108, read_depth 21,
                                                      tracker at k 5, 21, 32                 repairs 11, screen_evidence 14, hit_track 158
  tbk_read_depth_kernel: first byte mask (a + 1) & 3  whole set: read_depth at k 5, 21, 32   read_depth 22 cases; no other file
  tbk_depth_bin_kernel: last byte mask p1 & 3         whole set: track at k 5, 21, 32        copy_track 9 cases; no other file
No mutant passed the slide tests, and none passed the earlier tests of its own call (tests/test_gpu_db_query.py,
test_gpu_copy_track.py, test_gpu_repairs.py, test_gpu_screen_evidence.py, test_gpu_read_depth.py, test_gpu_hit_track.py): their
long batches of many sequences and their fuzz reach these masks too, by the offsets their sequences happen to add up to.  What
the slide tests add is that every offset is reached by construction, for every call, and that a failure names the placement.
The first mutant keeps one bit too many - the separator's, or a window start among a sequence's last k - 1, which is never
clean - unless the range ends on the last bit of a word, where it keeps the word's bit 0 alone: at k = 32 the 31 bits it drops
there are never set in a range of a whole sequence, so add, evidence and read_depth cannot notice it at k = 32 and the track,
whose bins end inside a sequence, does.  The halo mutant needs a window that reaches past a lane's 48th base: k above 17.
"""
import numpy as np
import pytest

import copy_track_ref as ctr
import read_depth_ref as rd
import repair_ref as rr
import screen_ref as sr
import slide_case as sc

pytestmark = pytest.mark.gpu

KS = sc.KS
CALLS = ("add", "track", "repairs", "evidence", "read_depth")
FOUND_FROM = 3  # add's min_count: a counter of 2 is clean and not found


@pytest.fixture()
def load(gpu, tmp_path):
    """load(file bytes) -> KmerDatabase; closed at the end of the test"""
    from trio_binning_amd import kmers

    opened = []

    def _load(data):
        path = tmp_path / "db{}.tbkdb".format(len(opened))
        path.write_bytes(data)
        opened.append(kmers.KmerDatabase.load(str(path)))
        return opened[-1]

    yield _load
    for d in opened:
        d.close()


# ---- what a failure says -------------------------------------------------------------------------------------------------------------
def _where(c, s, read):
    if read == 0:
        return "shift {}, the lead (read 0): stream positions 0 .. {}, total {}".format(s, s, c.total(s))
    return c.place(s, read - 1)


def _records(c, s, what, got, want, read_of=lambda i, rec: i):
    """two structured arrays, record for record; read_of(i, wanted record) -> the read the record belongs to"""
    assert got.dtype == want.dtype, what
    if got.tobytes() == want.tobytes():
        return
    if got.size != want.size:
        raise AssertionError("{}: {} records for {}; shift {}, total {}".format(what, got.size, want.size, s, c.total(s)))
    for i in range(got.size):
        if got[i].tobytes() != want[i].tobytes():
            field = next((f for f in got.dtype.names if got[i][f].tobytes() != want[i][f].tobytes()), "?")
            raise AssertionError("{}: record {}, field {!r}: {} for {}; got {}, want {}\n{}".format(
                what, i, field, got[i][field], want[i][field], got[i], want[i], _where(c, s, read_of(i, want[i]))))


def _bytes(c, s, what, got, want, offsets):
    """two arrays with one byte per base of the batch"""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if np.array_equal(got, want):
        return
    at = int(np.flatnonzero(got != want)[0])
    read = int(np.searchsorted(offsets, at, side="right")) - 1
    raise AssertionError("{}: batch byte {} (base {} of read {}): {} for {} ({} bytes differ)\n{}".format(
        what, at, at - int(offsets[read]), read, got[at], want[at], int((got != want).sum()), _where(c, s, read)))


# ---- one call at one shift -----------------------------------------------------------------------------------------------------------
def _add(query, c, s, state):
    bases, offsets = c.packed(s)
    per_read, counts = query.add(bases, offsets, FOUND_FROM, True)
    want_per_read, want_counts = c.want_add(s, FOUND_FROM)
    again = state["tally"].add(bases, offsets, c.k, FOUND_FROM)  # the tally is given the same shifted batch
    assert np.array_equal(again[0], want_per_read) and np.array_equal(again[1], want_counts), s
    what = "add, k {}".format(c.k)
    _bytes(c, s, what + ", counts", counts, want_counts, offsets)
    assert per_read.shape == want_per_read.shape, what
    if not np.array_equal(per_read, want_per_read):
        read = int(np.flatnonzero((per_read != want_per_read).any(axis=1))[0])
        raise AssertionError("{}: per_read[{}] (clean, found) is {} for {}\n{}".format(what, read, per_read[read], want_per_read[read], _where(c, s, read)))


def _track(query, c, s, state):
    bases, offsets = c.packed(s)
    for window in sc.TRACK_WINDOWS:
        bins, prefix = query.track(bases, offsets, window, sc.PEAK)
        want, want_prefix = c.want_track(s, state["cargo_tally"], window)
        what = "track, k {}, window {}".format(c.k, window)
        assert prefix.dtype == np.uint64 and np.array_equal(prefix, want_prefix), (what, s)
        _records(c, s, what, bins, want, lambda i, rec: int(np.searchsorted(want_prefix, i, side="right")) - 1)


def _repairs(query, c, s, state):
    bases, offsets = c.packed(s)
    for min_count, min_support in sc.REPAIR_PARAMS:
        got = query.repairs(bases, offsets, min_count, min_support)
        want = c.want_repairs(s, min_count, min_support)
        what = "repairs, k {}, min_count {}, min_support {}".format(c.k, min_count, min_support)
        if got.size != want.size:  # name the first stretch that is missing or too many
            mine, theirs = [(int(r["read"]), int(r["first"])) for r in got], [(int(r["read"]), int(r["first"])) for r in want]
            odd = sorted(set(mine) ^ set(theirs))
            raise AssertionError("{}: {} records for {}; (read, first) in one only: {}\n{}".format(
                what, got.size, want.size, odd[:6], _where(c, s, odd[0][0]) if odd else ""))
        _records(c, s, what, got, want, lambda i, rec: int(rec["read"]))


def _evidence(query, c, s, state):
    bases, offsets = c.packed(s)
    for min_count, max_count in sc.EVIDENCE_PARAMS:
        got = query.evidence(bases, offsets, min_count, max_count)
        _records(c, s, "evidence, k {}, counters {} .. {}".format(c.k, min_count, max_count), got, c.want_evidence(s, min_count, max_count))


def _read_depth(query, c, s, state):
    bases, offsets = c.packed(s)
    for min_count in sc.DEPTH_PARAMS:
        got = query.read_depth(bases, offsets, min_count)
        _records(c, s, "read_depth, k {}, min_count {}".format(c.k, min_count), got, c.want_read_depth(s, min_count))


CHECK = {"add": _add, "track": _track, "repairs": _repairs, "evidence": _evidence, "read_depth": _read_depth}


def _session_state(query):
    return (query.histogram(),) + tuple(query.completeness(*pair) for pair in sc.COMPLETENESS) + (query.copy_spectrum(),)


def _slide(gpu, load, c, call, shifts, wave_slots=None):
    """one session, one call, every shift"""
    with load(c.file).query(copies=True) as query:
        if wave_slots:
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, wave_slots) == 0
        state = {"tally": c.tally()}
        if call == "track":  # the copies of the track: the unshifted cargo, once
            query.add(c.cargo_bytes, c.cargo_offsets)
            state["cargo_tally"] = c.cargo_tally()
            state["tally"].add(c.cargo_bytes, c.cargo_offsets, c.k)
        before = _session_state(query)
        for s in shifts:
            CHECK[call](query, c, s, state)
        after = _session_state(query)
        tally = state["tally"]
        want = (tally.hist,) + tuple(tally.completeness(*pair) for pair in sc.COMPLETENESS) + (tally.spectrum(),)
        for name, got, wanted in zip(("histogram", "completeness", "completeness", "copy_spectrum"), after, want):
            assert np.array_equal(got, wanted), (call, c.k, name)
        if call != "add":  # every other call only reads the session
            assert all(np.array_equal(a, b) for a, b in zip(before, after)), (call, c.k)
        else:
            assert int(after[0].sum()) > int(before[0].sum()) == 0


# ---- 1. every call over the whole shift set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_add_at_every_stream_offset(gpu, load, k):
    """per_read and the count bytes per shift; at the end histogram, completeness at two cut-off pairs and the copy spectrum
    against a TallyNp that was given the same shifted batches"""
    c = sc.case(k)
    _slide(gpu, load, c, "add", c.shifts())


@pytest.mark.parametrize("k", KS)
def test_track_at_every_stream_offset(gpu, load, k):
    """bins and prefix at windows of 64 and 100 window starts, on a session that was given the unshifted cargo once; the peak
    makes windows collapsed, expanded and neither, and 255 is saturated"""
    c = sc.case(k)
    _slide(gpu, load, c, "track", c.shifts())


@pytest.mark.parametrize("k", KS)
def test_repairs_at_every_stream_offset(gpu, load, k):
    c = sc.case(k)
    _slide(gpu, load, c, "repairs", c.shifts())


@pytest.mark.parametrize("k", KS)
def test_evidence_at_every_stream_offset(gpu, load, k):
    c = sc.case(k)
    _slide(gpu, load, c, "evidence", c.shifts())


@pytest.mark.parametrize("k", KS)
def test_read_depth_at_every_stream_offset(gpu, load, k):
    c = sc.case(k)
    _slide(gpu, load, c, "read_depth", c.shifts())


# ---- 2. the small set again: one wave slot, and an empty database ---------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("k", KS)
def test_one_wave_slot_carries_from_pass_to_pass(gpu, load, k, call):
    """with one wave slot one wave takes every pass, and one wave every sequence, of a batch in turn: what it carries from one
    to the next - staged chunks, rows of LDS, counts - is at work at shifts 0 .. 35"""
    c = sc.case(k)
    assert c.total(0) > sc.PASS  # more than one pass even without a lead
    _slide(gpu, load, c, call, sc.SMALL, wave_slots=1)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("k", KS)
def test_an_empty_database_at_the_small_offsets(gpu, load, k, call):
    """every clean window is absent, nothing is found, and the repairs are all NONE or LONG - the lead's stretch among them"""
    c = sc.case(k, empty=True)
    if call == "repairs":
        for params in sc.REPAIR_PARAMS:
            want = c.want_repairs(sc.SMALL[-1], *params)
            assert set(want["kind"].tolist()) == {rr.NONE, rr.LONG} and int(want[0]["read"]) == 0
    _slide(gpu, load, c, call, sc.SMALL)


def test_the_references_dtypes_are_the_packages(gpu):
    from trio_binning_amd import kmers

    assert kmers.DEPTH_BIN == ctr.BIN and kmers.REPAIR == rr.REPAIR and kmers.READ_EVIDENCE == sr.READ_EVIDENCE and kmers.READ_DEPTH == rd.READ_DEPTH
