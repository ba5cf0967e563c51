"""Fixed sequences slid through every stream offset of the hit tracker (kmers.HitTracker.marks and .runs, csrc/tbk_track.hip,
which shares its staging and its roll with the count-database query kernels through tbk_lookup.h), without `compress`.

The batches are those of tests/test_gpu_query_slide.py (tests/slide_case.py): a fixed cargo of sequences behind a lead L[:s], so
that over the shift set every boundary of the cargo meets every residue of the 16-base chunks, the 32-bit words of the two
marker bitmaps and the 64-base lanes, every place from k + 2 before to 2 behind a pass edge, and the edges of the run stage's
tiles of 1024.  The two lists are disjoint subsets of the database's k-mers plus a few that both hold (hapA wins).  The cargo's
marks and runs are hit_track_ref's for the cargo alone, computed once, with `read` moved by one; the lead's come from the marks
of L.  Every comparison is exact, and a failure names the shift, the sequence and where its ends lie modulo 4, 32 and 2048.

Run times on an MI355X, the slowest k (32): marks and runs over the whole shift set 0.53 s, the small set with one wave slot
0.05 s, with either case 0.02 s.  The scratch mutants of the staging and of the roll that this file was held against once, and
what noticed them: the table in tests/test_gpu_query_slide.py."""
import numpy as np
import pytest

import slide_case as sc

pytestmark = pytest.mark.gpu

KS = sc.KS


@pytest.fixture()
def tracker(gpu):
    """tracker(case) -> a HitTracker on the case's two lists; everything is closed at the end of the test"""
    from trio_binning_amd import kmers

    opened = []

    def make(c):
        sets = (kmers.HashSet.from_keys(c.keys_a, c.k), kmers.HashSet.from_keys(c.keys_b, c.k))
        opened.extend(sets)
        opened.append(kmers.HitTracker(*sets))
        return opened[-1]

    yield make
    for thing in reversed(opened):
        thing.close()


def _where(c, s, read):
    if read == 0:
        return "shift {}, the lead (read 0): stream positions 0 .. {}, total {}".format(s, s, c.total(s))
    return c.place(s, read - 1)


def _check(trk, c, s, ignore_case):
    from trio_binning_amd import kmers

    bases, offsets = c.packed(s)
    want, want_runs, want_counts = c.want_track_marks(s, ignore_case)
    what = "k {}, ignore_case {}".format(c.k, ignore_case)
    got = trk.marks(bases, offsets, ignore_case)
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        read = int(np.searchsorted(offsets, at, side="right")) - 1
        raise AssertionError("marks, {}: batch byte {} (window {} of read {}): {} for {} ({} bytes differ)\n{}".format(
            what, at, at - int(offsets[read]), read, got[at], want[at], int((got != want).sum()), _where(c, s, read)))
    runs, counts = trk.runs(bases, offsets, ignore_case)
    assert runs.dtype == np.dtype(kmers.HIT_RUN_DTYPE) == want_runs.dtype, what
    if not np.array_equal(counts, want_counts):
        read = int(np.flatnonzero((counts != want_counts).any(axis=1))[0])
        raise AssertionError("runs' counts, {}: read {}: {} for {}\n{}".format(what, read, counts[read], want_counts[read], _where(c, s, read)))
    if runs.tobytes() != want_runs.tobytes():
        n = min(runs.size, want_runs.size)
        i = next((i for i in range(n) if runs[i] != want_runs[i]), n)
        one, other = (runs[i] if i < runs.size else None), (want_runs[i] if i < want_runs.size else None)
        field = next((f for f in runs.dtype.names if one is not None and other is not None and one[f] != other[f]), "?")
        read = int((other if other is not None else one)["read"])
        raise AssertionError("runs, {}: {} runs for {}; run {}, field {!r}: got {}, want {}\n{}".format(
            what, runs.size, want_runs.size, i, field, one, other, _where(c, s, read)))


def _not_vacuous(c):
    marks, runs, counts = c.want_track_marks(0)
    assert (marks == 1).any() and (marks == 2).any() and counts[1:].any(axis=0).all()
    assert any({0, 1} <= set(runs["hap"][runs["read"] == r].tolist()) for r in range(1, len(c.cargo) + 1))  # both haplotypes in one sequence


@pytest.mark.parametrize("k", KS)
def test_marks_and_runs_at_every_stream_offset(tracker, k):
    c = sc.case(k)
    _not_vacuous(c)
    trk = tracker(c)
    for s in c.shifts():
        _check(trk, c, s, False)


@pytest.mark.parametrize("ignore_case", [False, True])
@pytest.mark.parametrize("k", KS)
def test_either_case_at_the_small_offsets(tracker, k, ignore_case):
    c = sc.case(k)
    assert not np.array_equal(c.want_track_marks(0, False)[0], c.want_track_marks(0, True)[0])  # the lower-case stretch holds markers
    trk = tracker(c)
    for s in sc.SMALL:
        _check(trk, c, s, ignore_case)


@pytest.mark.parametrize("k", KS)
def test_one_wave_slot_carries_from_pass_to_pass(gpu, tracker, k):
    """with one wave slot one wave takes every pass of a batch in turn: what it carries from one to the next is at work"""
    c = sc.case(k)
    assert c.total(0) > sc.PASS  # more than one pass even without a lead
    trk = tracker(c)
    assert gpu.lib.tbk_hit_tracker_set_wave_slots_(trk._h, 1) == 0
    for s in sc.SMALL:
        _check(trk, c, s, False)
        _check(trk, c, s, True)
