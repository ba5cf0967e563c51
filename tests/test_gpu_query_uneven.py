"""A query session (tbk_kmerdb_query_*: csrc/tbk_query.hip, tbk_depth.hip, tbk_repair.hip, tbk_screen.hip) on the uneven database
of tests/uneven_case.py: a directory of 17 bits with a mean bucket of two to three entries and one bucket of more than 4096,
whose searches run 13 bisection steps in the same group of four in-flight windows as searches that end at once.  The batch
hits that bucket's first, last and middle entry, misses below, above and between its entries and in the empty buckets beside
it, hits rank 0 and the database's last entry on either strand and in lower case, carries a substitution, a missing and an extra
base whose candidates' windows lie partly in the deep bucket, and crosses the pass edge at stream position 2048 inside a run of
deep hits.  tests/test_host_query_uneven.py asserts all of that without a device, and `claims` asserts it here again, so that
nothing below can run vacuous.  add, counts, histogram, completeness, copy spectrum and track are held to the numpy references
(db_query_ref.TallyNp, copy_track_ref.track_np), repairs and evidence to the Python loops (repair_ref, screen_ref) over
tests/rank_db.py, on the solid database and on its full twin.  Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import copy_track_ref as ctr
import repair_ref as rr
import screen_ref as sr
import uneven_case as uc

pytestmark = pytest.mark.gpu

CUTS = ((2, 255), (10, 200))


@pytest.fixture(scope="module")
def case(gpu):
    c = uc.case()
    uc.claims(c)
    return c


@pytest.fixture(scope="module")
def databases(gpu, case, tmp_path_factory):
    from trio_binning_amd import kmers

    opened = {}
    for full in (False, True):
        path = tmp_path_factory.mktemp("uneven") / "{}.tbkdb".format("full" if full else "solid")
        path.write_bytes(case.files[full])
        opened[full] = kmers.KmerDatabase.load(str(path))
        assert len(opened[full]) == case.ranks[full].size and opened[full].floor == (1 if full else 2)
    yield opened
    for db in opened.values():
        db.close()


def _state(query):
    return (query.histogram(), query.completeness(), query.completeness(10, 200)) + ((query.copy_spectrum(),) if query.copies else ())


def _same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_tally(query, tally, what):
    assert np.array_equal(query.histogram(), tally.hist), what
    for cuts in CUTS:
        assert query.completeness(*cuts) == tally.completeness(*cuts), (what, cuts)
    spec = query.copy_spectrum()
    assert np.array_equal(spec, tally.spectrum()), (what, np.argwhere(spec != tally.spectrum())[:10])


def _check_tracks(query, c, tally, state, full):
    before = _state(query)
    for window in uc.WINDOWS:
        want, want_prefix = c.want_track(tally, state, full, window)
        bins, prefix = query.track(*c.packed, window, uc.PEAK)
        what = "full {}, added {} times, window {}".format(full, state, window)
        assert bins.dtype == ctr.BIN and np.array_equal(prefix, want_prefix), what
        assert ctr.equal(bins, want), (what, ctr.first_difference(bins, want))
    assert _same_state(_state(query), before)


@pytest.mark.parametrize("full", (False, True), ids=("solid", "full"))
def test_add_counts_and_track_against_the_numpy_references(case, databases, full):
    c = case
    with databases[full].query(copies=True) as query:
        tally = c.tally(full)
        _check_tracks(query, c, tally, 0, full)  # before anything was added
        per_read, counts = query.add(*c.packed, return_counts=True)
        want_per_read, want_counts = tally.add(*c.packed, uc.K)
        assert np.array_equal(counts, want_counts), np.flatnonzero(counts != want_counts)[:10]
        assert np.array_equal(per_read, want_per_read), np.flatnonzero((per_read != want_per_read).any(axis=1))[:10]
        _check_tally(query, tally, "added once")
        _check_tracks(query, c, tally, 1, full)
        again = query.counts(*c.packed)  # (counts adds the batch as add does)
        tally.add(*c.packed, uc.K)
        assert np.array_equal(again, want_counts), np.flatnonzero(again != want_counts)[:10]
        _check_tally(query, tally, "added twice")
        _check_tracks(query, c, tally, 2, full)
    with databases[full].query() as query:  # a session without copies answers add and counts alike
        plain = c.tally(full)
        per_read, counts = query.add(*c.packed, return_counts=True)
        want_per_read, want_counts = plain.add(*c.packed, uc.K)
        assert np.array_equal(counts, want_counts) and np.array_equal(per_read, want_per_read)
        assert np.array_equal(query.histogram(), plain.hist) and query.completeness() == plain.completeness()


def _check_repairs(query, c, min_count, min_support, full, what=""):
    from trio_binning_amd import kmers

    want = c.want_repairs(min_count, min_support, full)
    before = _state(query)
    got = query.repairs(*c.packed, min_count, min_support)
    what = "{} min_count {}, min_support {}, full {}".format(what, min_count, min_support, full)
    assert got.dtype == kmers.REPAIR == rr.REPAIR, what
    assert got.tobytes() == want.tobytes(), (what, rr.first_difference(got, want))
    assert _same_state(_state(query), before), what


def _check_evidence(query, c, min_count, max_count, full, what=""):
    from trio_binning_amd import kmers

    want = c.want_evidence(min_count, max_count, full)
    before = _state(query)
    got = query.evidence(*c.packed, min_count, max_count)
    what = "{} range [{}, {}], full {}".format(what, min_count, max_count, full)
    assert got.dtype == kmers.READ_EVIDENCE == sr.READ_EVIDENCE, what
    assert got.tobytes() == want.tobytes(), (what, sr.first_difference(got, want))
    assert _same_state(_state(query), before), what


@pytest.mark.parametrize("full", (False, True), ids=("solid", "full"))
def test_repairs_against_the_loop_reference(case, databases, full):
    with databases[full].query(copies=full) as query:
        for min_count, min_support in uc.REPAIR_PARAMETERS[full]:
            _check_repairs(query, case, min_count, min_support, full)
        query.add(*case.packed)  # what was added changes no answer
        _check_repairs(query, case, 2, 1, full, "after an add,")


@pytest.mark.parametrize("full", (False, True), ids=("solid", "full"))
def test_evidence_against_the_loop_reference(case, databases, full):
    with databases[full].query(copies=not full) as query:
        for min_count, max_count in uc.RANGES:
            _check_evidence(query, case, min_count, max_count, full)
        per_read = query.add(*case.packed)
        whole = case.want_evidence(1, 255, full)
        assert np.array_equal(per_read[:, 0], whole["clean"])
        if not full:  # (on a full database add's found asks for c >= 2, the evidence for c >= 1)
            assert np.array_equal(per_read[:, 1], whole["held"])


@pytest.mark.parametrize("slots", (1, 2))
@pytest.mark.parametrize("full", (False, True), ids=("solid", "full"))
def test_small_grids_take_the_deep_searches_on_a_later_trip(gpu, case, databases, full, slots):
    """with one wave every pass behind the first is a later trip of the pass loop - the pass edge inside the run of deep hits is
    one between two trips of one wave - and with two the third and fourth pass are, where deep hits and three of the errors lie"""
    with databases[full].query(copies=True) as query:
        assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
        for min_count, min_support in uc.REPAIR_PARAMETERS[full]:
            _check_repairs(query, case, min_count, min_support, full, "{} slots,".format(slots))
        for min_count, max_count in uc.RANGES:
            _check_evidence(query, case, min_count, max_count, full, "{} slots,".format(slots))
        tally = case.tally(full)
        _check_tracks(query, case, tally, 0, full)
        counts = query.counts(*case.packed)
        assert np.array_equal(counts, tally.add(*case.packed, uc.K)[1])
