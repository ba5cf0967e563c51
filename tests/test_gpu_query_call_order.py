"""The five methods of one query session (tbk_kmerdb_query_*) called interleaved, with batches that shrink and grow.  In one
session the device buffers are shared and only grow: `found_bits` is the found, present, broken or held bitmap depending on the
caller, `bytes` belongs to add(return_counts) and to track, and `sep`, `offsets` and `clean_bits` belong to every pass.  A fixed
script runs every pass once directly behind each other pass with the larger batch before it - `small` behind `big` is where a
pass that reads a word which an earlier, larger call left behind would give another answer - and `big` behind `small`, where a
buffer that was reserved too small would show.  After each call its answer is the reference's for that call alone, given the tally
so far; after each read-only call the session's state is what it was, and after each call it is the reference tally's.

`big` is the first batch of tests/test_gpu_copy_track.py's case (more than seven passes, 23 sequences, nine of them shorter than
k, some empty); `small` has three sequences over fewer than 2048 stream positions and ends in the middle of a bitmap word.  Once
on a session with copies on the solid database, once without copies - and without the track calls - on a full twin of it with
min_count 1.  Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref
import kmerdb_files as kf
import repair_ref as rr
import screen_ref as sr
from test_gpu_copy_track import PASS, Case

pytestmark = pytest.mark.gpu

FULL = b"TBKKMFB1"
WINDOW, PEAK = 64, 10
# (method, batch, arguments); for repairs the argument is min_count - None: the session's lowest, 2 on a solid and 1 on a full database
SCRIPT = (("track", "big"), ("add_counts", "big"), ("evidence", "small", 1, 255), ("repairs", "big", None), ("track", "small"), ("counts", "big"),
          ("evidence", "big", 1, 255), ("repairs", "small", None), ("add", "small"), ("track", "big"), ("repairs", "small", 10),
          ("evidence", "small", 255, 255), ("counts", "small"), ("reset",), ("track", "small"), ("evidence", "big", 1, 255))
READ_ONLY = ("track", "evidence", "repairs")


class Ordered:
    """The copy-track case of one k, a small batch beside its first one, a full twin of its database, and the references' answers."""

    def __init__(self, k):
        from trio_binning_amd import kmers

        c = Case(k)
        self.k, self.c = k, c
        long_one = c.first[0]
        hurt = list(long_one[300:900])
        hurt[200] = "ACGT"[("ACGT".index(hurt[200].upper()) + 1) % 4]
        self.batches = {"big": c.first, "small": ["".join(hurt), long_one[1990:2400], c.first[-1][:345]]}
        assert "N" in self.batches["small"][1] and len(self.batches["small"]) == 3
        stream = {name: sum(len(s) + 1 for s in b) for name, b in self.batches.items()}
        assert stream["big"] > 7 * PASS and len(c.first) > 20 and sum(len(s) < k for s in c.first) >= 4 and "" in c.first
        assert stream["small"] < PASS and 4 <= (stream["small"] - 2) % 32 <= 27  # its last base lies in the middle of a bitmap word
        self.packed = {name: kmers.pack_reads(b) for name, b in self.batches.items()}
        self.lengths = {name: [len(s) for s in b] for name, b in self.batches.items()}
        # the full twin: the database and, seen once, the first 150 k-mers of the batch that it does not hold
        absent = []
        for km in (km for s in c.first for km in ref.window_kmers(s, k)):
            if km is not None and km not in c.db and km not in absent and len(absent) < 150:
                absent.append(km)
        if k <= 5:  # (every small k-mer the database does not hold is among them: keep every other one, or nothing is absent)
            absent = absent[::2]
        full_db = dict(c.db, **{km: 1 for km in absent})
        self.dbs = {False: c.db, True: full_db}
        self.tables, self.files = {False: (c.ranks, c.counters)}, {False: c.file}
        ranks = np.array(sorted(ref.lex_rank(km) for km in full_db), dtype=np.uint64)
        by_rank = {ref.lex_rank(km): v for km, v in full_db.items()}
        counters = np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
        hist = np.bincount(counters, minlength=256).astype(np.uint64)
        hist[0] = ranks.size
        self.tables[True], self.files[True] = (ranks, counters), kf.file_bytes(k, ranks, counters, hist, reads=1, bases=k, magic=FULL)
        self.n_once = len(absent)
        self._answers = {}

    def tally(self, full):
        return ref.TallyNp(*self.tables[full])

    def answer(self, full, method, batch, *args):
        """what does not depend on the tally, computed once"""
        key = (full, method, batch) + args
        if key not in self._answers:
            floor = 1 if full else 2
            if method == "repairs":
                self._answers[key] = rr.as_array(rr.repairs(self.dbs[full], self.batches[batch], self.k, args[0], 1, floor=floor))
            else:
                if (full, "counters", batch) not in self._answers:
                    self._answers[full, "counters", batch] = sr.window_counters(self.dbs[full], self.batches[batch], self.k)
                self._answers[key] = sr.as_array(sr.records(self._answers[full, "counters", batch], self.lengths[batch], self.k, *args, floor=floor))
        return self._answers[key]


_ORDERED = {}


@pytest.fixture(scope="module")
def ordered(gpu):
    def get(k):
        if k not in _ORDERED:
            _ORDERED[k] = Ordered(k)
        return _ORDERED[k]

    yield get
    _ORDERED.clear()


def _state(query):
    return (query.histogram(), query.completeness(), query.completeness(10, 200)) + ((query.copy_spectrum(),) if query.copies else ())


def _state_of(tally, copies):
    return (tally.hist, tally.completeness(), tally.completeness(10, 200)) + ((tally.spectrum(),) if copies else ())


def _same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _found(counts, bases, offsets, k, m):
    """per sequence: its clean windows with a counter of at least m"""
    clean = ref.window_ranks(bases, offsets, k)[1]
    before = np.concatenate([[0], np.cumsum(clean & (counts >= m))]).astype(np.uint64)
    off = np.asarray(offsets).astype(np.int64)
    return before[off[1:]] - before[off[:-1]]


def run_script(o, query, full, copies):
    from trio_binning_amd import kmers

    k, lowest = o.k, 1 if full else 2
    tally = o.tally(full)
    done = []
    for step, (method, *rest) in enumerate(SCRIPT, 1):
        if method == "track" and not copies:
            continue
        what = "k {}, step {}: {}{}, behind {}".format(k, step, method, tuple(rest), done[-1] if done else None)
        before = _state(query)
        if method == "reset":
            query.reset()
            tally = o.tally(full)
        elif method == "track":
            want, want_prefix = ctr.track_np(tally, *o.packed[rest[0]], k, WINDOW, PEAK)
            bins, prefix = query.track(*o.packed[rest[0]], WINDOW, PEAK)
            assert bins.dtype == ctr.BIN and np.array_equal(prefix, want_prefix), what
            assert ctr.equal(bins, want), (what, ctr.first_difference(bins, want))
        elif method == "evidence":
            want = o.answer(full, "evidence", *rest)
            got = query.evidence(*o.packed[rest[0]], *rest[1:])
            assert got.dtype == kmers.READ_EVIDENCE and got.tobytes() == want.tobytes(), (what, sr.first_difference(got, want))
        elif method == "repairs":
            min_count = lowest if rest[1] is None else rest[1]
            want = o.answer(full, "repairs", rest[0], min_count)
            got = query.repairs(*o.packed[rest[0]], min_count, 1)
            assert got.dtype == kmers.REPAIR and got.tobytes() == want.tobytes(), (what, rr.first_difference(got, want))
        else:
            want_per_read, want_counts = tally.add(*o.packed[rest[0]], k)
            want_per_read[:, 1] = _found(want_counts, *o.packed[rest[0]], k, lowest)
            if method == "counts":
                counts = query.counts(*o.packed[rest[0]])
            elif method == "add_counts":
                per_read, counts = query.add(*o.packed[rest[0]], lowest, return_counts=True)
            else:
                per_read, counts = query.add(*o.packed[rest[0]], lowest), None
            if method != "counts":
                assert np.array_equal(per_read, want_per_read), (what, np.flatnonzero((per_read != want_per_read).any(axis=1))[:10])
            if counts is not None:
                assert np.array_equal(counts, want_counts), (what, np.flatnonzero(counts != want_counts)[:10])
        after = _state(query)
        if method in READ_ONLY:
            assert _same_state(after, before), what
        assert _same_state(after, _state_of(tally, copies)), what
        done.append((method,) + tuple(rest))
    return done


@pytest.mark.parametrize("k", (4, 21))
def test_any_call_order_in_a_session_with_copies(gpu, ordered, tmp_path, k):
    from trio_binning_amd import kmers

    o = ordered(k)
    path = tmp_path / "solid.tbkdb"
    path.write_bytes(o.files[False])
    with kmers.KmerDatabase.load(str(path)) as db, db.query(copies=True) as query:
        done = run_script(o, query, False, True)
    assert len(done) == len(SCRIPT)
    # not vacuous: every pass runs directly behind each other pass on the larger batch, and on the larger batch behind the smaller
    passes = {"track": "track", "evidence": "evidence", "repairs": "repairs", "add": "add", "add_counts": "add", "counts": "add"}
    pairs = {(passes[a[0]], passes[b[0]]) for a, b in zip(done, done[1:]) if a[0] != "reset" and b[0] != "reset" and a[1] == "big" and b[1] == "small"}
    assert pairs >= {("add", "evidence"), ("repairs", "track"), ("evidence", "repairs"), ("track", "repairs")}, pairs
    assert any(a[0] != "reset" and b[0] != "reset" and a[1] == "small" and b[1] == "big" for a, b in zip(done, done[1:]))
    assert o.answer(False, "repairs", "small", 2).size > 0 and o.answer(False, "evidence", "small", 1, 255)["held"].any()
    assert o.answer(False, "repairs", "small", 10).tobytes() != o.answer(False, "repairs", "small", 2).tobytes()
    assert o.answer(False, "evidence", "small", 255, 255).tobytes() != o.answer(False, "evidence", "small", 1, 255).tobytes()


@pytest.mark.parametrize("k", (4, 21))
def test_any_call_order_in_a_session_without_copies_on_a_full_database(gpu, ordered, tmp_path, k):
    from trio_binning_amd import kmers

    o = ordered(k)
    path = tmp_path / "full.tbkdb"
    path.write_bytes(o.files[True])
    with kmers.KmerDatabase.load(str(path)) as db, db.query() as query:
        assert db.floor == 1 and not query.copies
        done = run_script(o, query, True, False)
    assert len(done) == len(SCRIPT) - sum(step[0] == "track" for step in SCRIPT)
    # not vacuous: the k-mers seen once are at work - held with min_count 1, broken with 2
    assert o.n_once > 0 and o.answer(True, "evidence", "big", 1, 255)["held"].sum() > o.answer(False, "evidence", "big", 1, 255)["held"].sum()
    assert o.answer(True, "repairs", "big", 1).size > 0 and o.answer(True, "repairs", "big", 1).tobytes() != o.answer(False, "repairs", "big", 2).tobytes()
