"""The second trip of the database query's strided loops (csrc/tbk_query.hip): tbk_query_lookup_kernel - all four template forms,
BYTES x COPIES - strides over the passes by the session's wave_slots and keeps its LDS histogram across the trips, flushing it
once behind the loop; tbk_query_totals_kernel and tbk_query_counts_kernel stride over the sequences.  wave_slots is compute
units x 32, so nothing a Python loop can follow ever wraps them.  tbk_kmerdb_query_set_wave_slots_ (a test hook) makes the grid
1, 2, 3 or 5 waves: a batch of 23 sequences over 8 passes then takes up to eight trips.

The session is held to db_query_ref.Tally, computed once per k: the per-sequence totals, the counter of every window, the
histogram, completeness and the copy spectrum, after one batch, after a second one, and after reset() and the first batch
again.  Counter 0 and every counter 2..255 occur in every pass of the first batch, so a histogram that is flushed per trip, or not
carried from one trip to the next, is wrong in every row.  Every comparison is exact."""
import numpy as np
import pytest

import db_query_ref as ref

pytestmark = pytest.mark.gpu

KS = (5, 21, 32)
PASS = 2048
PASSES = 8
SLOTS = (1, 2, 3, 5)
STREAM = (PASSES - 1) * PASS + 1900  # the separated stream of the first batch: seven full passes and a partial one
BODY = 1400                          # a sequence that lies inside one pass
CUTS = ((2, 255), (100, 200))
INSIDE = (0, 4, 7, 10, 13, 16, 18, 22)  # the sequences of the first batch that lie inside one pass


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _layout(k):
    """The lengths of the 23 sequences.  BODY lies inside its pass; ("edge", p) ends 250 + 10 p positions behind stream position
    2048 p, whatever came before it; "rest" fills the stream up to STREAM."""
    plan = [BODY, 0, k - 1, ("edge", 1), BODY, k, ("edge", 2), BODY, 0, ("edge", 3), BODY, 1, ("edge", 4), BODY, k + 1, ("edge", 5),
            BODY, ("edge", 6), BODY, 0, ("edge", 7), 2, "rest"]
    lengths, at = [], 0  # at: the stream position of the next sequence's first base
    for item in plan:
        if item == "rest":
            n = STREAM - 1 - at
            assert n >= BODY and at // PASS == PASSES - 1
        elif isinstance(item, tuple):
            n = item[1] * PASS + 250 + 10 * item[1] - at
            assert at <= item[1] * PASS - 150  # the sequence holds the 150 positions on either side of the edge
        else:
            n = item
            assert item != BODY or at // PASS == (at + BODY) // PASS
        lengths.append(n)
        at += n + 1
    assert at == STREAM and len(lengths) == 23
    return lengths


def _stream(per_base, sequences):
    """one value per base of a batch -> the same by position of the separated stream (0 at the separators)"""
    out = np.zeros(sum(len(s) + 1 for s in sequences), dtype=per_base.dtype)
    at = 0
    for r, s in enumerate(sequences):
        out[at + r:at + r + len(s)] = per_base[at:at + len(s)]
        at += len(s)
    return out


class Case:
    """Two batches, a database made from part of the first, and everything the reference says about them - for one k."""

    def __init__(self, k):
        rng = np.random.default_rng(50 + k)
        self.k = k
        lengths = _layout(k)
        if k == 5:
            # 300 of the 512 canonical 5-mers are held; each of the first 254, one per counter, is written out at the head of
            # every sequence that lies inside a pass.  A random window is absent two times in five.
            from itertools import product

            every = sorted({ref.canonical("".join(p)) for p in product("ACGT", repeat=5)})
            held = [every[i] for i in rng.permutation(len(every))[:300]]
            head = "".join(held[:254])
            assert len(head) < BODY - 100
            first = [head + _seq(rng, n - len(head)) if i in INSIDE else _seq(rng, n) for i, n in enumerate(lengths)]
        else:
            # held: the first 1300 windows of every sequence inside a pass, and every sequence across an edge but for its last
            # windows - in the order of the stream, so that 254 held windows in a row carry every counter
            first = [_seq(rng, n) for n in lengths]
            held, known = [], set()
            for i, s in enumerate(first):
                windows = ref.window_kmers(s, k)
                for km in windows[:1300] if i in INSIDE else windows[:max(len(windows) - 60, 0)]:
                    if km not in known:
                        known.add(km)
                        held.append(km)
        self.db = {km: 2 + i % 254 for i, km in enumerate(held)}
        # an N and a soft-masked stretch in the first batch (a k-mer of the database stays found in lower case)
        hurt = list(first[3])
        hurt[300] = "N"
        hurt[500:560] = [c.lower() for c in hurt[500:560]]
        first[3] = "".join(hurt)
        first[6] = first[6][:200] + "n" + first[6][201:]
        self.first = first
        # the second batch: the same sequences from the back, every other one as its reverse complement, but for two (their
        # k-mers stay at one copy); the heads of three of them once, twice and four times more (three, four and six copies);
        # and sequences of its own
        second = [ref.revcomp(s.upper()) if i % 2 else s for i, s in enumerate(first[::-1])]
        more = [first[0][:300]] + [first[4][:300]] * 2 + [first[7][:300]] * 4
        self.second = second[:5] + more + second[7:] + [_seq(rng, 700), "N" * 40, first[0][200:260].lower()]
        self.tally = ref.Tally(self.db)
        self.want = []  # per batch: (per_read, counts); self.state: the session behind it
        self.state = []
        for batch in (self.first, self.second):
            self.want.append(self.tally.add(batch, k))
            self.state.append((self.tally.hist.copy(), [self.tally.completeness(*c) for c in CUTS], self.tally.spectrum()))
        self.file = ref.database_bytes(self.db, k)


_CASES = {}


@pytest.fixture(scope="module")
def case():
    def get(k):
        if k not in _CASES:
            _CASES[k] = Case(k)
        return _CASES[k]

    yield get
    _CASES.clear()


@pytest.mark.parametrize("k", KS)
def test_the_batches_are_what_they_are_meant_to_be(gpu, case, k):
    c = case(k)
    for batch, (per_read, counts) in zip((c.first, c.second), c.want):
        stream_counts = _stream(counts, batch)
        clean = np.zeros(sum(len(s) for s in batch), dtype=np.uint8)
        at = 0
        for s in batch:
            for w, km in enumerate(ref.window_kmers(s, k)):
                clean[at + w] = km is not None
            at += len(s)
        stream_clean = _stream(clean, batch)
        passes = (stream_counts.size + PASS - 1) // PASS
        # not vacuous: with every hooked grid the pass loop and the sequence loops (four waves to a block) take a second trip
        assert passes >= PASSES and all(passes > s and len(batch) > 4 * s for s in SLOTS)
        for p in range(passes):
            here = stream_counts[p * PASS:(p + 1) * PASS][stream_clean[p * PASS:(p + 1) * PASS] > 0]
            # the first batch: absent windows and every counter in every pass; the second one's passes cut its sequences
            # elsewhere: absent windows in every pass, most counters in every full one
            if batch is c.first:
                assert set(here.tolist()) == {0} | set(range(2, 256)), (k, p)
            else:
                assert 0 in here and (p == passes - 1 or np.unique(here).size > 128), (k, p)
    assert len(c.first) == 23 and sum(len(s) + 1 for s in c.first) == STREAM
    assert sum(len(s) == 0 for s in c.first) >= 3 and sum(0 < len(s) < k for s in c.first) >= 2
    spec = c.state[1][2]
    assert k == 5 or (spec.sum(axis=1) > 0).all()  # every row of the copy spectrum is filled: 0, 1, 2, 3, 4 and more than four copies


def _run(gpu, database, c, copies, return_counts, slots):
    from trio_binning_amd import kmers

    what = f"k {c.k}, copies {copies}, return_counts {return_counts}, wave_slots {slots}"
    with database.query(copies=copies) as query:
        if slots:
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
        for batch, want, state in ((c.first, c.want[0], c.state[0]), (c.second, c.want[1], c.state[1]), (None, None, None), (c.first, c.want[0], c.state[0])):
            if batch is None:
                query.reset()
                assert int(query.histogram().sum()) == 0 and query.completeness() == (0, len(c.db)), what
                continue
            bases, offsets = kmers.pack_reads(batch)
            got = query.add(bases, offsets, 2, return_counts=return_counts)
            per_read, counts = got if return_counts else (got, None)
            assert per_read.dtype == np.uint64 and np.array_equal(per_read, want[0]), (what, np.flatnonzero((per_read != want[0]).any(axis=1))[:10])
            if return_counts:
                assert counts.dtype == np.uint8 and np.array_equal(counts, want[1]), (what, np.flatnonzero(counts != want[1])[:10])
            hist = query.histogram()
            assert np.array_equal(hist, state[0]), (what, np.flatnonzero(hist != state[0])[:10], hist[:4], state[0][:4])
            for cuts, answer in zip(CUTS, state[1]):
                assert query.completeness(*cuts) == answer, (what, cuts)
            if copies:
                assert np.array_equal(query.copy_spectrum(), state[2]), what


@pytest.mark.parametrize("return_counts", [False, True])
@pytest.mark.parametrize("copies", [False, True])
@pytest.mark.parametrize("k", KS)
def test_every_grid_against_the_reference(gpu, case, tmp_path, k, copies, return_counts):
    from trio_binning_amd import kmers

    c = case(k)
    path = tmp_path / "grid.tbkdb"
    path.write_bytes(c.file)
    with kmers.KmerDatabase.load(str(path)) as database:
        assert len(database) == len(c.db)
        for slots in (0,) + SLOTS:  # 0: the device's own grid
            _run(gpu, database, c, copies, return_counts, slots)


def test_the_hook_refuses_zero_and_null(gpu, case, tmp_path):
    from trio_binning_amd import _lib, kmers

    c = case(21)
    path = tmp_path / "grid.tbkdb"
    path.write_bytes(c.file)
    with kmers.KmerDatabase.load(str(path)) as database, database.query(copies=True) as query:
        assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, 3) == 0
        assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, 0) == _lib.TBK_ERR_INVALID
        assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(None, 3) == _lib.TBK_ERR_INVALID
        per_read, counts = query.add(*kmers.pack_reads(c.first), 2, return_counts=True)  # the session is as it was: it still runs
        assert np.array_equal(per_read, c.want[0][0]) and np.array_equal(counts, c.want[0][1])
        assert np.array_equal(query.histogram(), c.state[0][0]) and np.array_equal(query.copy_spectrum(), c.state[0][2])
