"""kmers.DatabaseQuery.pieces (tbk_kmerdb_query_pieces; kernels: csrc/tbk_pieces.hip behind csrc/tbk_screen.hip's lookup) against
tests/pieces_ref.py, record for record and byte for byte.  The batch is test_gpu_screen_evidence.Case's - runs that end at window
2047 and begin at 4096, a run over a word edge, held windows at a sequence's first and last window, windows k and k + 1 apart (the
two runs of k bases are the tie of `longest`), an N inside a run, lower case, a run over a pass edge, a sequence held throughout
that is longer than two passes, a sequence that ends covered before one that begins covered, sequences of 0, k - 1, k and k + 1
bases - with four sequences behind it: one that ends uncovered, one that begins and ends uncovered, one of N only and one that
begins uncovered, so that only the separators keep four uncovered pieces apart.  Everything is integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import db_query_ref as ref
import pieces_ref as pr
import screen_ref as sr
from test_gpu_screen_evidence import COUNTERS, KS, PASS, RANGES, Case, _same_state, _seq, _state, load  # noqa: F401  (load: a fixture)

pytestmark = pytest.mark.gpu

SIDES = ("covered", "uncovered")
WHICH = ("all", "longest")
ALL_N = 37


def min_lengths(k):
    return (0, 1, k, k + 1, 2 * k, 1 << 40)


class PiecesCase:
    """Case(k)'s batch and the four sequences behind it, with the reference's covered masks and runs per range and database"""

    def __init__(self, k):
        from trio_binning_amd import kmers

        self.case = c = Case(k)
        self.k = k
        rng = np.random.default_rng(2900 + k)

        def open_ended(first, last):
            """a sequence of 40 to 69 bases whose first and / or last base no window of the solid database covers, whatever the range
            (nor of the full one from k = 21 on; below that its k-mers seen once are all over a random sequence)"""
            for _ in range(2000):
                s = _seq(rng, int(rng.integers(40, 70)))
                mask = pr.covered_mask(sr.window_counters(c.full_db if k >= 21 else c.db, [s], k)[0], len(s), k, 1, 255)
                if not (first and mask[0]) and not (last and mask[-1]):
                    return s
            raise AssertionError("no sequence with uncovered ends for k {}".format(k))

        self.extras = [open_ended(False, True), open_ended(True, True), "N" * ALL_N, open_ended(True, False)]
        self.first_extra = len(c.batch)
        self.batch = c.batch + self.extras
        self.lengths = [len(s) for s in self.batch]
        self.packed = kmers.pack_reads(self.batch)
        self.counters = {full: c.counters[full] + sr.window_counters(c.full_db if full else c.db, self.extras, k) for full in (False, True)}
        self.found = {}

    def runs(self, min_count, max_count, full, side):
        """per sequence, its runs on `side` before min_length and which"""
        key = (min_count, max_count, full, side)
        if key not in self.found:
            m = sr.threshold(min_count, 1 if full else 2)
            for s in SIDES:
                self.found[key[:3] + (s,)] = []
            for counters, n in zip(self.counters[full], self.lengths):
                mask = pr.covered_mask(counters, n, self.k, m, max_count)
                for s in SIDES:
                    self.found[key[:3] + (s,)].append(pr.runs(mask, s == "covered"))
        return self.found[key]

    def want(self, min_count, max_count, full, side, which, min_length):
        return [(r, f, e) for r, found in enumerate(self.runs(min_count, max_count, full, side)) for f, e in pr.select(found, which, min_length)]

    def evidence(self, min_count, max_count, full):
        head = self.case.want(min_count, max_count, full)
        tail = sr.as_array(sr.records(self.counters[full][self.first_extra:], self.lengths[self.first_extra:], self.k, min_count, max_count, 1 if full else 2))
        return np.concatenate([head, tail])


_CASES = {}


@pytest.fixture(scope="module")
def case(gpu):
    def get(k):
        if k not in _CASES:
            _CASES[k] = PiecesCase(k)
        return _CASES[k]

    yield get
    _CASES.clear()


def _check(query, c, min_count, max_count, full, side, which, min_length):
    from trio_binning_amd import kmers

    want = pr.as_array(c.want(min_count, max_count, full, side, which, min_length))
    got = query.pieces(*c.packed, min_count, max_count, side, which, min_length)
    what = "k {}, range [{}, {}], full {}, {} {}, min_length {}".format(c.k, min_count, max_count, full, side, which, min_length)
    assert got.dtype == kmers.READ_PIECE == pr.READ_PIECE, what
    assert got.tobytes() == want.tobytes(), (what, pr.first_difference(got, want))
    return want


# ---- 1. every k, both databases, every range, both sides, both selections, every min_length -----------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_rule_against_the_reference(case, load, k):
    c = case(k)
    with load(c.case.file).query(copies=True) as query:
        _check(query, c, 1, 255, False, "covered", "all", 1)  # before anything was added
        query.add(*c.packed)
        before = _state(query)
        for min_count, max_count in RANGES:
            for side in SIDES:
                for which in WHICH:
                    for min_length in min_lengths(k):
                        _check(query, c, min_count, max_count, False, side, which, min_length)
            # the evidence of the same lookup pass is the evidence call's, byte for byte
            got, evidence = query.pieces(*c.packed, min_count, max_count, "uncovered", "longest", k, evidence=True)
            assert evidence.tobytes() == query.evidence(*c.packed, min_count, max_count).tobytes() == c.evidence(min_count, max_count, False).tobytes()
            assert got.tobytes() == pr.as_array(c.want(min_count, max_count, False, "uncovered", "longest", k)).tobytes()
        assert _same_state(_state(query), before)  # the call only reads the session
    with load(c.case.full_file).query() as query:  # a session without copies, on a full database: min_count 1 counts presence
        before = _state(query)
        for min_count, max_count in RANGES:
            for side in SIDES:
                for which in WHICH:
                    for min_length in min_lengths(k):
                        _check(query, c, min_count, max_count, True, side, which, min_length)
            got, evidence = query.pieces(*c.packed, min_count, max_count, evidence=True)
            assert evidence.tobytes() == query.evidence(*c.packed, min_count, max_count).tobytes() == c.evidence(min_count, max_count, True).tobytes()
        assert _same_state(_state(query), before)
    not_vacuous(c)


def not_vacuous(c):
    """the reference's own answers hold the placements that the batch was built for (no device is asked)"""
    k, L = c.k, c.lengths
    covered, uncovered = c.want(1, 255, False, "covered", "all", 1), c.want(1, 255, False, "uncovered", "all", 1)
    assert not c.want(1, 1, False, "covered", "all", 1)  # empty after a solid database's floor: everything is one uncovered piece
    assert c.want(1, 1, False, "uncovered", "all", 1) == [(r, 0, n) for r, n in enumerate(L) if n]
    assert c.want(10, 20, False, "covered", "all", 1) != covered and c.want(1, 1, True, "covered", "all", 1)
    # the identities with the evidence: stretches, covered, longest
    evidence = c.evidence(1, 255, False)
    for r in range(len(L)):
        mine = [e - f for read, f, e in covered if read == r]
        assert (len(mine), sum(mine), max(mine + [0])) == (int(evidence[r]["stretches"]), int(evidence[r]["covered"]), int(evidence[r]["longest"]))
    # the four sequences at the end: u1 ends uncovered, u2 begins and ends uncovered, the N's are one piece, u3 begins uncovered -
    # four pieces that only the separators keep apart, for every range
    x = c.first_extra
    for full in (False, True) if k >= 21 else (False,):
        for min_count, max_count in RANGES:
            mine = c.want(min_count, max_count, full, "uncovered", "all", 1)
            assert [p for p in mine if p[0] == x][-1][2] == L[x] and [p for p in mine if p[0] == x + 1][0][1] == 0
            assert [p for p in mine if p[0] == x + 1][-1][2] == L[x + 1] and [p for p in mine if p[0] == x + 2] == [(x + 2, 0, ALL_N)]
            assert [p for p in mine if p[0] == x + 3][0][1] == 0
            assert not [p for p in c.want(min_count, max_count, full, "covered", "all", 1) if p[0] == x + 2]
    # sequences of 0 and k - 1 bases: no piece of the empty one, one whole uncovered piece and no covered one of the other
    assert L[1] == 0 and L[2] == k - 1 and not [p for p in covered + uncovered if p[0] == 1] and not [p for p in covered if p[0] == 2]
    assert [p for p in uncovered if p[0] == 2] == ([(2, 0, k - 1)] if k > 1 else [])
    # min_length and longest leave pieces out, and 2^40 leaves none
    assert 0 < len(c.want(1, 255, False, "covered", "all", k + 1)) < len(covered) and not c.want(1, 255, False, "uncovered", "all", 1 << 40)
    longest = c.want(1, 255, False, "covered", "longest", 1)
    assert len(longest) == len({p[0] for p in covered}) < len(covered)
    if k >= 21:  # the placements are the ones planted (below that every k-mer recurs all over the genome)
        first = [(f, e) for r, f, e in covered if r == 0]
        assert (200, 200 + 2 * k) in first and (400, 400 + k) in first and (401 + k, 401 + 2 * k) in first  # k apart: one piece; k + 1 apart: two
        assert (PASS - 18, PASS - 1 + k) in first and (2 * PASS, 2 * PASS + 14 + k) in first  # ends at window 2047, begins at 4096
        assert (1000, c.case.n_at) in first and (c.case.n_at + 1, 1000 + 4 * k) in first  # the N splits a run
        assert (1500, 1540 + k) in first and longest[0] == (0, 1500, 1540 + k) and first[-1] == (4500 - k, 4500)
        # the tie of `longest`: with the run in lower case and the others out of the way the runs of k bases are the longest, and the first wins
        tie = [p for p in c.want(1, 255, False, "covered", "all", 1) if p[0] == 0 and p[2] - p[1] == k]
        assert len(tie) > 2 and pr.select([(f, e) for _, f, e in tie], "longest") == [tie[0][1:]]
        assert (5, 300 - k, 300) in covered and (6, 0, k) in covered  # ends covered before one that begins covered
        assert [p for p in covered if p[0] == c.case.whole] == [(c.case.whole, 0, L[c.case.whole])] and L[c.case.whole] > 2 * PASS
        assert [p for p in uncovered if p[0] == c.case.whole] == []
        assert [p for p in covered if p[0] == c.case.straddler] == [(c.case.straddler, c.case.edge - 3, c.case.edge + 2 + k)]  # over a pass edge


@pytest.mark.parametrize("k", (21, 32))
def test_the_first_of_equal_pieces_is_the_longest(gpu, load, k):
    """two, three and four runs of exactly k bases, nothing longer: the first wins, on either side"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(50 + k)
    genome = _seq(rng, 600)
    reads = [genome[:200], genome[200:400], genome[400:600]]
    held = [10, 100, 210, 260, 330, 400 + k, 400 + 3 * k, 400 + 5 * k] + list(range(400 + min(6 * k, 200 - k), 600 - k + 1))  # (held through from 6k to the end)
    db = {ref.canonical(genome[w:w + k]): 7 for w in held}
    want = pr.pieces(db, reads, k, which="longest")
    assert want[:2] == [(0, 10, 10 + k), (1, 10, 10 + k)] and want[2][2] == 200 and want[2][2] - want[2][1] > k  # (the third read's tail is longer)
    gaps = pr.pieces(db, reads, k, side="uncovered", which="longest")
    assert gaps[2] == (2, 0, k) and len([p for p in pr.pieces(db, reads, k, side="uncovered") if p[0] == 2 and p[2] - p[1] == k]) == 3
    with load(ref.database_bytes(db, k)).query() as query:
        assert query.pieces(*kmers.pack_reads(reads), which="longest").tobytes() == pr.as_array(want).tobytes()
        assert query.pieces(*kmers.pack_reads(reads), side="uncovered", which="longest").tobytes() == pr.as_array(gaps).tobytes()


# ---- 2. the later trips of the strided loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 21))
def test_small_grids_take_later_trips(gpu, case, load, k):
    """with one, two and three wave slots - as many one-wave blocks - the lookup strides over the seven passes, the side kernel over
    their 448 bitmap words and, for k = 4, the kernel of the per-read keys over more than 192 pieces; the separators' kernel strides
    over a second batch's 500 short sequences"""
    from trio_binning_amd import kmers

    c = case(k)
    assert c.case.stream > 6 * PASS
    assert k != 4 or len(c.want(1, 255, False, "covered", "all", 1)) > 3 * 64
    rng = np.random.default_rng(77 + k)
    shorts = [_seq(rng, int(n)) for n in rng.integers(0, 3 * k, 500)]
    counters, lengths = sr.window_counters(c.case.db, shorts, k), [len(s) for s in shorts]
    packed = kmers.pack_reads(shorts)
    with load(c.case.file).query() as query:
        for slots in (1, 2, 3):
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            for side in SIDES:
                for which in WHICH:
                    _check(query, c, 1, 255, False, side, which, 1)
                    _check(query, c, 10, 20, False, side, which, k + 1)
                    want = pr.as_array(pr.pieces_from(counters, lengths, k, 1, 255, side, which, 2))
                    got = query.pieces(*packed, 1, 255, side, which, 2)
                    assert got.tobytes() == want.tobytes(), (slots, side, which, pr.first_difference(got, want))
            got, evidence = query.pieces(*c.packed, evidence=True)
            assert evidence.tobytes() == c.evidence(1, 255, False).tobytes()
    assert len(pr.pieces_from(counters, lengths, k, 1, 255, "uncovered", "all", 2)) > 3 * 64


def _tiled(unit_pieces, unit_reads, tiles):
    """the pieces of `tiles` copies of a batch of unit_reads sequences, from the pieces of one copy"""
    unit = pr.as_array(unit_pieces)
    out = np.tile(unit, tiles)
    out["read"] += np.repeat(np.arange(tiles, dtype=np.uint64) * np.uint64(unit_reads), unit.size)
    return out


def test_the_grid_of_a_whole_device_takes_a_second_trip_over_reads_and_pieces(gpu, load):
    """the kernels that stride over sequences (the separators) and over pieces (the per-read keys) start min(ceil(n / 64),
    wave_slots) one-wave blocks, and wave_slots is 32 x compute units - 8192 on the 256 of an MI355X: from 64 x 8192 + 1 = 524289
    items on their loops take a second trip.  600 copies of 1000 short sequences, the uncovered side: a piece per sequence and more.
    A sequence's pieces depend on nothing but the sequence, so the reference is that of one copy, repeated."""
    k, unit_reads, tiles = 5, 1000, 600
    rng = np.random.default_rng(29)
    unit = [_seq(rng, int(n)) for n in rng.integers(1, 11, unit_reads)]
    unit[7], unit[990] = "ACNTA", "ACGTACGTAC"
    db = {ref.canonical(km): COUNTERS[i % 6] for i, km in enumerate(sorted({s[:k] for s in unit[::2] if len(s) >= k and "N" not in s[:k]}))}
    assert unit_reads * tiles > 64 * 8192
    lengths = np.tile(np.array([len(s) for s in unit], dtype=np.uint64), tiles)
    offsets = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lengths, dtype=np.uint64)])
    bases = np.tile(np.frombuffer("".join(unit).encode(), dtype=np.uint8), tiles)
    with load(ref.database_bytes(db, k)).query() as query:
        for side, which, min_length in (("uncovered", "longest", 1), ("uncovered", "all", 2), ("covered", "longest", 1)):
            one = pr.pieces(db, unit, k, 5, 127, side, which, min_length)
            want = _tiled(one, unit_reads, tiles)
            assert (side, which) != ("uncovered", "longest") or want.size > 64 * 8192  # (the keys' kernel strides over these and the ones left out)
            assert 0 < len(one) and len({p[0] for p in one}) < unit_reads
            got = query.pieces(bases, offsets, 5, 127, side, which, min_length)
            assert got.size == want.size and got.tobytes() == want.tobytes(), (side, which, np.flatnonzero(got != want)[:3])


def test_the_grid_of_a_whole_device_takes_a_second_trip_over_words(gpu, load):
    """the side kernel strides over the bitmap's 32-bit words, 64 to a one-wave block: from 524289 words - 16.8 M stream positions -
    on it takes a second trip.  4000 copies of one sequence of 4200 bases with a handful of held windows."""
    k, n, tiles = 21, 4200, 4000
    rng = np.random.default_rng(31)
    s = _seq(rng, n)
    db = {ref.canonical(s[w:w + k]): 9 for w in (0, 31, 32, 33, 700, 2047, 2048, 3000, 3000 + k, n - k)}
    assert tiles * (n + 1) > 32 * 64 * 8192
    bases = np.tile(np.frombuffer(s.encode(), dtype=np.uint8), tiles)
    offsets = np.arange(tiles + 1, dtype=np.uint64) * np.uint64(n)
    with load(ref.database_bytes(db, k)).query() as query:
        for side in SIDES:
            one = pr.pieces(db, [s], k, side=side)
            assert len(one) == (6 if side == "covered" else 5)  # every copy ends covered before one that begins covered
            want = _tiled(one, 1, tiles)
            got = query.pieces(bases, offsets, side=side)
            assert got.size == want.size and got.tobytes() == want.tobytes(), (side, np.flatnonzero(got != want)[:3])


# ---- 3. small databases and batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 21))
def test_an_empty_database(load, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(80 + k)
    sequences = [_seq(rng, 2100), "", _seq(rng, k) + "N" + _seq(rng, 2 * k), _seq(rng, k)]
    with load(ref.database_bytes({}, k)).query() as query:
        assert query.pieces(*kmers.pack_reads(sequences)).size == 0 and query.pieces(*kmers.pack_reads(sequences), which="longest").size == 0
        got, evidence = query.pieces(*kmers.pack_reads(sequences), side="uncovered", evidence=True)
        assert got.tobytes() == pr.as_array([(0, 0, 2100), (2, 0, 3 * k + 1), (3, 0, k)]).tobytes() == pr.as_array(pr.pieces({}, sequences, k, side="uncovered")).tobytes()
        assert evidence.tobytes() == sr.as_array(sr.evidence({}, sequences, k)).tobytes()
        assert query.pieces(*kmers.pack_reads(sequences), side="uncovered", min_length=2101).size == 0


@pytest.mark.parametrize("k", (2, 21, 32))
def test_a_database_of_one_entry(load, k):
    """one entry: the directory has no prefix bits"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(90 + k)
    s = _seq(rng, 3 * k)
    db = {ref.canonical(s[k:2 * k]): 5}
    sequences = [s, s[k:2 * k], ref.revcomp(s[k:2 * k]).lower(), s[k + 1:2 * k]]
    with load(ref.database_bytes(db, k)).query() as query:
        for min_count, max_count in ((1, 255), (5, 5), (6, 255), (1, 4)):
            for side in SIDES:
                for which in WHICH:
                    got = query.pieces(*kmers.pack_reads(sequences), min_count, max_count, side, which)
                    want = pr.as_array(pr.pieces(db, sequences, k, min_count, max_count, side, which))
                    assert got.tobytes() == want.tobytes(), pr.first_difference(got, want)
    if k > 2:
        assert pr.pieces(db, sequences, k) == [(0, k, 2 * k), (1, 0, k), (2, 0, k)]
        assert pr.pieces(db, sequences, k, side="uncovered") == [(0, 0, k), (0, 2 * k, 3 * k), (3, 0, k - 1)]


def test_batches_without_a_window_or_a_read(gpu, case, load):
    from trio_binning_amd import kmers

    c = case(21)
    with load(c.case.file).query() as query:
        reads = ["ACGT", "", "A" * 20]
        got, evidence = query.pieces(*kmers.pack_reads(reads), evidence=True)
        assert got.dtype == kmers.READ_PIECE and got.size == 0 and evidence.dtype == kmers.READ_EVIDENCE and evidence.tobytes() == bytes(120)
        assert query.pieces(*kmers.pack_reads(reads), side="uncovered").tobytes() == pr.as_array([(0, 0, 4), (2, 0, 20)]).tobytes()
        assert query.pieces(*kmers.pack_reads(["N" * 30]), side="uncovered").tobytes() == pr.as_array([(0, 0, 30)]).tobytes()
        assert query.pieces(*kmers.pack_reads(["", "", ""]), side="uncovered").size == 0  # not a base in the batch
        for side in SIDES:  # n_reads = 0
            got, evidence = query.pieces(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), side=side, evidence=True)
            assert got.size == 0 and got.dtype == kmers.READ_PIECE and evidence.size == 0
        ptr, count = C.c_void_p(77), C.c_uint64(77)
        assert gpu.lib.tbk_kmerdb_query_pieces(query._h, None, np.zeros(1, dtype=np.uint64).ctypes.data, 0, 1, 255, 1, 1, 0, None, C.byref(ptr), C.byref(count)) == 0
        assert (ptr.value, count.value) == (None, 0)  # no piece: NULL
        _check(query, c, 1, 255, False, "covered", "all", 1)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_session_usable(gpu, case, load):
    from trio_binning_amd import _lib

    c = case(21)
    bases, offsets = c.packed
    n = offsets.size - 1
    with load(c.case.file).query(copies=True) as query:
        query.add(bases, offsets)
        before = _state(query)
        evidence = np.full(n * 5, 77, dtype=np.uint64)
        ptr, count = C.c_void_p(77), C.c_uint64(77)

        def call(q, min_count, max_count, side, which, pieces=C.byref(ptr), n_pieces=C.byref(count), offs=offsets):
            return gpu.lib.tbk_kmerdb_query_pieces(q, bases.ctypes.data, offs.ctypes.data, n, min_count, max_count, side, which, 1, evidence.ctypes.data,
                                                   pieces, n_pieces)

        for min_count, max_count, side, which, word in ((0, 255, 0, 0, "min_count"), (256, 256, 0, 0, "min_count"), (2, 1, 0, 0, "max_count"),
                                                        (2, 256, 1, 1, "max_count"), (255, 254, 0, 0, "max_count"), (1, 255, 2, 0, "side"),
                                                        (1, 255, 0xFFFFFFFF, 0, "side"), (1, 255, 0, 2, "which"), (1, 255, 1, 7, "which")):
            assert call(query._h, min_count, max_count, side, which) == _lib.TBK_ERR_INVALID, (min_count, max_count, side, which)
            assert word in _lib.last_error() and (evidence == 77).all() and (ptr.value, count.value) == (77, 77)  # nothing is written
        assert call(None, 1, 255, 0, 0) == _lib.TBK_ERR_INVALID and call(query._h, 1, 255, 0, 0, pieces=None) == _lib.TBK_ERR_INVALID
        assert call(query._h, 1, 255, 0, 0, n_pieces=None) == _lib.TBK_ERR_INVALID and "NULL" in _lib.last_error()
        # a sequence of 2^32 bases, by its offsets alone: refused before a byte of it is read
        huge = offsets.copy()
        huge[1:] += np.uint64(1 << 32)
        assert call(query._h, 1, 255, 0, 0, offs=huge) == _lib.TBK_ERR_INVALID and "2^32" in _lib.last_error()
        assert (evidence == 77).all() and (ptr.value, count.value) == (77, 77)
        for args in ((0, 255), (256, 256), (2, 1), (2, 256), (-1, 255), (2, -5), (1 << 32, 255), (2, 1 << 32), (1, 255, "both"), (1, 255, "covered", "first"),
                     (1, 255, "covered", "all", -1), (1, 255, "covered", "all", 1 << 64), (1, 255, 0), (1, 255, "covered", 1)):
            with pytest.raises(ValueError):
                query.pieces(bases, offsets, *args)
        assert _same_state(_state(query), before)
        _check(query, c, 1, 255, False, "covered", "all", 1)
        _check(query, c, 255, 255, False, "uncovered", "longest", 21)
