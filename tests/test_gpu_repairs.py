"""kmers.DatabaseQuery.repairs (tbk_kmerdb_query_repairs; kernels: csrc/tbk_repair.hip) against tests/repair_ref.py, record for
record and byte for byte, pad included.  One batch per k holds every placement at which the kernels can go wrong: stretches over
the pass edges at stream positions 2048 and 4096, an edit neighbourhood over an edge that its stretch does not touch, errors at
both ends of a sequence, beside an N and in lower case, errors closer than k and between k and 2k apart, extra and missing bases
in homopolymer runs of 2 to 9, sequences shorter than k, empty ones, one of exactly k bases, a stretch at a sequence's end before
one at the next one's start, a reverse-complemented copy and k-mers that are their own reverse complement.
tests/test_host_repair_ref.py holds the reference to a brute force and to hand-worked records.  Everything is integers: every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
import repair_ref as rr

pytestmark = pytest.mark.gpu

PASS = 2048
KS = (1, 2, 4, 5, 21, 31, 32)
COUNTERS = (2, 5, 10, 20, 127, 255)  # with min_count 10 the k-mers that the database holds with 2 or 5 are broken
LONG = 4500  # the first sequence: its windows cross the pass edges at 2048 and 4096
FULL = b"TBKKMFB1"  # a full database's magic: it also holds the k-mers seen once (floor 1)


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _other(c):
    return "ACGT"[("ACGT".index(c.upper()) + 1) % 4]


def _own_reverse_complement(k):
    half = "ACGGTCAATCGATTGC"[:k // 2]
    return half + ref.revcomp(half)


def _file(db, k, full):
    if not full:
        return ref.database_bytes(db, k)
    ranks = np.array(sorted(ref.lex_rank(km) for km in db), dtype=np.uint64)
    by_rank = {ref.lex_rank(km): c for km, c in db.items()}
    counts = np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[0] = counts.size
    return kf.file_bytes(k, ranks, counts, hist, reads=1, bases=k, magic=FULL)


def _edited(true, edits):
    """`true` with (pos, kind, base) edits in its own coordinates, applied from the right"""
    s = list(true)
    for pos, kind, base in sorted(set(edits), reverse=True):
        if kind == rr.SUB:
            s[pos] = base
        elif kind == rr.DEL:
            del s[pos]
        else:
            s.insert(pos, base)
    return "".join(s)


class Case:
    """One genome, a solid and a full database of it, and one batch of erroneous copies for one k, with the reference's answers."""

    def __init__(self, k):
        from trio_binning_amd import kmers

        rng = np.random.default_rng(2400 + k)
        self.k = k
        genome = list(_seq(rng, 9000))
        self.runs = []
        for i in range(16):  # runs of 2 .. 9 equal bases, two of each length, 100 apart
            pos, n = 200 + 100 * i, 2 + i // 2
            base = next(c for c in "ACGT" if c != genome[pos - 1] and c != genome[pos + n])
            genome[pos:pos + n] = base * n
            self.runs.append((pos, n, base))
        if k == 32:  # (at k = 2 and 4 a random sequence holds them by itself)
            for at in (2150, 3000, 4200):
                genome[at:at + k] = _own_reverse_complement(k)
        genome = "".join(genome)
        windows = ref.window_kmers(genome, k)
        held = sorted({km for i, km in enumerate(windows) if not 6000 <= i < 6300})  # an absent region: long stretches
        dropped = []
        if k <= 5:  # nearly every small k-mer occurs somewhere: drop some, or nothing is broken
            held, dropped = [km for i, km in enumerate(held) if i % 3 != 1], [km for i, km in enumerate(held) if i % 3 == 1]
        # from k = 21 on one k-mer in 450 has a counter below 10 (more would bury the planted errors under stretches at min_count 10)
        self.db = {km: COUNTERS[h % 6 if k <= 5 else h % 2 if h < 2 else 2 + h % 4] for km in held for h in [(ref.lex_rank(km) * 7 + len(km)) % 907]}
        once = dropped[::2] + [km for km in windows[6000:6150] if km not in self.db]
        self.full_db = dict(self.db, **{km: 1 for km in once})  # the same, and some k-mers seen once

        true = genome[:LONG]
        edits = [(p, rr.SUB, _other(true[p])) for p in {0, 1, k - 2, k - 1, LONG - k, LONG - 2, LONG - 1, 100} if 0 <= p < LONG]
        for i, (pos, n, base) in enumerate(self.runs):  # an extra base in the first run of each length, a missing one in the second
            edits.append((pos, rr.DEL if i & 1 else rr.INS, base))
        self.straddling = (PASS - 1 + k // 2, 2 * PASS + k // 2)  # a substitution here: a stretch over a pass edge (k >= 2)
        for p in self.straddling + (1902, 2300, 2300 + max(1, k // 2), 2600, 2600 + k + k // 2):  # two closer than k, two between k and 2k apart
            edits.append((p, rr.SUB, _other(true[p])))
        first = list(_edited(true, edits))
        assert len(first) == LONG  # (the runs' extra and missing bases alternate: the coordinates past them are the genome's)
        first[1900] = "N"  # two bases before the error at 1902
        first[95:106] = [c.lower() for c in first[95:106]]  # lower case at and around the error at 100
        short = [genome[10:10 + max(k - 1, 0)], "", genome[40:40 + k // 2]]
        exactly_k = _edited(genome[5000:5000 + k], [(k // 2, rr.SUB, _other(genome[5000 + k // 2]))])
        ends = _edited(genome[4600:4900], [(299, rr.SUB, _other(genome[4899]))])  # ends in a stretch ...
        begins = _edited(genome[4900:5200], [(0, rr.SUB, _other(genome[4900]))])  # ... and the next one begins with one
        self.batch = ["".join(first)] + short + [exactly_k, ends, begins, ref.revcomp("".join(first[100:1700]).upper())] + short[::-1]
        # a neighbourhood over the pass edge at 8192 whose stretch ends two positions below it
        start = sum(len(s) + 1 for s in self.batch)
        self.beside = 4 * PASS - 2 - start
        assert 1340 < self.beside < 2200  # (behind the absent region and its last windows)
        self.batch += [_edited(genome[5000:7300], [(self.beside, rr.SUB, _other(genome[5000 + self.beside]))]), genome[2000:5000],
                       "n" + genome[6701:9000].lower(), genome[:1500]]
        self.beside_read = len(self.batch) - 4
        self.stream = sum(len(s) + 1 for s in self.batch)
        assert self.stream > 7 * PASS  # a grid of three waves takes a third trip over the passes
        if k in (2, 4, 32):
            assert any(km == ref.revcomp(km) for km in self.db)
        self.file, self.full_file = _file(self.db, k, False), _file(self.full_db, k, True)
        self.packed = kmers.pack_reads(self.batch)
        self.evaluated = {}

    def want(self, min_count, min_support, full=False):
        """the reference's records; what does not depend on min_support is computed once per (min_count, database)"""
        key = (min_count, full)
        if key not in self.evaluated:
            self.evaluated[key] = rr.evaluate(self.full_db if full else self.db, self.batch, self.k, min_count, floor=1 if full else 2)
        return rr.as_array(rr.records(self.evaluated[key], self.k, min_support))


_CASES = {}


@pytest.fixture(scope="module")
def case(gpu):
    def get(k):
        if k not in _CASES:
            _CASES[k] = Case(k)
        return _CASES[k]

    yield get
    _CASES.clear()


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


def _state(query):
    return (query.histogram(), query.completeness(), query.completeness(10, 200)) + ((query.copy_spectrum(),) if query.copies else ())


def _same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check(query, c, min_count, min_support, full=False):
    from trio_binning_amd import kmers

    want = c.want(min_count, min_support, full)
    before = _state(query)
    got = query.repairs(*c.packed, min_count, min_support)
    what = "k {}, min_count {}, min_support {}, full {}".format(c.k, min_count, min_support, full)
    assert got.dtype == kmers.REPAIR == rr.REPAIR, what
    assert got.tobytes() == want.tobytes(), (what, rr.first_difference(got, want))
    assert _same_state(_state(query), before), what  # the call only reads the session
    return want


# ---- 1. every k, every threshold, every support -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_parameter_against_the_reference(case, load, k):
    c = case(k)
    with load(c.file).query(copies=True) as query:
        _check(query, c, 2, 1)  # before anything was added
        query.add(*c.packed)
        for min_count in (2, 10):
            for min_support in sorted({1, k // 2 + 1, k}):
                _check(query, c, min_count, min_support)
        _check(query, c, 1, 1)  # a solid database's threshold is 2 all the same
    plain = c.want(2, 1)
    assert c.want(10, 1).tobytes() != plain.tobytes()  # counters below 10 are broken with min_count 10
    with load(c.full_file).query() as query:  # a session without copies, on a full database: min_count 1 counts presence
        for min_support in sorted({1, k}):
            _check(query, c, 1, min_support, full=True)
        assert _check(query, c, 2, 1, full=True).tobytes() != c.want(1, 1, full=True).tobytes()
    # not vacuous, on the reference's answer.  `kind` names the smallest accepted edit, and among the few k-mers of k <= 2 a
    # substitution is accepted wherever anything is (at k = 1 nothing else has a window to vouch for it): all five kinds from k = 4 on.
    kinds = {int(v) for v in plain["kind"]}
    assert kinds == {rr.NONE, rr.SUB, rr.DEL, rr.INS, rr.LONG} if k >= 4 else kinds >= {rr.SUB, rr.LONG}, kinds
    assert int(plain["accepted"].max()) > 1
    if k > 1:
        assert ((plain["kind"] >= rr.SUB) & (plain["kind"] <= rr.INS) & (plain["support"] < k)).any()
    if k >= 21:  # (below that the stretches are those of the k-mers that were dropped, thousands of them, wherever they fall)
        last = plain["first"] + plain["windows"] - 1
        for edge in (PASS, 2 * PASS):  # a stretch of the first sequence over each pass edge
            assert ((plain["read"] == 0) & (plain["first"] < edge) & (last >= edge)).any(), edge
        # the stretch beside the fourth edge ends below it and its neighbourhood reaches over it
        at = sum(len(s) + 1 for s in c.batch[:c.beside_read])
        mine = plain[(plain["read"] == c.beside_read) & (plain["first"] + plain["windows"] - 1 == c.beside)]
        assert mine.size == 1 and at + c.beside == 4 * PASS - 2 and at + int(mine["first"][0]) + 2 * k - 2 >= 4 * PASS
        assert int(mine["accepted"][0]) == 1 and int(mine["kind"][0]) == rr.SUB
    reads = {int(v) for v in plain["read"]}
    assert 0 in reads and len(reads) >= 4 and np.all(np.diff(plain["read"].astype(np.int64)) >= 0)


# ---- 2. the later trips of both strided loops ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 21))
def test_small_grids_take_later_trips(gpu, case, load, k):
    c = case(k)
    assert len(c.want(2, 1)) > 3 * 3 and c.stream > 7 * PASS  # a fourth trip over the stretches, a third over the passes
    with load(c.file).query() as query:
        for slots in (1, 2, 3):
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            _check(query, c, 2, 1)
            _check(query, c, 10, k // 2 + 1)


# ---- 3. small databases and batches ---------------------------------------------------------------------------------------------------
def _small(load, db, k, sequences, min_count=2, min_support=1):
    from trio_binning_amd import kmers

    with load(ref.database_bytes(db, k)).query() as query:
        before = _state(query)
        got = query.repairs(*kmers.pack_reads(sequences), min_count, min_support)
        want = rr.as_array(rr.repairs(db, sequences, k, min_count, min_support))
        assert got.tobytes() == want.tobytes(), rr.first_difference(got, want)
        assert _same_state(_state(query), before)
        return got


@pytest.mark.parametrize("k", (1, 5, 21))
def test_an_empty_database(load, k):
    rng = np.random.default_rng(80 + k)
    sequences = [_seq(rng, 2100), "", _seq(rng, k) + "N" + _seq(rng, 2 * k), _seq(rng, k)]
    got = _small(load, {}, k, sequences)  # every clean window is broken and nothing is accepted
    assert got.size == 4 and not got["accepted"].any() and not got["pos"].any()
    assert [int(v) for v in got["windows"]] == [2100 - k + 1, 1, k + 1, 1] and [int(v) for v in got["kind"]] == [rr.LONG, rr.NONE, rr.LONG, rr.NONE]


@pytest.mark.parametrize("k", (2, 21, 32))
def test_a_database_of_one_entry(load, k):
    """one entry: the directory has no prefix bits"""
    rng = np.random.default_rng(90 + k)
    s = _seq(rng, 3 * k)
    db = {ref.canonical(s[k:2 * k]): 5}
    got = _small(load, db, k, [s, s[k:2 * k], ref.revcomp(s[k:2 * k]).lower(), _other(s[k]) + s[k + 1:2 * k]])
    if k > 2:  # the windows of s before and behind the entry's, and the last sequence, which one substitution turns into it
        assert [int(v) for v in got["read"]] == [0, 0, 3]
        assert (int(got[2]["kind"]), int(got[2]["pos"]), chr(int(got[2]["base"])), int(got[2]["support"])) == (rr.SUB, 0, s[k], 1)


def test_a_batch_without_a_stretch(gpu, case, load):
    from trio_binning_amd import kmers

    c = case(21)
    with load(c.file).query() as query:
        for sequences in ([c.batch[-1], c.batch[-3]], ["ACGT", "", "A" * 20], ["NNNNNNNNNNNNNNNNNNNNNNNNNNNNNN"]):
            got = query.repairs(*kmers.pack_reads(sequences))
            assert got.size == 0 and got.dtype == kmers.REPAIR
        got = query.repairs(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        assert got.size == 0
        ptr, count = C.c_void_p(0x1234), C.c_uint64(77)
        assert gpu.lib.tbk_kmerdb_query_repairs(query._h, None, np.zeros(1, dtype=np.uint64).ctypes.data, 0, 2, 1, C.byref(ptr), C.byref(count)) == 0
        assert ptr.value is None and count.value == 0  # NULL when there is no stretch


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_usable(gpu, case, load):
    from trio_binning_amd import _lib

    c = case(21)
    bases, offsets = c.packed
    n = offsets.size - 1
    with load(c.file).query(copies=True) as query:
        query.add(bases, offsets)
        before = _state(query)
        for min_count, min_support, word in ((0, 1, "min_count"), (256, 1, "min_count"), (2, 0, "min_support"), (2, 33, "min_support")):
            ptr, count = C.c_void_p(0x1234), C.c_uint64(77)
            assert gpu.lib.tbk_kmerdb_query_repairs(query._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, min_support, C.byref(ptr),
                                                    C.byref(count)) == _lib.TBK_ERR_INVALID, (min_count, min_support)
            assert word in _lib.last_error() and ptr.value == 0x1234 and count.value == 77  # nothing is written
        for min_count, min_support in ((0, 1), (256, 1), (2, 0), (2, 33), (-1, 1), (2, -5), (1 << 32, 1), (2, 1 << 32), ((1 << 32) + 2, 1)):
            with pytest.raises(ValueError):
                query.repairs(bases, offsets, min_count, min_support)
        assert _same_state(_state(query), before)
        _check(query, c, 2, 1)
        _check(query, c, 255, 32)
