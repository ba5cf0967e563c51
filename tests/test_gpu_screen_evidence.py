"""kmers.DatabaseQuery.evidence (tbk_kmerdb_query_evidence; kernels: csrc/tbk_screen.hip) against tests/screen_ref.py, record for
record and byte for byte.  One batch per k holds every placement at which the kernels can go wrong: a first sequence of 4500
bases whose stream positions cross the pass edges at 2048 and 4096 and whose bitmap words take three trips of the evidence
kernel's 64-lane word loop, with a held run that ends at window 2047, one that begins at 4096, one over a word edge, held windows
at the sequence's first and last window, two exactly k apart (one stretch of 2k) and two k + 1 apart (two stretches), an N inside
a held run and a held run in lower case; a sequence with a held run over a pass edge (2047 / 2048 of its pass); a sequence held
throughout that is longer than 4096; a sequence whose last window is held before one whose first window is held; sequences of 0,
k - 1, k and k + 1 bases; a reverse-complemented copy; and a k-mer that is its own reverse complement.  From k = 21 on the database
is made of chosen windows of a random genome, so the placements are what the comments say, and the test says so on the
reference's answer; below that every k-mer recurs all over the genome and the reference alone is the judge.
tests/test_host_screen_ref.py holds the reference to a second formulation and to hand-worked records.  Everything is integers:
every comparison is exact."""
import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
import screen_ref as sr

pytestmark = pytest.mark.gpu

PASS = 2048
KS = (1, 2, 4, 5, 21, 31, 32)
COUNTERS = (2, 5, 10, 20, 127, 255)
RANGES = ((1, 255), (10, 20), (255, 255), (1, 1))
LONG = 4500  # the first sequence: 141 bitmap words, three trips of 64 lanes
WHOLE = 4200  # the sequence held throughout: longer than two passes
FULL = b"TBKKMFB1"  # a full database's magic: it also holds the k-mers seen once (floor 1)


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


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


class Case:
    """One genome, a solid and a full database of chosen windows of it, and one batch for one k, with the reference's answers."""

    def __init__(self, k):
        from trio_binning_amd import kmers

        rng = np.random.default_rng(2600 + k)
        self.k = k
        genome = list(_seq(rng, 12000))
        if k % 2 == 0:
            genome[3500:3500 + k] = _own_reverse_complement(k)
        genome = "".join(genome)
        # the held windows of the first sequence, genome[:LONG], by window start (its stream positions: it comes first)
        first_held = {0, LONG - k, 3500}
        first_held |= set(range(28, 36))                      # over the word edge 31 / 32
        first_held |= {200, 200 + k}                          # exactly k apart: one stretch of 2k
        first_held |= {400, 400 + k + 1}                      # k + 1 apart: two stretches
        first_held |= set(range(1000, 1000 + 3 * k + 1))      # an N goes to 1000 + 2k
        first_held |= set(range(1500, 1541))                  # in lower case
        first_held |= set(range(PASS - 18, PASS))             # ends at window 2047
        first_held |= set(range(2 * PASS, 2 * PASS + 15))     # begins at window 4096
        once = set(range(3000, 3011))                         # seen once: a full database alone holds them
        first = list(genome[:LONG])
        self.n_at = 1000 + 2 * k
        first[self.n_at] = "N"
        first[1495:1545 + k] = [c.lower() for c in first[1495:1545 + k]]
        first = "".join(first)
        whole = genome[LONG:LONG + WHOLE]
        ends, begins = genome[8700:9000], genome[9000:9300]
        short = ["", genome[11700:11700 + max(k - 1, 0)], genome[11800:11800 + k], genome[11900:11900 + k + 1]]
        self.batch = [first] + short + [ends, begins, ref.revcomp(genome[100:1700])]
        # a held run over a pass edge of the stream: the windows edge - 3 .. edge + 2 of the next sequence, genome[9300:11700]
        start = sum(len(s) + 1 for s in self.batch)
        self.straddler, self.edge = len(self.batch), (start // PASS + 1) * PASS - start
        if self.edge < 10:
            self.edge += PASS
        assert 10 <= self.edge < 2400 - k - 10
        self.batch += [genome[9300:11700], whole]
        self.whole = len(self.batch) - 1
        held = {genome[w:w + k] for w in first_held}
        held |= {genome[9300 + w:9300 + w + k] for w in range(self.edge - 3, self.edge + 3)}
        held |= {whole[w:w + k] for w in range(WHOLE - k + 1)}
        held |= {ends[300 - k:], begins[:k], short[2], short[3][:k]}
        held = sorted({ref.canonical(km) for km in held})
        if k <= 5:  # nearly every small k-mer is among them: keep a third, or everything is held everywhere
            held = held[::3]
            if k % 2 == 0 and _own_reverse_complement(k) not in held:
                held.append(_own_reverse_complement(k))
        self.db = {km: COUNTERS[i % 6] for i, km in enumerate(sorted(held))}
        seen_once = {ref.canonical(genome[w:w + k]) for w in once} - set(self.db)
        self.full_db = dict(self.db, **{km: 1 for km in seen_once})
        if k % 2 == 0:
            assert any(km == ref.revcomp(km) for km in self.db)
        self.stream = sum(len(s) + 1 for s in self.batch)
        assert self.stream > 6 * PASS  # a grid of three waves takes a third trip over the passes
        self.lengths = [len(s) for s in self.batch]
        self.file, self.full_file = _file(self.db, k, False), _file(self.full_db, k, True)
        self.packed = kmers.pack_reads(self.batch)
        self.counters = {False: sr.window_counters(self.db, self.batch, k), True: sr.window_counters(self.full_db, self.batch, k)}
        self.answers = {}

    def want(self, min_count, max_count, full=False):
        key = (min_count, max_count, full)
        if key not in self.answers:
            self.answers[key] = sr.as_array(sr.records(self.counters[full], self.lengths, self.k, min_count, max_count, floor=1 if full else 2))
        return self.answers[key]


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


def _check(query, c, min_count, max_count, full=False):
    from trio_binning_amd import kmers

    want = c.want(min_count, max_count, full)
    before = _state(query)
    got = query.evidence(*c.packed, min_count, max_count)
    what = "k {}, range [{}, {}], full {}".format(c.k, min_count, max_count, full)
    assert got.dtype == kmers.READ_EVIDENCE == sr.READ_EVIDENCE, what
    assert got.tobytes() == want.tobytes(), (what, sr.first_difference(got, want))
    assert _same_state(_state(query), before), what  # the call only reads the session
    return want


# ---- 1. every k, both databases, every range --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_range_against_the_reference(case, load, k):
    c = case(k)
    with load(c.file).query(copies=True) as query:
        _check(query, c, 1, 255)  # before anything was added
        per_read = query.add(*c.packed)
        for min_count, max_count in RANGES:
            _check(query, c, min_count, max_count)
        # clean is add's clean, and with no upper bound held is add's found
        for min_count in (2, 10, 255):
            assert np.array_equal(query.add(*c.packed, min_count)[:, 1], c.want(min_count, 255)["held"]), min_count
        assert np.array_equal(per_read[:, 0], c.want(1, 255)["clean"]) and np.array_equal(per_read[:, 1], c.want(1, 255)["held"])
    with load(c.full_file).query() as query:  # a session without copies, on a full database: min_count 1 counts presence
        for min_count, max_count in RANGES:
            _check(query, c, min_count, max_count, full=True)
    not_vacuous(c)


def not_vacuous(c):
    """the reference's own answers hold the placements that the batch was built for (no device is asked)"""
    k = c.k
    plain, once = c.want(1, 255), c.want(1, 1, full=True)
    assert not c.want(1, 1)["held"].any() and not c.want(1, 1)["covered"].any()  # empty after a solid database's floor
    assert c.want(10, 20).tobytes() != plain.tobytes() and (k < 4 or c.want(255, 255)["held"].any())
    # sequences of 0 and k - 1 bases get five zeros; one of k bases is one window
    assert plain[1].tobytes() == plain[2].tobytes() == bytes(40)
    assert int(plain[3]["clean"]) == 1 and int(plain[4]["clean"]) == 2
    L = c.lengths[c.whole]
    if k >= 21:  # the placements are the ones planted (below that every k-mer recurs all over the genome)
        assert int(once[0]["held"]) == 11 and int(once[0]["covered"]) == 10 + k and int(once[0]["stretches"]) == 1  # the k-mers seen once alone
        assert tuple(int(v) for v in plain[3]) == (1, 1, k, k, 1) and tuple(int(v) for v in plain[4]) == (2, 1, k, k, 1)
        assert tuple(int(v) for v in plain[c.whole]) == (L - k + 1, L - k + 1, L, L, 1)  # longest == L across the three trips
        # the last window of one sequence and the first of the next: two runs of k, nothing joins
        assert tuple(int(v) for v in plain[5]) == tuple(int(v) for v in plain[6]) == (300 - k + 1, 1, k, k, 1)
        assert tuple(int(v) for v in plain[c.straddler])[1:] == (6, k + 5, k + 5, 1)
        assert (c.edge + sum(c.lengths[:c.straddler]) + c.straddler) % PASS == 0  # its fourth held window is a pass's first
        # the first sequence: windows 0, 28 .. 35, 200 and 200 + k, 400 and 401 + k, the run around the N less the k windows that hold
        # it, 1500 .. 1540 in lower case, 2030 .. 2047, 3500, 4096 .. 4110 and the last one; its longest stretch is the 40 + k bases
        # in lower case, and [200, 200 + 2k) is one stretch where [400, 400 + k) and [401 + k, 401 + 2k) are two
        assert int(plain[0]["clean"]) == LONG - k + 1 - k and int(plain[0]["held"]) == 1 + 8 + 2 + 2 + (2 * k + 1) + 41 + 18 + 1 + 15 + 1
        assert int(plain[0]["longest"]) == 40 + k and int(plain[0]["stretches"]) == (11 if k >= 29 else 12)  # ([0, k) meets [28, 35 + k) from k = 29 on)
        assert LONG - k > 2 * PASS + 64
        mirrored = plain[7]  # the reverse-complemented copy of [100, 1700): the same windows from the other end, all of them clean
        assert int(mirrored["clean"]) == 1600 - k + 1 and int(mirrored["held"]) == 2 + 2 + (3 * k + 1) + 41
        assert int(mirrored["stretches"]) == 5 and int(mirrored["longest"]) == 4 * k
    else:
        assert int(plain[c.whole]["held"]) > 0 and int(plain[0]["stretches"]) > 12


# ---- 2. the later trips of the strided loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 21))
def test_small_grids_take_later_trips(gpu, case, load, k):
    """with one, two and three wave slots the lookup strides over the seven passes and the evidence kernel, four sequences to a
    block, over the ten sequences"""
    c = case(k)
    assert len(c.batch) > 2 * 4 and c.stream > 6 * PASS
    with load(c.file).query() as query:
        for slots in (1, 2, 3):
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            _check(query, c, 1, 255)
            _check(query, c, 10, 20)


def test_the_grid_of_a_whole_device_takes_a_second_trip(gpu, load):
    """tbk_launch_screen_evidence starts min(ceil(n / 4), wave_slots) blocks of four waves, a sequence to a wave, and wave_slots is
    32 x compute units - 8192 on the 256 of an MI355X: from 4 x 8192 + 1 = 32769 sequences on the loop over the sequences takes a
    second trip.  33000 reads of k bases, a window each."""
    from trio_binning_amd import kmers

    k, n = 5, 33000
    rng = np.random.default_rng(26)
    reads = [_seq(rng, k) for _ in range(n)]
    reads[100] = reads[32768] = reads[32999] = "ACGTA"
    reads[32900] = "ACNTA"
    db = {ref.canonical(km): COUNTERS[i % 6] for i, km in enumerate(sorted(set(reads[::2]))) if "N" not in km}
    want = sr.as_array(sr.evidence(db, reads, k, 5, 127))
    assert want["held"][32769:].any() and not want["held"][32769:].all() and int(want[32900]["clean"]) == 0
    with load(ref.database_bytes(db, k)).query() as query:
        got = query.evidence(*kmers.pack_reads(reads), 5, 127)
    assert got.tobytes() == want.tobytes(), sr.first_difference(got, want)


# ---- 3. small databases and batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 21))
def test_an_empty_database(load, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(80 + k)
    sequences = [_seq(rng, 2100), "", _seq(rng, k) + "N" + _seq(rng, 2 * k), _seq(rng, k)]
    with load(ref.database_bytes({}, k)).query() as query:
        got = query.evidence(*kmers.pack_reads(sequences))
    assert got.tobytes() == sr.as_array(sr.evidence({}, sequences, k)).tobytes()
    assert [int(v) for v in got["clean"]] == [2100 - k + 1, 0, k + 2, 1] and not got["held"].any() and not got["longest"].any()


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
            got = query.evidence(*kmers.pack_reads(sequences), min_count, max_count)
            want = sr.as_array(sr.evidence(db, sequences, k, min_count, max_count))
            assert got.tobytes() == want.tobytes(), sr.first_difference(got, want)
    if k > 2:
        assert [tuple(int(v) for v in r) for r in sr.evidence(db, sequences, k)[:3]] == [(2 * k + 1, 1, k, k, 1), (1, 1, k, k, 1), (1, 1, k, k, 1)]


def test_batches_without_a_window_or_a_read(gpu, case, load):
    from trio_binning_amd import kmers

    c = case(21)
    with load(c.file).query() as query:
        got = query.evidence(*kmers.pack_reads(["ACGT", "", "A" * 20]))
        assert got.dtype == kmers.READ_EVIDENCE and got.size == 3 and got.tobytes() == bytes(120)
        got = query.evidence(*kmers.pack_reads(["N" * 30]))
        assert got.tobytes() == bytes(40)
        got = query.evidence(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))  # n_reads = 0
        assert got.size == 0 and got.dtype == kmers.READ_EVIDENCE
        assert gpu.lib.tbk_kmerdb_query_evidence(query._h, None, np.zeros(1, dtype=np.uint64).ctypes.data, 0, 1, 255, None) == 0
        _check(query, c, 1, 255)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_usable(gpu, case, load):
    from trio_binning_amd import _lib

    c = case(21)
    bases, offsets = c.packed
    n = offsets.size - 1
    with load(c.file).query(copies=True) as query:
        query.add(bases, offsets)
        before = _state(query)
        out = np.full(n * 5, 77, dtype=np.uint64)
        for min_count, max_count, word in ((0, 255, "min_count"), (256, 256, "min_count"), (2, 1, "max_count"), (2, 256, "max_count"), (255, 254, "max_count")):
            assert gpu.lib.tbk_kmerdb_query_evidence(query._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, max_count,
                                                     out.ctypes.data) == _lib.TBK_ERR_INVALID, (min_count, max_count)
            assert word in _lib.last_error() and (out == 77).all()  # nothing is written
        for min_count, max_count in ((0, 255), (256, 256), (2, 1), (2, 256), (-1, 255), (2, -5), (1 << 32, 255), (2, 1 << 32), ((1 << 32) + 2, 255)):
            with pytest.raises(ValueError):
                query.evidence(bases, offsets, min_count, max_count)
        assert _same_state(_state(query), before)
        _check(query, c, 1, 255)
        _check(query, c, 255, 255)
