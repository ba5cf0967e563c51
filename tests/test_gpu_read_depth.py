"""kmers.DatabaseQuery.read_depth (tbk_kmerdb_query_read_depth; kernels: csrc/tbk_read_depth.hip) against tests/read_depth_ref.py,
record for record and byte for byte, pad included.  One batch per k holds every shape at which the kernels can go wrong: a first
sequence of 4500 bases whose stream positions cross the pass edges at 2048 and 4096 and that takes several trips of the
256-positions-per-trip byte loop and of the 64-word bitmap loop, with six counters on window ranges that begin or end at 4-byte
word edges and at 32-bit bitmap edges, an N and a lower-case stretch inside them and k-mers seen once that a full database alone
holds; sequences of 0, k - 1, k, k + 1, k + 2 and k + 3 bases, so that every rank formula meets 1 to 4 clean windows and consecutive
sequences begin at all four byte alignments; sequences whose windows are all absent, all saturated, all at one counter, and all N;
even and odd numbers of clean and of present windows around two middle values that differ; a sequence whose median is 0 and whose
present_median is not; a reverse-complemented copy and, for even k, a k-mer that is its own reverse complement; and short
sequences of low counters that follow, four places behind - on the same wave of a one-block grid - long ones full of high
counters, which finds rows of LDS that were not cleared.  From k = 21 on the database is made of chosen windows of a random genome,
so the shapes are what the comments say, and the test says so on the reference's answer; below that every k-mer recurs all over
the genome and the reference alone is the judge.  tests/test_host_read_depth_ref.py holds the reference to a second formulation
and to hand-worked records.  Everything is integers: every comparison is exact."""
import os

import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
import read_depth_ref as rd

pytestmark = pytest.mark.gpu

PASS = 2048
KS = (1, 2, 5, 21, 31, 32)
COUNTERS = (2, 5, 10, 20, 127, 255)
MIN_COUNTS = (1, 2, 6, 255)
LONG = 4500  # the first sequence: 141 bitmap words - three trips of 64 lanes - and 1125 byte words - five trips of 256 positions
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

        rng = np.random.default_rng(2800 + k)
        self.k = k
        genome = list(_seq(rng, 16000))
        if k % 2 == 0:
            genome[3500:3500 + k] = _own_reverse_complement(k)
        genome = "".join(genome)
        planted = {}  # canonical k-mer -> counter, window by window

        def plant(source, windows, counter):
            for w in windows:
                planted.setdefault(ref.canonical(source[w:w + k].upper()), counter)

        # the first sequence, genome[:LONG]: its window w is stream position w
        plant(genome, range(28, 36), 5)                       # from a 4-byte word edge over the bitmap edge 31 / 32 to a word edge
        plant(genome, range(61, 67), 10)                      # begins and ends inside words, over the bitmap edge 63 / 64
        plant(genome, range(96, 128), 20)                     # one whole bitmap word
        plant(genome, range(1000, 1000 + 3 * k + 1), 127)     # an N goes to 1000 + 2k
        plant(genome, range(1500, 1541), 255)                 # in lower case
        plant(genome, range(PASS - 18, PASS), 2)              # ends at window 2047, a pass's last
        plant(genome, range(2 * PASS, 2 * PASS + 15), 10)     # begins at window 4096, a pass's first
        plant(genome, (0, LONG - k, 3500), 20)                # the first and the last window, and the k-mer that is its own reverse complement
        once = range(3000, 3011)                              # seen once: a full database alone holds them
        first = list(genome[:LONG])
        self.n_at = 1000 + 2 * k
        first[self.n_at] = "N"
        first[1495:1545 + k] = [c.lower() for c in first[1495:1545 + k]]
        first = "".join(first)
        self.cursor = LONG + 100

        def take(n):
            self.cursor += n + 40
            return genome[self.cursor - n - 40:self.cursor - 40]

        short = ["", take(max(k - 1, 0)), take(k), take(k + 1), take(k + 2), take(k + 3)]
        plant(short[2], (0,), 127)
        plant(short[3], (0,), 5); plant(short[3], (1,), 2)                                   # follows the first sequence on wave 0 of a one-block grid
        plant(short[4], (0,), 255); plant(short[4], (1,), 2); plant(short[4], (2,), 20)
        plant(short[5], (0,), 127); plant(short[5], (1,), 10); plant(short[5], (3,), 5)      # window 2 is absent
        saturated, absent, uniform = take(399 + k), take(200), take(320 + k)
        plant(saturated, range(400), 255)
        plant(uniform, range(321), 20)
        even, odd, even_present, odd_present, mostly_absent = take(k + 9), take(k + 10), take(k + 11), take(k + 11), take(k + 39)
        plant(even, range(0, 5), 5); plant(even, range(5, 10), 20)                           # 10 windows: the middle ones are 5 and 20
        plant(odd, range(0, 5), 5); plant(odd, range(5, 11), 20)                             # 11 windows
        plant(even_present, range(3, 6), 10); plant(even_present, range(6, 9), 127)          # 6 of 12 present: the middle ones are 10 and 127
        plant(odd_present, (1, 3), 2); plant(odd_present, (5,), 10); plant(odd_present, (7, 9), 255)  # 5 of 12 present
        plant(mostly_absent, range(0, 12, 2), 10); plant(mostly_absent, range(1, 12, 2), 127)  # 12 of 40 present: median 0, present_median 10
        tail = take(2400)
        plant(tail, range(0, 2400 - k + 1, 7), 10)
        #             0      1..6    7          8       9        10        11    12   13            14           15             16
        self.batch = [first] + short + [saturated, absent, uniform, "N" * 50, even, odd, even_present, odd_present, mostly_absent,
                                        ref.revcomp(genome[100:1700]), tail]
        self.index = {"short": 1, "saturated": 7, "absent": 8, "uniform": 9, "all_n": 10, "even": 11, "odd": 12, "even_present": 13, "odd_present": 14,
                      "mostly_absent": 15, "mirrored": 16, "tail": 17}
        held = sorted(planted)
        if k <= 5:  # nearly every small k-mer is among them: keep a third, or everything is present everywhere
            held = held[::3]
            if k % 2 == 0 and _own_reverse_complement(k) not in held:
                held.append(_own_reverse_complement(k))
            self.db = {km: COUNTERS[i % 6] for i, km in enumerate(sorted(held))}
        else:
            self.db = dict(planted)
        seen_once = {ref.canonical(genome[w:w + k]) for w in once} - set(self.db)
        self.full_db = dict(self.db, **{km: 1 for km in seen_once})
        if k % 2 == 0:
            assert any(km == ref.revcomp(km) for km in self.db)
        self.stream = sum(len(s) + 1 for s in self.batch)
        assert self.stream > 4 * PASS  # a grid of one, two or three waves takes later trips over the passes
        self.lengths = [len(s) for s in self.batch]
        self.starts = np.cumsum([0] + [n + 1 for n in self.lengths[:-1]])  # offsets[r] + r
        self.file, self.full_file = _file(self.db, k, False), _file(self.full_db, k, True)
        self.packed = kmers.pack_reads(self.batch)
        self.counters = {False: rd.window_counters(self.db, self.batch, k), True: rd.window_counters(self.full_db, self.batch, k)}
        self.answers = {}

    def want(self, min_count, full=False):
        key = (min_count, full)
        if key not in self.answers:
            self.answers[key] = rd.as_array(rd.records(self.counters[full], min_count, floor=1 if full else 2))
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


def _check(query, c, min_count, full=False):
    from trio_binning_amd import kmers

    want = c.want(min_count, full)
    before = _state(query)
    got = query.read_depth(*c.packed, min_count)
    what = "k {}, min_count {}, full {}".format(c.k, min_count, full)
    assert got.dtype == kmers.READ_DEPTH == rd.READ_DEPTH, what
    assert got.tobytes() == want.tobytes(), (what, rd.first_difference(got, want))
    assert _same_state(_state(query), before), what  # the call only reads the session
    return want


def _tuple(rec):
    return tuple(int(rec[f]) for f in rd.FIELDS)


# ---- 1. every k, both databases, every threshold -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_threshold_against_the_reference(case, load, k):
    c = case(k)
    not_vacuous(c)
    with load(c.file).query(copies=True) as query:
        _check(query, c, 1)  # before anything was added
        per_read = query.add(*c.packed)
        for min_count in MIN_COUNTS:
            _check(query, c, min_count)
        # clean is add's clean, and present is add's found
        for min_count in (2, 6, 255):
            assert np.array_equal(query.add(*c.packed, min_count)[:, 1], c.want(min_count)["present"]), min_count
        assert np.array_equal(per_read[:, 0], c.want(1)["clean"])
    with load(c.full_file).query() as query:  # a session without copies, on a full database: min_count 1 counts the k-mers seen once
        for min_count in MIN_COUNTS:
            _check(query, c, min_count, full=True)


def not_vacuous(c):
    """the reference's own answers hold the shapes that the batch was built for (no device is asked)"""
    k, at = c.k, c.index
    plain, full = c.want(1), c.want(1, full=True)
    assert plain[1].tobytes() == plain[2].tobytes() == plain[at["all_n"]].tobytes() == bytes(40)  # 0 and k - 1 bases, all N: all-zero records
    assert [int(plain[i]["clean"]) for i in (3, 4, 5, 6)] == [1, 2, 3, 4]
    judged = [r for r in range(len(c.batch)) if int(plain[r]["clean"])]
    assert {int(c.starts[r]) % 4 for r in judged[:8]} == {0, 1, 2, 3}  # every byte alignment of a sequence's first word
    assert c.want(6).tobytes() != plain.tobytes() != c.want(255).tobytes() and full.tobytes() != plain.tobytes()
    assert c.want(2).tobytes() == plain.tobytes()  # a solid database's floor
    assert LONG - k > 2 * PASS + 64 and (LONG + 3) // 4 > 4 * 256 and (LONG + 31) // 32 > 2 * 64
    # a short sequence of low counters four places behind a long one of high counters: the same wave of a one-block grid
    stale = [r for r in range(4, len(c.batch)) if int(plain[r - 4]["clean"]) >= 300 and int(plain[r - 4]["highest"]) == 255
             and 0 < int(plain[r]["clean"]) <= 12 and int(plain[r]["highest"]) <= 20]
    assert (4 in stale and at["even"] in stale) or k < 21
    if k >= 21:  # the shapes are the ones planted (below that every k-mer recurs all over the genome)
        #                                  clean present saturated sum    lowest q1 median q3 highest present_median
        assert _tuple(plain[3]) == (1, 1, 0, 127, 127, 127, 127, 127, 127, 127)
        assert _tuple(plain[4]) == (2, 2, 0, 7, 2, 2, 2, 2, 5, 2)
        assert _tuple(plain[5]) == (3, 3, 1, 277, 2, 2, 20, 20, 255, 20)
        assert _tuple(plain[6]) == (4, 3, 0, 142, 0, 0, 5, 10, 127, 10)
        assert _tuple(plain[at["saturated"]]) == (400, 400, 400, 400 * 255) + (255,) * 6
        assert _tuple(plain[at["absent"]]) == (200 - k + 1,) + (0,) * 9
        assert _tuple(plain[at["uniform"]]) == (321, 321, 0, 321 * 20) + (20,) * 6
        assert _tuple(plain[at["even"]]) == (10, 10, 0, 125, 5, 5, 5, 20, 20, 5)
        assert _tuple(plain[at["odd"]]) == (11, 11, 0, 145, 5, 5, 20, 20, 20, 20)
        assert _tuple(plain[at["even_present"]]) == (12, 6, 0, 411, 0, 0, 0, 10, 127, 10)
        assert _tuple(plain[at["odd_present"]]) == (12, 5, 2, 524, 0, 0, 0, 2, 255, 10)
        assert _tuple(plain[at["mostly_absent"]]) == (40, 12, 0, 822, 0, 0, 0, 10, 127, 10)
        assert _tuple(c.want(6)[at["even"]]) == (10, 5, 0, 100, 0, 0, 0, 20, 20, 20)  # the 5s are below 6: depth 0
        assert _tuple(c.want(255)[at["odd_present"]]) == (12, 2, 2, 510, 0, 0, 0, 0, 255, 255)
        # the first sequence: 8 windows at 5, 6 at 10, 32 at 20, 2k + 1 at 127 around the N, 41 at 255 in lower case, 18 at 2, 15 at 10, 3 at 20
        present = 8 + 6 + 32 + (2 * k + 1) + 41 + 18 + 15 + 3
        assert _tuple(plain[0])[:4] == (LONG - k + 1 - k, present, 41, 8 * 5 + 21 * 10 + 35 * 20 + (2 * k + 1) * 127 + 41 * 255 + 18 * 2)
        assert _tuple(plain[0])[4:] == (0, 0, 0, 0, 255, 127)  # 82 present windows at 20 or less, more than that above
        assert _tuple(full[0])[:4] == (LONG - k + 1 - k, present + 11, 41, int(plain[0]["sum"]) + 11)  # the k-mers seen once
        mirrored = plain[at["mirrored"]]  # the reverse-complemented copy of [100, 1700): the same windows from the other end, all of them clean
        assert int(mirrored["clean"]) == 1600 - k + 1 and int(mirrored["present"]) == 28 + 3 * k + 1 + 41 and int(mirrored["saturated"]) == 41
    else:
        assert int(plain[0]["present"]) > 0 and int(plain[0]["clean"]) > int(plain[0]["present"])


# ---- 2. the later trips of the strided loops, and rows that a wave filled before ------------------------------------------------------
@pytest.mark.parametrize("k", (5, 21, 32))
def test_small_grids_take_later_trips(gpu, case, load, k):
    """with one, two and three wave slots the lookup strides over the passes and the per-read kernel, four sequences to a block, over
    the eighteen sequences: a wave's fifth sequence meets the rows that its first one filled"""
    c = case(k)
    assert len(c.batch) > 4 * 4 and c.stream > 4 * PASS
    with load(c.file).query() as query:
        for slots in (1, 2, 3):
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            _check(query, c, 1)
            _check(query, c, 6)
    with load(c.full_file).query() as query:
        assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, 1) == 0
        _check(query, c, 1, full=True)


def test_the_grid_of_a_whole_device_takes_a_second_trip(gpu, load):
    """tbk_launch_read_depth starts min(ceil(n / 4), wave_slots) blocks of four waves, a sequence to a wave, and wave_slots is 32 x
    compute units - 8192 on the 256 of an MI355X: from 4 x 8192 + 1 = 32769 sequences on the loop over the sequences takes a second
    trip.  33000 reads of k to k + 3 bases."""
    from trio_binning_amd import kmers

    k, n = 5, 33000
    rng = np.random.default_rng(28)
    reads = [_seq(rng, k + i % 4) for i in range(n)]
    reads[100] = reads[32768] = reads[32999] = "ACGTACG"
    reads[32900] = "ACNTA"
    db = {ref.canonical(km[:k]): COUNTERS[i % 6] for i, km in enumerate(sorted(set(reads[::2]))) if "N" not in km}
    want = rd.as_array(rd.read_depth(db, reads, k, 5))
    assert want["present"][32769:].any() and not want["median"][32769:].all() and int(want[32900]["clean"]) == 0
    with load(ref.database_bytes(db, k)).query() as query:
        got = query.read_depth(*kmers.pack_reads(reads), 5)
    assert got.tobytes() == want.tobytes(), rd.first_difference(got, want)


# ---- 3. the session, small databases and batches --------------------------------------------------------------------------------------
def test_the_session_is_only_read_and_calls_do_not_meet(gpu, case, load):
    from trio_binning_amd import kmers

    c, other = case(21), case(31)  # (the other batch: another genome, looked up in this database as 21-mers)
    other_want = rd.as_array(rd.read_depth(c.db, other.batch, 21))
    with load(c.file).query(copies=True) as query, load(c.file).query(copies=True) as untouched:
        query.add(*c.packed)
        untouched.add(*c.packed)
        _check(query, c, 1)
        got = query.read_depth(*other.packed)  # two calls in a row on different batches: the second is not the first's
        assert got.tobytes() == other_want.tobytes(), rd.first_difference(got, other_want)
        _check(query, c, 6)
        assert np.array_equal(query.histogram(), untouched.histogram())
        a, b = query.add(*other.packed, 2, True), untouched.add(*other.packed, 2, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same_state(_state(query), _state(untouched))
        assert gpu.lib.tbk_kmerdb_query_set_windows_(query._h, (1 << 32) - 2) == 0  # nearly at the session's limit: the batch does not count
        _check(query, c, 1)
        with pytest.raises(ValueError):
            query.add(*c.packed)
    assert kmers.READ_DEPTH.itemsize == 40


@pytest.mark.parametrize("k", (1, 5, 21))
def test_an_empty_database(load, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(80 + k)
    sequences = [_seq(rng, 2100), "", _seq(rng, k) + "N" + _seq(rng, 2 * k), _seq(rng, k)]
    with load(ref.database_bytes({}, k)).query() as query:
        got = query.read_depth(*kmers.pack_reads(sequences))
    assert got.tobytes() == rd.as_array(rd.read_depth({}, sequences, k)).tobytes()
    assert [int(v) for v in got["clean"]] == [2100 - k + 1, 0, k + 2, 1]
    assert not any(got[f].any() for f in rd.FIELDS[1:]) and not got["pad"].any()  # every depth is 0


@pytest.mark.parametrize("k", (2, 21, 32))
def test_a_database_of_one_entry(load, k):
    """one entry: the directory has no prefix bits"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(90 + k)
    s = _seq(rng, 3 * k)
    db = {ref.canonical(s[k:2 * k]): 5}
    sequences = [s, s[k:2 * k], ref.revcomp(s[k:2 * k]).lower(), s[k + 1:2 * k]]
    with load(ref.database_bytes(db, k)).query() as query:
        for min_count in (1, 5, 6):
            got = query.read_depth(*kmers.pack_reads(sequences), min_count)
            want = rd.as_array(rd.read_depth(db, sequences, k, min_count))
            assert got.tobytes() == want.tobytes(), rd.first_difference(got, want)
    if k > 2:
        assert rd.read_depth(db, sequences, k)[:3] == [(2 * k + 1, 1, 0, 5, 0, 0, 0, 0, 5, 5), (1, 1, 0, 5, 5, 5, 5, 5, 5, 5), (1, 1, 0, 5, 5, 5, 5, 5, 5, 5)]


def test_batches_without_a_window_or_a_read(gpu, case, load):
    from trio_binning_amd import kmers

    c = case(21)
    with load(c.file).query() as query:
        got = query.read_depth(*kmers.pack_reads(["ACGT", "", "A" * 20]))
        assert got.dtype == kmers.READ_DEPTH and got.size == 3 and got.tobytes() == bytes(120)
        got = query.read_depth(*kmers.pack_reads(["N" * 30]))
        assert got.tobytes() == bytes(40)
        got = query.read_depth(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))  # n_reads = 0
        assert got.size == 0 and got.dtype == kmers.READ_DEPTH
        assert gpu.lib.tbk_kmerdb_query_read_depth(query._h, None, np.zeros(1, dtype=np.uint64).ctypes.data, 0, 1, None) == 0
        _check(query, c, 1)


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
        for min_count in (0, 256, 1 << 31):
            assert gpu.lib.tbk_kmerdb_query_read_depth(query._h, bases.ctypes.data, offsets.ctypes.data, n, min_count, out.ctypes.data) == _lib.TBK_ERR_INVALID
            assert "min_count" in _lib.last_error() and (out == 77).all()  # nothing is written
        assert gpu.lib.tbk_kmerdb_query_read_depth(query._h, bases.ctypes.data, offsets.ctypes.data, n, 1, None) == _lib.TBK_ERR_INVALID
        assert "out is NULL" in _lib.last_error()
        # a sequence of 2^32 window starts is refused by its offsets alone, before a base is read (bases: one byte, never looked at)
        huge = np.array([0, 7, 7 + (1 << 32) + 20], dtype=np.uint64)
        assert gpu.lib.tbk_kmerdb_query_read_depth(query._h, bases.ctypes.data, huge.ctypes.data, 2, 1, out.ctypes.data) == _lib.TBK_ERR_INVALID
        assert "2^32" in _lib.last_error() and "sequence 1" in _lib.last_error() and (out == 77).all()
        for min_count in (0, 256, -1, 1 << 32, (1 << 32) + 2):
            with pytest.raises(ValueError):
                query.read_depth(bases, offsets, min_count)
        assert _same_state(_state(query), before)
        _check(query, c, 1)
        _check(query, c, 255)


# ---- 5. seeded fuzz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "6"))))  # more seeds for a soak run
def test_random_batches_and_databases(gpu, load, seed):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(28000 + seed)
    k = int(rng.choice([1, 3, 4, 8, 15, 16, 21, 27, 31, 32]))
    genome = _seq(rng, 6000)
    sequences = []
    for _ in range(int(rng.integers(5, 30))):
        n = int(rng.integers(0, 3001)) if rng.random() < 0.5 else int(rng.integers(0, 2 * k + 6))
        at = int(rng.integers(0, len(genome) - n + 1))
        s = list(genome[at:at + n] if rng.random() < 0.8 else _seq(rng, n))
        if s and rng.random() < 0.3:
            s = list(ref.revcomp("".join(s)))
        for _ in range(int(rng.integers(0, 4))) if n else ():
            s[int(rng.integers(0, n))] = "N"
        if n and rng.random() < 0.5:
            lo = int(rng.integers(0, n))
            hi = int(rng.integers(lo, n + 1))
            s[lo:hi] = [ch.lower() for ch in s[lo:hi]]
        sequences.append("".join(s))
    windows = [int(w) for w in rng.integers(0, len(genome) - k + 1, int(rng.integers(0, 3000)))]
    kind = seed % 3  # counters spread over the whole range, clustered at a depth with saturated repeats, or both with k-mers seen once
    db = {}
    for w in windows:
        counter = int(rng.integers(2, 256)) if kind == 0 else int(rng.choice([29, 30, 30, 31, 32, 255])) if kind == 1 else int(rng.integers(1, 256))
        db.setdefault(ref.canonical(genome[w:w + k]), counter)
    full = kind == 2
    counters = rd.window_counters(db, sequences, k)
    packed = kmers.pack_reads(sequences)
    with load(_file(db, k, full)).query() as query:
        for slots in (None, 1):
            if slots:
                assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, slots) == 0
            for min_count in (1, int(rng.integers(2, 256))):
                want = rd.as_array(rd.records(counters, min_count, floor=1 if full else 2))
                got = query.read_depth(*packed, min_count)
                assert got.tobytes() == want.tobytes(), (seed, k, slots, min_count, rd.first_difference(got, want))
