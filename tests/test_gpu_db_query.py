"""kmers.DatabaseQuery (tbk_kmerdb_query) against the Python loop of tests/db_query_ref.py: the counter of every window, the
per-sequence totals, the histogram, completeness and the copy spectrum - at the lengths and positions where the lookup kernel
changes path (a pass of 2048 window starts, a sequence's ends, a separator), at the edges of the directory over the ranks, and
on seeded random input.  Everything is integers: every comparison is exact."""
import os

import numpy as np
import pytest

import db_query_ref as ref

pytestmark = pytest.mark.gpu

KS = (5, 21, 31, 32)


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _counter_of(kmer):
    """a counter 2..255 that depends on the k-mer alone, 255 and 2 among them"""
    return 2 + ref.lex_rank(kmer) % 254


def _db_of(sequences, k):
    return {km: _counter_of(km) for s in sequences for km in ref.window_kmers(s, k) if km is not None}


@pytest.fixture()
def load(gpu, tmp_path):
    """load(db dict, k) -> KmerDatabase of a crafted file; closed at the end of the test"""
    from trio_binning_amd import kmers

    opened = []

    def _load(db, k):
        path = tmp_path / "db{}.tbkdb".format(len(opened))
        path.write_bytes(ref.database_bytes(db, k))
        opened.append(kmers.KmerDatabase.load(str(path)))
        assert len(opened[-1]) == len(db)
        return opened[-1]

    yield _load
    for d in opened:
        d.close()


def _check_batch(query, tally, sequences, k, min_count=2):
    """one batch through both; everything a batch answers with is compared"""
    from trio_binning_amd import kmers

    bases, offsets = kmers.pack_reads(sequences)
    want_per_read, want_counts = tally.add(sequences, k, min_count)
    per_read, counts = query.add(bases, offsets, min_count, return_counts=True)
    assert per_read.dtype == np.uint64 and per_read.shape == (len(sequences), 2) and counts.dtype == np.uint8
    assert np.array_equal(counts, want_counts), np.flatnonzero(counts != want_counts)[:10]
    assert np.array_equal(per_read, want_per_read), (per_read.tolist(), want_per_read.tolist())
    return per_read, counts


def _check_session(query, tally, copies=False):
    assert np.array_equal(query.histogram(), tally.hist)
    assert query.completeness() == tally.completeness()
    if copies:
        assert np.array_equal(query.copy_spectrum(), tally.spectrum())


# ---- 1. lengths around k and around the pass edge ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_lengths_alone_and_behind_a_first_sequence(load, k):
    rng = np.random.default_rng(100 + k)
    genome = _seq(rng, 2049 + k + 150)
    db = _db_of([genome[:1500]], k)  # (windows past 1500 are absent at k >= 21; at k = 5 nearly every 5-mer is held)
    with load(db, k).query() as query:
        tally = ref.Tally(db)
        for length in (k - 1, k, k + 1, 2047, 2048, 2049 + k):
            _check_batch(query, tally, [genome[:length]], k)
            _check_batch(query, tally, [genome[100:150], genome[:length]], k)
        _check_batch(query, tally, ["", genome[:300], "", "", genome[2000:2100 + k], ""], k)
        _check_batch(query, tally, ["", ""], k)
        _check_session(query, tally)
        # an empty batch
        per_read = query.add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        assert per_read.shape == (0, 2)
        assert query.counts(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)).size == 0
        _check_session(query, tally)


# ---- 2. N and lower case at the ends and on each side of a pass edge ------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_n_and_lower_case_at_the_ends_and_the_pass_edge(load, k):
    rng = np.random.default_rng(200 + k)
    s = _seq(rng, 2048 + 3 * k)
    db = _db_of([s], k)
    with load(db, k).query() as query:
        tally = ref.Tally(db)
        plain, plain_counts = _check_batch(query, tally, [s], k)
        assert int(plain[0, 0]) == int(plain[0, 1]) == len(s) - k + 1 and plain_counts[:len(s) - k + 1].min() >= 2
        for at in (0, len(s) - 1, 2047, 2048):
            with_n = s[:at] + "N" + s[at + 1:]
            per_read, _ = _check_batch(query, tally, [with_n], k)
            lost = min(at, len(s) - k) - max(at - k + 1, 0) + 1
            assert int(per_read[0, 0]) == len(s) - k + 1 - lost
            with_n_lower = s[:at] + "n" + s[at + 1:]
            _check_batch(query, tally, [with_n_lower], k)
            lower = s[:at] + s[at].lower() + s[at + 1:]
            per_read, counts = _check_batch(query, tally, [lower], k)
            assert np.array_equal(per_read, plain) and np.array_equal(counts, plain_counts)  # lower case is found as upper case
        per_read, counts = _check_batch(query, tally, [s.lower()], k)
        assert np.array_equal(per_read, plain) and np.array_equal(counts, plain_counts)
        # the same positions behind a first sequence: the separator moves the stream by one
        _check_batch(query, tally, [s[:7], s[:2039] + "N" + s[2040:]], k)
        _check_batch(query, tally, [s[:7], s[:2040] + "n" + s[2041:]], k)
        _check_session(query, tally)


# ---- 3. a database queried with the reads it was counted from --------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_a_database_finds_the_reads_it_was_counted_from(gpu, k):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    rng = np.random.default_rng(300 + k)
    genome = _seq(rng, 1500)
    reads = [genome[p:p + n] for p, n in ((int(rng.integers(0, 1300)), int(rng.integers(k, 200))) for _ in range(60))]
    reads += ["A" * 400, "acgtn" + genome[:100].lower(), "N" * 40, "", _seq(rng, 90)]  # poly-A past 255, lower case, singletons
    occurrences = uo.count_kmers(reads, k)
    db = uo.database(occurrences)
    assert max(occurrences.values()) > 255 and min(occurrences.values()) == 1
    with kmers.KmerCounter(k, 100_000) as counter:
        counter.add_reads(reads)
        with counter.database() as database, database.query() as query:
            assert len(database) == len(db)
            tally = ref.Tally(db)
            _, counts = _check_batch(query, tally, reads, k)
            at = 0
            for s in reads:
                for w, km in enumerate(ref.window_kmers(s, k)):
                    if km is not None:
                        assert int(counts[at + w]) == (min(occurrences[km], 255) if occurrences[km] >= 2 else 0)
                at += len(s)
            assert query.completeness(2, 255) == (len(db), len(db))
            _check_session(query, tally)


# ---- 4. the edges of the directory --------------------------------------------------------------------------------------------------
def _canonical_with_prefix(k, prefix, n, rng):
    """n distinct canonical k-mers that start with `prefix`, sorted: tails are drawn until enough of them are canonical"""
    out = set()
    while len(out) < n:
        km = prefix + _seq(rng, k - len(prefix))
        if ref.canonical(km) == km:
            out.add(km)
    return sorted(out)


@pytest.mark.parametrize("k", KS)
def test_directory_edges(load, k):
    rng = np.random.default_rng(400 + k)
    # the largest canonical k-mer: it starts with as many T as it ends with A, and an odd k's middle base is at most its complement
    largest = "T" * (k // 2) + ("C" if k % 2 else "") + "A" * (k // 2)
    assert ref.canonical(largest) == largest
    probe = _seq(rng, 300)
    cases = {
        "empty": {},
        "one": {ref.canonical(probe[10:10 + k]): 7},
        "two": {ref.canonical(probe[10:10 + k]): 7, ref.canonical(probe[90:90 + k]): 255},
        "poly_a": {"A" * k: 9},
        "largest_rank": {largest: 11, "A" * k: 2},
    }
    if k > 5:
        # keys that crowd one prefix bucket (they share their first 16 bases), and keys that leave most buckets empty
        crowd = _canonical_with_prefix(k, "ACCA" * 4, 300, rng)
        cases["crowded_bucket"] = {km: _counter_of(km) for km in crowd}
        sparse = _canonical_with_prefix(k, "AAAAAAAAAA", 150, rng) + _canonical_with_prefix(k, "CCCCCCCCCA", 150, rng)
        cases["sparse_buckets"] = {km: _counter_of(km) for km in sparse}
    for name, db in cases.items():
        held = sorted(db)
        sequences = [probe, "A" * (k + 3), largest, ref.revcomp(largest) + "N" + largest]
        sequences += ["N".join(held[:40]), "".join(ref.revcomp(km) for km in held[-40:])]
        with load(db, k).query(copies=True) as query:
            tally = ref.Tally(db)
            _check_batch(query, tally, sequences, k)
            _check_session(query, tally, copies=True)
            assert query.completeness()[1] == len(db), name


def test_every_canonical_5_mer(load):
    from itertools import product

    every = sorted({ref.canonical("".join(p)) for p in product("ACGT", repeat=5)})
    assert len(every) == 512 and every[0] == "AAAAA" and every[-1] == "TTCAA"
    db = {km: _counter_of(km) for km in every}
    rng = np.random.default_rng(45)
    with load(db, 5).query(copies=True) as query:
        tally = ref.Tally(db)
        per_read, counts = _check_batch(query, tally, ["".join(every), _seq(rng, 3000)], 5)
        assert np.array_equal(per_read[:, 0], per_read[:, 1]) and counts[:512 * 5 - 4].min() >= 2  # nothing is absent
        _check_session(query, tally, copies=True)
        assert query.completeness() == (512, 512)


# ---- 5. a k-mer that is its own reverse complement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (4, 32))
def test_a_k_mer_that_is_its_own_reverse_complement(load, k):
    half = "ACGGTCAATCGATTGC"[:k // 2]
    own = half + ref.revcomp(half)
    assert ref.revcomp(own) == own and len(own) == k
    other = ref.canonical("C" + own[1:])
    db = {own: 33, other: 5}
    with load(db, k).query(copies=True) as query:
        tally = ref.Tally(db)
        per_read, counts = _check_batch(query, tally, [own, "T" + own + "N" + own, ref.revcomp(other)], k)
        assert per_read.tolist() == [[1, 1], [3, 2], [1, 1]] and int(counts[0]) == 33
        assert tally.copies[own] == 3  # once per window, whichever strand
        spec = query.copy_spectrum()
        assert np.array_equal(spec, tally.spectrum()) and int(spec[3, 33]) == 1 and int(spec[1, 5]) == 1 and int(spec.sum()) == 2


# ---- 6. copies ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_copies_of_repeated_sequences(load, k):
    rng = np.random.default_rng(600 + k)
    units = [_seq(rng, 60 + k) for _ in range(8)]  # unit i is held i times, unit 0 by the database alone
    db = _db_of(units, k)
    with load(db, k).query(copies=True) as query:
        tally = ref.Tally(db)
        first = [u for i, u in enumerate(units) for _ in range(min(i, 3))]
        second = [ref.revcomp(u) if i % 2 else u for i, u in enumerate(units) for _ in range(max(i - 3, 0))]
        _check_batch(query, tally, first, k)
        _check_session(query, tally, copies=True)
        _check_batch(query, tally, second, k)  # two batches accumulate
        _check_session(query, tally, copies=True)
        spec = query.copy_spectrum()
        assert int(spec.sum()) == len(db) and int(spec[0].sum()) > 0
        if k >= 21:  # (the units share no k-mer: every k-mer of unit i has exactly i copies, and 5, 6 and 7 fold into the last row)
            for i in range(5):
                assert int(spec[i].sum()) == len(_db_of([units[i]], k))
            assert int(spec[5].sum()) == len(_db_of(units[5:], k))
        query.reset()
        fresh = ref.Tally(db)
        _check_session(query, fresh, copies=True)
        assert int(query.histogram().sum()) == 0 and query.completeness() == (0, len(db))
        _check_batch(query, fresh, units[:2], k)
        _check_session(query, fresh, copies=True)
    with load(db, k).query() as plain:
        with pytest.raises(ValueError, match="without copies"):
            plain.copy_spectrum()


# ---- 7. min_count ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_min_count_changes_found_and_solid_but_not_counts(load, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(700 + k)
    s = _seq(rng, 900)
    db = _db_of([s[:600]], k)
    with load(db, k).query() as query:
        tally = ref.Tally(db)
        low, counts_low = _check_batch(query, tally, [s, s[:50]], k, 2)
        high, counts_high = _check_batch(query, tally, [s, s[:50]], k, 100)
        assert np.array_equal(counts_low, counts_high) and np.array_equal(low[:, 0], high[:, 0])
        assert int(high[0, 1]) < int(low[0, 1])
        assert np.array_equal(query.counts(*kmers.pack_reads([s, s[:50]])), counts_low)
        tally.add([s, s[:50]], k)
        for cuts in ((2, 255), (100, 255), (2, 99), (100, 100), (0, 1000), (200, 100)):
            assert query.completeness(*cuts) == tally.completeness(*cuts), cuts
        assert query.completeness(100, 255)[1] < query.completeness(2, 255)[1]
        none, _ = _check_batch(query, tally, [s], k, 256)
        assert int(none[0, 1]) == 0 and int(none[0, 0]) == int(low[0, 0])
        _check_session(query, tally)


# ---- 8. seeded fuzz ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "100"))))  # more seeds for a soak run
def test_fuzz_against_the_reference_loop(load, seed):
    from oracle import unique_oracle as uo

    rng = np.random.default_rng(8000 + seed)
    k = int(rng.choice(KS))
    genome = _seq(rng, int(rng.integers(300, 1500)))
    reads = []
    for _ in range(int(rng.integers(5, 60))):
        n = int(rng.integers(k, 150))
        p = int(rng.integers(0, max(len(genome) - n, 1)))
        r = genome[p:p + n]
        reads.append(ref.revcomp(r) if rng.integers(0, 2) else r)
    db = uo.database(uo.count_kmers(reads, k))
    contigs = []
    for _ in range(int(rng.integers(1, 6))):
        n = int(rng.integers(0, len(genome)))
        p = int(rng.integers(0, len(genome) - n + 1))
        c = list(genome[p:p + n])
        for _ in range(int(rng.integers(0, 4))):  # planted substitutions, an N, a soft-masked stretch
            if c:
                at = int(rng.integers(0, len(c)))
                c[at] = "ACGT"[("ACGT".index(c[at]) + 1 + int(rng.integers(0, 3))) % 4]
        if c and rng.integers(0, 3) == 0:
            c[int(rng.integers(0, len(c)))] = "N"
        if c and rng.integers(0, 3) == 0:
            at = int(rng.integers(0, len(c)))
            c[at:at + 30] = [x.lower() for x in c[at:at + 30]]
        c = "".join(c)
        contigs.append(ref.revcomp(c.upper()) if rng.integers(0, 4) == 0 else c)
    min_count = int(rng.choice((2, 2, 3, 5)))
    copies = bool(rng.integers(0, 2))
    with load(db, k).query(copies=copies) as query:
        tally = ref.Tally(db)
        _check_batch(query, tally, contigs, k, min_count)
        if rng.integers(0, 2):
            _check_batch(query, tally, contigs[::-1] + reads[:3], k, min_count)
        _check_session(query, tally, copies=copies)
        cuts = (min_count, int(rng.integers(min_count, 256)))
        assert query.completeness(*cuts) == tally.completeness(*cuts)


# ---- 9. the window cap --------------------------------------------------------------------------------------------------------------------
def test_a_session_refuses_to_pass_the_window_cap(load, gpu):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(9)
    s = _seq(rng, 120)  # 100 window starts
    db = _db_of([s], k)
    with load(db, k).query(copies=True) as query:
        tally = ref.Tally(db)
        bases, offsets = kmers.pack_reads([s, "ACGT"])
        assert gpu.lib.tbk_kmerdb_query_set_windows_(query._h, (1 << 32) - 1 - 100) == 0
        _check_batch(query, tally, [s, "ACGT"], k)  # exactly 2^32 - 1: taken
        with pytest.raises(ValueError, match="2\\^32 - 1 window starts"):
            query.add(bases, offsets)
        with pytest.raises(ValueError, match="2\\^32 - 1 window starts"):
            query.counts(*kmers.pack_reads(["A" * k]))
        query.add(*kmers.pack_reads(["A" * (k - 1), ""]))  # no window start: nothing to refuse
        _check_session(query, tally, copies=True)  # a refused batch left nothing behind
        query.reset()
        fresh = ref.Tally(db)
        _check_batch(query, fresh, [s], k)
        _check_session(query, fresh, copies=True)
