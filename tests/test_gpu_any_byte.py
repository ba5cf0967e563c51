"""Every byte value through the kernels that read ASCII bases: the query session's five passes (csrc/tbk_query.hip, tbk_depth.hip,
tbk_repair.hip, tbk_screen.hip), the k-mer counter and the hit tracker.  The rule everywhere: a base is one of the eight bytes
ACGTacgt - for the hit tracker without ignore_case one of ACGT - and every other value, 0x00 and 0x80 .. 0xFF included, makes the
windows over it unclean and nothing else.  The kernels decide that with masks (`& 0xDF`, a SWAR compare of the byte rebuilt from
its 2-bit code, a switch); the references decide it with a table of 256 entries (db_query_ref._CODE, hit_track_ref._CODE).

At k = 1 every value stands at every position of a chunk of 16 bytes, as one sequence and cut into sequences of 1, 15, 16, 17 and
255 bytes (see K1_LAYOUTS: the 256 x 17 bytes of tests/test_host_pack.py, and the same values in blocks of 257).  At k = 21 and k = 32 every value is planted into copies of a random
genome whose k-mers are the database, once at each of the stream residues 15, 10, 5 and 0 mod 16 - the four byte places of a
32-bit word, the first and the last byte of a chunk among them - at least k + 3 apart and away from the ends.

add, counts and track are judged by the numpy references on the raw bytes.  evidence and repairs are judged by the Python
loops, which take text: they get the batch with every byte that is no base rewritten to N, while the device gets the raw bytes.
That is the rule itself, not a shortcut - "every other value reads as N does" - and it is applied to the reference's copy alone.
Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref
import hit_track_ref as htr
import kmerdb_files as kf
import repair_ref as rr
import screen_ref as sr

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
COUNTERS = (2, 5, 10, 20, 127, 255)
RESIDUES = (15, 10, 5, 0)  # of the stream position mod 16, plant after plant: steps of 11 (mod 16), and 15 from 0 to 15
READ = 3000  # bases of one copy of the genome


def _as_text(bases):
    """the reference's copy: every byte that is no base rewritten to N, the case kept"""
    rewritten = np.where(np.isin(bases, BASES), bases, np.uint8(ord("N"))).astype(np.uint8)
    return rewritten.tobytes().decode("ascii")


def _sequences(text, offsets):
    return [text[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def _file(ranks, counters, k):
    hist = np.bincount(counters, minlength=256).astype(np.uint64)
    hist[0] = ranks.size
    return kf.file_bytes(k, ranks, counters, hist, reads=1, bases=k)


@pytest.fixture()
def load(gpu, tmp_path):
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
    return query.histogram(), query.completeness(), query.completeness(10, 200), query.copy_spectrum()


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- k = 1: every value at every position of a chunk ---------------------------------------------------------------------------------
# 256 x 17 bytes as tests/test_host_pack.py gives them to the classifier's packer.  In one sequence that puts value v at the bytes
# v + 256 j, always at chunk position v mod 16, since 16 divides 256; so the same values are given again in 16 blocks of 257 bytes - the
# 256 values and an N - which puts value v of block j at chunk position (v + j) mod 16: every value at every position.  Cut into
# sequences, the separators behind them shift the stream further; there 32 blocks of 258 bytes put every value at every position.
EVERY = np.tile(np.arange(256, dtype=np.uint8), 17)
SHIFTED = np.tile(np.append(np.arange(256, dtype=np.uint8), np.uint8(ord("N"))), 16)
SHIFTED_CUT = np.tile(np.append(np.arange(256, dtype=np.uint8), np.frombuffer(b"NN", dtype=np.uint8)), 32)


def _cut(total, lengths):
    """offsets of sequences of the given lengths, repeating, over `total` bytes (the last one takes what is left)"""
    offsets, i = [0], 0
    while offsets[-1] < total:
        offsets.append(min(offsets[-1] + lengths[i % len(lengths)], total))
        i += 1
    return np.array(offsets, dtype=np.uint64)


def _whole(total):
    return np.array([0, total], dtype=np.uint64)


K1_LAYOUTS = {"tiled, one sequence": (EVERY, _whole(EVERY.size)), "tiled, cut": (EVERY, _cut(EVERY.size, (1, 15, 16, 17, 255))),
              "shifted, one sequence": (SHIFTED, _whole(SHIFTED.size)), "shifted, cut": (SHIFTED_CUT, _cut(SHIFTED_CUT.size, (1, 15, 16, 17, 255)))}


def _chunk_positions(bases, offsets, value):
    """the positions mod 16 in the separated stream (a separator behind every sequence) at which `value` stands"""
    lengths = np.diff(offsets.astype(np.int64))
    stream = np.arange(bases.size) + np.repeat(np.arange(lengths.size), lengths)
    return {int(p) % 16 for p in stream[bases == value]}


@pytest.mark.parametrize("layout", sorted(K1_LAYOUTS))
def test_every_value_at_every_chunk_position_at_k_1(load, layout):
    k, (bases, offsets) = 1, K1_LAYOUTS[layout]
    ranks, counters = np.array([0, 1], dtype=np.uint64), np.array([7, 200], dtype=np.uint8)  # A (and T), C (and G)
    lengths = np.diff(offsets.astype(np.int64))
    assert EVERY.size == 4352 and int(offsets[-1]) == bases.size and ("cut" not in layout or {1, 15, 16, 17, 255} <= set(lengths.tolist()))
    if layout.startswith("shifted"):
        assert all(_chunk_positions(bases, offsets, v) == set(range(16)) for v in range(256)), layout
    times = {"tiled": 17, "shifted, one sequence": 16, "shifted, cut": 32}[layout if layout.startswith("shifted") else "tiled"]
    is_base = np.isin(bases, BASES)
    expected = np.zeros(bases.size, dtype=np.uint8)
    expected[np.isin(bases, np.frombuffer(b"AaTt", dtype=np.uint8))] = 7
    expected[np.isin(bases, np.frombuffer(b"CcGg", dtype=np.uint8))] = 200
    assert int(is_base.sum()) == 8 * times and np.array_equal(expected > 0, is_base)
    with load(_file(ranks, counters, k)).query(copies=True) as query:
        tally = ref.TallyNp(ranks, counters)
        want_per_read, want_counts = tally.add(bases, offsets, k)
        assert np.array_equal(want_counts, expected)  # the reference itself, against the rule spelled out
        per_read, counts = query.add(bases, offsets, return_counts=True)
        assert np.array_equal(counts, expected), np.flatnonzero(counts != expected)[:10]
        assert np.array_equal(per_read, want_per_read), np.flatnonzero((per_read != want_per_read).any(axis=1))[:10]
        assert int(per_read[:, 0].sum()) == 8 * times
        assert np.array_equal(query.histogram(), tally.hist) and np.array_equal(query.copy_spectrum(), tally.spectrum())
        before = _state(query)
        # evidence, from the numpy counters: None where the byte is no base
        per_sequence = [[int(c) if ok else None for c, ok in zip(expected[int(a):int(b)], is_base[int(a):int(b)])] for a, b in zip(offsets[:-1], offsets[1:])]
        for min_count, max_count in ((1, 255), (10, 255), (2, 7)):
            want = sr.as_array(sr.records(per_sequence, lengths.tolist(), k, min_count, max_count))
            got = query.evidence(bases, offsets, min_count, max_count)
            assert got.tobytes() == want.tobytes(), (min_count, max_count, sr.first_difference(got, want))
        assert int(sr.as_array(sr.records(per_sequence, lengths.tolist(), k, 1, 255))["held"].sum()) == 8 * times
        want, want_prefix = ctr.track_np(tally, bases, offsets, k, 64, 10)
        bins, prefix = query.track(bases, offsets, 64, 10)
        assert np.array_equal(prefix, want_prefix) and ctr.equal(bins, want), ctr.first_difference(bins, want)
        assert int(want["clean"].sum()) == 8 * times and int(want["absent"].sum()) == 0
        assert _same_state(_state(query), before)
        assert np.array_equal(query.counts(bases, offsets), expected)


# ---- k = 21 and k = 32: every value planted into copies of a genome ------------------------------------------------------------------
class Planted:
    def __init__(self, k):
        rng = np.random.default_rng(4100 + k)
        self.k = k
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        self.genome = letters[rng.integers(0, 4, READ)]
        # stream positions of the 1024 plants: residues 15, 10, 5, 0 and again, each step the smallest of its residue that keeps k + 3
        step = {r: next(s for s in range(k + 3, k + 19) if s % 16 == r) for r in (11, 15)}
        places, p = [], 2 * k + (15 - 2 * k) % 16
        for i in range(1024):
            while p % (READ + 1) < 2 * k or p % (READ + 1) > READ - 2 * k:  # away from the ends, and never a separator
                p += 16
            assert p % 16 == RESIDUES[i % 4]
            places.append(p)
            p += step[15] if i % 4 == 3 else step[11]
        places = np.array(places)
        assert (np.diff(places) >= k + 3).all()
        self.n_reads = int(places[-1]) // (READ + 1) + 1
        self.read_of, self.pos_of = places // (READ + 1), places % (READ + 1)
        self.values = (np.arange(1024) // 4).astype(np.uint8)  # every value at each of the four residues
        self.at = self.read_of * READ + self.pos_of  # in the batch's bytes: no separators there
        self.bases = np.tile(self.genome, self.n_reads)
        self.bases[self.at] = self.values
        self.offsets = (np.arange(self.n_reads + 1) * READ).astype(np.uint64)
        assert np.array_equal((self.at + self.read_of) % 16, np.tile(RESIDUES, 256)) and {int(v) % 4 for v in self.at + self.read_of} == {0, 1, 2, 3}
        rank, clean = ref.window_ranks(self.genome, [0, READ], k)
        self.ranks = np.unique(rank[clean])
        self.counters = np.array(COUNTERS, dtype=np.uint8)[((self.ranks * np.uint64(7) + np.uint64(k)) % np.uint64(6)).astype(np.int64)]
        self.file = _file(self.ranks, self.counters, k)
        self.db = {ref.canonical(self.genome[i:i + k].tobytes().decode()): None for i in range(READ - k + 1)}
        for km in self.db:
            at = int(np.searchsorted(self.ranks, np.uint64(ref.lex_rank(km))))
            self.db[km] = int(self.counters[at])
        self.text = _sequences(_as_text(self.bases), self.offsets)  # the reference's copy
        self.is_base = np.isin(self.values, BASES)
        self.same = self.is_base & (ref._CODE[self.values] == ref._CODE[self.genome[self.pos_of]])  # the genome's own base, in either case
        self.window_counters = sr.window_counters(self.db, self.text, k)
        self.evaluated = rr.evaluate(self.db, self.text, k, 2)

    def not_vacuous(self):
        k = self.k
        assert self.is_base.sum() == 32 and 4 <= self.same.sum() <= 16 and self.n_reads >= 9
        records = rr.as_array(rr.records(self.evaluated, k, 1))
        # a planted base letter that is not the genome's: one stretch of k windows, mended by the substitution that restores the
        # genome's base; the genome's own base in either case, and every value that is no base: no record
        assert records.size == int((self.is_base & ~self.same).sum())
        for i in np.flatnonzero(self.is_base & ~self.same):
            mine = records[(records["read"] == self.read_of[i]) & (records["pos"] == self.pos_of[i])]
            assert mine.size == 1 and int(mine["kind"][0]) == rr.SUB and int(mine["base"][0]) == int(self.genome[self.pos_of[i]]) and int(mine["windows"][0]) == k, i
        assert {int(self.values[i]) for i in np.flatnonzero(self.is_base & ~self.same)} & set(b"acgt")  # in lower case too
        # a value that is no base costs exactly k clean windows
        clean = sum(c is not None for per_read in self.window_counters for c in per_read)
        assert clean == self.n_reads * (READ - k + 1) - k * int((~self.is_base).sum())
        assert ref.window_ranks(self.bases, self.offsets, k)[1].sum() == clean  # the table and the rewritten text agree
        return {"plants": 1024, "base letters": int(self.is_base.sum()), "of them the genome's own base": int(self.same.sum()), "bases": int(self.bases.size)}


_PLANTED = {}


@pytest.fixture(scope="module")
def planted(gpu):
    def get(k):
        if k not in _PLANTED:
            _PLANTED[k] = Planted(k)
        return _PLANTED[k]

    yield get
    _PLANTED.clear()


@pytest.mark.parametrize("k", (21, 32))
def test_every_value_planted_into_a_genome(load, planted, k):
    from trio_binning_amd import kmers

    p = planted(k)
    p.not_vacuous()
    with load(p.file).query(copies=True) as query:
        tally = ref.TallyNp(p.ranks, p.counters)
        want_per_read, want_counts = tally.add(p.bases, p.offsets, k)
        per_read, counts = query.add(p.bases, p.offsets, return_counts=True)
        assert np.array_equal(counts, want_counts), np.flatnonzero(counts != want_counts)[:10]
        assert np.array_equal(per_read, want_per_read), np.flatnonzero((per_read != want_per_read).any(axis=1))[:10]
        assert np.array_equal(query.histogram(), tally.hist) and np.array_equal(query.copy_spectrum(), tally.spectrum())
        before = _state(query)
        for window in (64, 1 << 31):
            want, want_prefix = ctr.track_np(tally, p.bases, p.offsets, k, window, 10)
            bins, prefix = query.track(p.bases, p.offsets, window, 10)
            assert np.array_equal(prefix, want_prefix) and ctr.equal(bins, want), (window, ctr.first_difference(bins, want))
        lengths = [READ] * p.n_reads
        for min_count, max_count in ((1, 255), (10, 20)):
            want = sr.as_array(sr.records(p.window_counters, lengths, k, min_count, max_count))
            got = query.evidence(p.bases, p.offsets, min_count, max_count)
            assert got.dtype == kmers.READ_EVIDENCE and got.tobytes() == want.tobytes(), (min_count, max_count, sr.first_difference(got, want))
        for min_support in (1, k // 2 + 1, k):
            want = rr.as_array(rr.records(p.evaluated, k, min_support))
            got = query.repairs(p.bases, p.offsets, 2, min_support)
            assert got.dtype == kmers.REPAIR and got.tobytes() == want.tobytes(), (min_support, rr.first_difference(got, want))
        assert _same_state(_state(query), before)
        assert np.array_equal(query.counts(p.bases, p.offsets), want_counts)


# ---- the counter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", (1, 2))
@pytest.mark.parametrize("k", (1, 21, 32))
def test_the_counter_counts_the_windows_of_bases_alone(gpu, planted, k, passes):
    from trio_binning_amd import kmers

    if k == 1:  # both k = 1 batches, cut into sequences, as one library
        (tiled, cut), (shifted, cut_shifted) = K1_LAYOUTS["tiled, cut"], K1_LAYOUTS["shifted, cut"]
        bases, offsets = np.concatenate([tiled, shifted]), np.concatenate([cut, cut_shifted[1:] + cut[-1]])
    else:
        bases, offsets = planted(k).bases, planted(k).offsets
    rank, clean = ref.window_ranks(bases, offsets, k)
    want_ranks, want_counts = np.unique(rank[clean], return_counts=True)
    if k == 1:
        assert want_ranks.tolist() == [0, 1] and want_counts.tolist() == [4 * 49, 4 * 49]  # the database is A, C
    else:
        assert (want_counts == 1).any() and (want_counts >= planted(k).n_reads - 1).any()  # k-mers over a planted base; the genome's, once a copy
    for keep in (True, False):
        with kmers.KmerCounter(k, 300_000, passes=passes, keep_singletons=keep) as counter:
            counter.add(bases, offsets)
            hist = counter.histogram()
            assert int(hist[0]) == want_ranks.size and int(hist[1]) == int((want_counts == 1).sum())
            with counter.database() as db:
                held = want_counts >= (1 if keep else 2)
                keys, counters = db.entries()
                assert db.floor == (1 if keep else 2) and len(db) == int(held.sum())
                assert np.array_equal(keys, want_ranks[held]), (k, passes, keep)
                assert np.array_equal(counters, np.minimum(want_counts[held], 255).astype(np.uint8)), (k, passes, keep)


# ---- the hit tracker -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (21, 32))
def test_the_hit_tracker_narrows_the_bases_without_ignore_case(gpu, planted, k):
    """with ignore_case the eight letters are bases; without it a c g t are none, nor is any other byte that `& 0xDF` would turn into
    a base (there is none besides them).  hit_track_ref decides with a table and takes the raw bytes."""
    from trio_binning_amd import kmers

    p = planted(k)
    keys, clean = htr.window_keys(p.genome.tobytes(), k, False)
    assert clean.all()
    keys_a, keys_b = np.unique(keys[0::2]), np.unique(keys[1::2])
    sets = kmers.HashSet.from_keys(keys_a, k), kmers.HashSet.from_keys(keys_b, k)
    try:
        with kmers.HitTracker(*sets) as tracker:
            wants = {}
            for ignore_case in (False, True):
                want = htr.marks(p.bases, p.offsets, keys_a, keys_b, k, ignore_case)
                got = tracker.marks(p.bases, p.offsets, ignore_case)
                assert np.array_equal(got, want), (ignore_case, np.flatnonzero(got != want)[:10])
                runs, counts = tracker.runs(p.bases, p.offsets, ignore_case)
                assert np.array_equal(counts, htr.counts_of(want, p.offsets)), ignore_case
                want_runs = htr.runs(want, p.offsets)
                assert runs.dtype == want_runs.dtype and np.array_equal(runs, want_runs), ignore_case
                wants[ignore_case] = want
            # not vacuous: a plant that is no base costs k marks; the genome's own base in lower case costs them without ignore_case alone
            lower_same = p.same & (p.values >= 0x61)
            assert lower_same.sum() >= 1
            windows = p.n_reads * (READ - k + 1)
            assert int((wants[True] > 0).sum()) == windows - k * int((~p.same).sum())
            assert int((wants[False] > 0).sum()) == windows - k * int((~p.same).sum()) - k * int(lower_same.sum())
    finally:
        for hs in sets:
            hs.close()
