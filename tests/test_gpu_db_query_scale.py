"""kmers.DatabaseQuery on a database of more than 2048 x 1024 entries (csrc/tbk_query.hip): tbk_query_completeness_kernel and
tbk_query_spectrum_kernel run at most 2048 blocks of one tile of 1024 entries each, so only here does a block take a second
tile and add to the sums it already holds; the directory has 20 prefix bits, and tbk_query_directory_kernel's last block holds
one thread, the one that writes the entry count behind the last prefix.

The database is crafted: the canonical ranks of every 21-mer of a seeded random genome of 2 200 000 bases, counter 2 + rank % 254.
The reference is tests/db_query_ref.py's numpy one (TallyNp), which tests/test_host_db_query_ref_np.py holds to the Python loop.
Per-window counters, per-sequence totals, histogram, completeness and copy spectrum: every comparison is exact."""
import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf

pytestmark = pytest.mark.gpu

K = 21
GENOME = 2_200_000
TILES_AT_ONCE = 2048 * 1024  # entries that the per-entry kernels take in one trip of their tile loop
CUTS = ((2, 255), (100, 255), (2, 99), (255, 255), (2, 2), (17, 200))


def _revcomp(codes):
    return (3 - codes[::-1]).astype(np.uint8)


class Crafted:
    def __init__(self, path):
        rng = np.random.default_rng(2200)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        codes = rng.integers(0, 4, GENOME).astype(np.uint8)
        genome = letters[codes]
        rank, clean = ref.window_ranks(genome, np.array([0, GENOME], dtype=np.uint64), K)
        assert clean[:GENOME - K + 1].all()
        self.ranks = np.unique(rank[:GENOME - K + 1])
        self.counters = (2 + self.ranks % np.uint64(254)).astype(np.uint8)
        hist = np.bincount(self.counters, minlength=256).astype(np.uint64)
        hist[0] = self.ranks.size
        with open(path, "wb") as fh:
            fh.write(kf.file_bytes(K, self.ranks, self.counters, hist, reads=1, bases=GENOME))
        self.path = path
        # where the smallest and the largest entry lie in the genome: the two ends of the directory
        self.at_first = int(np.flatnonzero(rank[:GENOME - K + 1] == self.ranks[0])[0])
        self.at_last = int(np.flatnonzero(rank[:GENOME - K + 1] == self.ranks[-1])[0])

        def piece(lo, n, flip=False):
            part = codes[lo:lo + n]
            return letters[_revcomp(part) if flip else part]

        # slices of the genome given 1, 2, 3, 4, 5 and 7 times (the rest of it: 0 times), every other copy as its reverse
        # complement; the slices lie across tiles of 1024 entries everywhere, the entries being in rank order
        sequences = []
        for times, lo in ((1, 100_000), (2, 400_000), (3, 700_000), (4, 1_000_000), (5, 1_300_000), (7, 1_600_000)):
            sequences += [piece(lo, 30_000, flip=bool(c % 2)) for c in range(times)]
        lo_first, lo_last = (min(max(at - 10, 0), GENOME - 60) for at in (self.at_first, self.at_last))
        sequences += [piece(lo_first, 60), piece(lo_last, 60, flip=True)]
        self.where = {"first": self.at_first - lo_first, "last": 60 - K - (self.at_last - lo_last)}  # the entry's window in its sequence
        hurt = piece(1_900_000, 5000).copy()
        hurt[2500] = ord("N")
        hurt[3000:3100] |= 0x20  # a soft-masked stretch: found as upper case
        sequences += [hurt, letters[rng.integers(0, 4, 20_000)], np.zeros(0, dtype=np.uint8), piece(5, K - 1)]
        self.bases = np.concatenate(sequences)
        self.offsets = np.concatenate([[0], np.cumsum([s.size for s in sequences])]).astype(np.uint64)
        self.slots = {"first": len(sequences) - 6, "last": len(sequences) - 5, "hurt": len(sequences) - 4, "unrelated": len(sequences) - 3}
        self.tally = ref.TallyNp(self.ranks, self.counters)
        self.per_read, self.counts = self.tally.add(self.bases, self.offsets, K)
        self.spectrum = self.tally.spectrum()


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    return Crafted(str(tmp_path_factory.mktemp("scale") / "scale.tbkdb"))


@pytest.fixture(scope="module")
def database(gpu, crafted):
    from trio_binning_amd import kmers

    with kmers.KmerDatabase.load(crafted.path) as db:
        yield db


def test_the_database_and_the_batch_are_what_they_are_meant_to_be(crafted):
    c = crafted
    n = c.ranks.size
    # not vacuous: a second trip of the tile loops, a directory of 20 bits whose last block is the one thread behind the prefixes
    assert n > TILES_AT_ONCE and (n + 1023) // 1024 > 2048
    assert n.bit_length() - 2 == 20 and ((1 << 20) + 1) % 256 == 1
    assert (c.counters == 2).sum() > 0 and (c.counters == 255).sum() > 0 and c.counters.min() == 2
    # the smallest and the largest entry are queried, and found with their own counters
    for name, rank in (("first", c.ranks[0]), ("last", c.ranks[-1])):
        where = int(c.offsets[c.slots[name]]) + c.where[name]
        assert int(c.counts[where]) == 2 + int(rank) % 254 and int(c.tally.copies[0 if name == "first" else n - 1]) >= 1
    # every row of the copy spectrum is filled, entries past the first trip among them; absent windows; the N costs K windows
    assert (c.spectrum.sum(axis=1) > 0).all() and int(c.spectrum.sum()) == n
    assert int(c.tally.copies[TILES_AT_ONCE:].sum()) > 0 and int((c.tally.copies[TILES_AT_ONCE:] == 0).sum()) > 0
    assert int(c.tally.hist[0]) > 19_000 and int(c.per_read[c.slots["unrelated"], 1]) == 0
    assert c.per_read[c.slots["hurt"]].tolist() == [5000 - K + 1 - K, 5000 - K + 1 - K]
    assert c.per_read[-2:].tolist() == [[0, 0], [0, 0]]
    seen = [c.tally.completeness(*cuts) for cuts in CUTS]
    assert all(0 < a < b for a, b in seen) and len(set(seen)) == len(CUTS)


@pytest.mark.parametrize("copies", [False, True])
def test_a_database_past_one_trip_of_the_tile_loops(database, crafted, copies):
    c = crafted
    assert len(database) == c.ranks.size > TILES_AT_ONCE
    with database.query(copies=copies) as query:
        per_read, counts = query.add(c.bases, c.offsets, 2, return_counts=True)
        assert np.array_equal(counts, c.counts), np.flatnonzero(counts != c.counts)[:10]
        assert np.array_equal(per_read, c.per_read), np.flatnonzero((per_read != c.per_read).any(axis=1))[:10]
        assert np.array_equal(query.histogram(), c.tally.hist)
        for cuts in CUTS:
            assert query.completeness(*cuts) == c.tally.completeness(*cuts), cuts
        # the ends of the directory: the first and the last entry, alone
        for name, rank in (("first", c.ranks[0]), ("last", c.ranks[-1])):
            lo, hi = int(c.offsets[c.slots[name]]), int(c.offsets[c.slots[name] + 1])
            alone = query.counts(c.bases[lo:hi], np.array([0, hi - lo], dtype=np.uint64))
            assert np.array_equal(alone, c.counts[lo:hi]) and (2 + int(rank) % 254) in alone.tolist()
        if copies:
            # (the two sequences asked again each gave their entries one more copy)
            again = ref.TallyNp(c.ranks, c.counters)
            again.copies = c.tally.copies.copy()
            for name in ("first", "last"):
                lo, hi = int(c.offsets[c.slots[name]]), int(c.offsets[c.slots[name] + 1])
                again.add(c.bases[lo:hi], np.array([0, hi - lo], dtype=np.uint64), K)
            spec = query.copy_spectrum()
            assert np.array_equal(spec, again.spectrum()), np.argwhere(spec != again.spectrum())[:10]
        query.reset()
        assert query.completeness() == (0, c.tally.completeness()[1]) and int(query.histogram().sum()) == 0
        if copies:
            spec = query.copy_spectrum()
            assert int(spec[1:].sum()) == 0 and np.array_equal(spec[0], np.bincount(c.counters, minlength=256).astype(np.uint64))
