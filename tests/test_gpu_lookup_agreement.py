"""The four calls of a query session that walk a batch and look every window up in the database - add, track, repairs and
evidence (tbk_kmerdb_query_*; their lookup kernels share csrc/tbk_lookup.h) - see the same lookup: per sequence, with m = 2,

    add(min_count=m)[:, 0] == evidence()["clean"] == the sum of `clean` over the sequence's track bins
    add(min_count=m)[:, 1] == evidence(min_count=m, max_count=255)["held"]
    the sum of `windows` over the sequence's repairs(min_count=m) records == clean - found

No reference is computed: the other tests hold each call to its own.  One batch of about 5000 bases - an empty sequence, one
shorter than k, one with an N and lower-case bases, one that crosses stream position 2048 (a pass edge) with windows the database
holds on both sides, all longer ones with windows across multiples of 32 (a bitmap word) - against a database of a few hundred
k-mers and against the empty one, with the default grid and with a grid of one wave, where every loop over passes takes later
trips.  Everything is integers: every comparison is exact."""
import numpy as np
import pytest

import db_query_ref as ref

pytestmark = pytest.mark.gpu

M = 2
PASS = 2048
COUNTERS = (2, 3, 5, 20, 254, 255)


class Batch:
    def __init__(self, k):
        from trio_binning_amd import kmers

        rng = np.random.default_rng(4100 + k)
        genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 5000))
        marked = list(genome[100:400])
        marked[150] = "N"
        marked[200:230] = [c.lower() for c in marked[200:230]]
        self.sequences = ["", genome[10:10 + k - 1], "".join(marked), genome[500:2700], ref.revcomp(genome[550:1400]), genome[2240:3600]]
        starts = np.cumsum([0] + [len(s) + 1 for s in self.sequences])  # stream positions: one separator behind every sequence
        assert 4500 <= sum(len(s) for s in self.sequences) <= 5500 and starts[-1] > 2 * PASS  # a third pass: a grid of one wave takes a third trip
        assert starts[3] < PASS - 100 and starts[4] > PASS + 100  # the fourth sequence crosses the pass edge
        # the database: the k-mers of two stretches of the genome - the second lies over the pass edge in the fourth sequence -
        # without thirty windows of the first
        edge = 500 + PASS - int(starts[3])  # the genome's base at stream position 2048
        held = [i for i in list(range(600, 900)) + list(range(edge - 60, edge + 60)) if not 700 <= i < 730]
        kmers_held = sorted({ref.canonical(genome[i:i + k]) for i in held})
        self.db = {km: COUNTERS[(ref.lex_rank(km) * 7 + len(km)) % len(COUNTERS)] for km in kmers_held}
        assert 200 <= len(self.db) <= 900
        self.k = k
        self.packed = kmers.pack_reads(self.sequences)


_BATCHES = {}


@pytest.fixture(scope="module")
def batch(gpu):
    def get(k):
        if k not in _BATCHES:
            _BATCHES[k] = Batch(k)
        return _BATCHES[k]

    yield get
    _BATCHES.clear()


@pytest.mark.parametrize("one_wave", (False, True), ids=("default_grid", "one_wave"))
@pytest.mark.parametrize("empty", (False, True), ids=("database", "empty_database"))
@pytest.mark.parametrize("k", (21, 32))
def test_the_four_calls_see_the_same_lookup(gpu, batch, tmp_path, k, empty, one_wave):
    from trio_binning_amd import kmers

    b = batch(k)
    bases, offsets = b.packed
    n = len(b.sequences)
    path = tmp_path / "db.tbkdb"
    path.write_bytes(ref.database_bytes({} if empty else b.db, k))
    with kmers.KmerDatabase.load(str(path)) as db, db.query(copies=True) as query:
        if one_wave:
            assert gpu.lib.tbk_kmerdb_query_set_wave_slots_(query._h, 1) == 0
        per_read = query.add(bases, offsets, M)
        plain = query.evidence(bases, offsets)
        ranged = query.evidence(bases, offsets, M, 255)
        bins, prefix = query.track(bases, offsets, 64, 10)
        repairs = query.repairs(bases, offsets, M, 1)
    clean, found = per_read[:, 0].astype(np.int64), per_read[:, 1].astype(np.int64)
    assert per_read.shape == (n, 2) and plain.shape == ranged.shape == (n,) and prefix.shape == (n + 1,)
    # clean: add, evidence (whatever its range) and the track's bins
    assert np.array_equal(plain["clean"], per_read[:, 0]) and np.array_equal(ranged["clean"], per_read[:, 0])
    binned = np.array([int(bins["clean"][int(prefix[r]):int(prefix[r + 1])].sum()) for r in range(n)], dtype=np.int64)
    assert np.array_equal(binned, clean), (binned, clean)
    # found: add's second column and the windows evidence holds in [m, 255]
    assert np.array_equal(ranged["held"], per_read[:, 1]), (ranged["held"], per_read[:, 1])
    # broken: the stretches' windows add up to the clean windows that were not found
    broken = np.bincount(repairs["read"].astype(np.int64), weights=repairs["windows"], minlength=n).astype(np.int64)
    assert np.array_equal(broken, clean - found), (broken, clean - found)
    # not vacuous: the sequences are what the docstring says they are, and the database is at work on both sides of the pass edge
    lengths = np.array([len(s) for s in b.sequences])
    assert clean[0] == clean[1] == 0 and clean[2] == lengths[2] - k + 1 - k and np.array_equal(clean[3:], lengths[3:] - k + 1)
    if empty:
        assert not found.any() and repairs.size >= 5 and not plain["held"].any()
    else:
        assert (found[3:] > 0).all() and (found[3:] < clean[3:]).all() and found[3] >= 300 + 120 - 30 - k and found[4] >= 200
        assert (plain["held"] >= ranged["held"]).all() and repairs.size > n
