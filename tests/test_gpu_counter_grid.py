"""The later trips of the strided loops of the k-mer counter and the count databases (csrc/tbk_count_kernels.hip).

Every launcher of that file that strides takes a fixed grid, and a thread takes a second trip of its loop only when the work
outgrows it: from 1 048 577 reads in a batch (separate), 268 435 457 stream positions (retain), 1 048 577 or 2 097 153 table slots
(clamp, histogram, distil, export; rehash, unique), 2 097 153 database entries (db_unique, db_rank, db_solid_keys, kmerdb_unique),
and the counting kernel's pass loop never, because count_stream cuts pieces smaller than its grid.  Five of these kernels carry
a wave append (ballot, leader atomicAdd, __shfl) inside a loop that whole waves must leave together.

Hooked cases: the test hook tbk_count_set_grid_caps_(stream_blocks, entry_blocks) caps those grids at c = 1, 2, 3 and 5 blocks,
so that a library the numpy oracle counts in a moment (about 100 kbases a parent) takes tens to thousands of trips of every loop,
the stage refill and the carried bucket line of the counting kernel among them.  Everything is exact: histogram, A-minus-B
lists, database entries and files against oracle/unique_oracle.py and tests/kmerdb_files.py, and byte for byte against a
counter that ran without the hook.  The numbers the trip counts rest on are asserted (test_the_library_...).

Unhooked cases at the kernels' real steps: a database subtraction of 2 199 978 entries (past the 8192 x 256 of
tbk_kmerdb_unique_kernel) and a table of more than 5 000 000 slots (several trips of histogram, unique and export - the only
place where tbk_count_export_kernel runs past its first trip with its real step).  tbk_separate_kernel beyond 1 M reads and
tbk_retain_kernel beyond 268 M positions are reached with the hook only.

The clamp's later trips: tests/test_gpu_counter_shapes.py::test_clamp_keeps_a_counter_below_the_carry[1].

What the file notices, from a library whose stride loops each end after one trip, one kernel at a time (once, on an MI355X; the
48 capped cases are k x passes x solid/full x c, "subtraction" and "table" the two unhooked tests; no mutant passed):
  separate, count (plain and class forms), rehash      all 48 capped cases
  the counting kernel's stage not refilled             all 48
  histogram                                            all 48 and table
  retain, distil, db_unique, db_rank                   the 24 with passes = 3
  db_solid_keys                                        the 12 with passes = 3 and full databases
  count_unique, export                                 the 24 with passes = 1 and table
  kmerdb_unique, kmerdb_check                          all 48 and subtraction
  kmerdb_tally                                         the 24 with full databases (their union)
  clamp                                                none here; both cases of the clamp test (its table has 14.7 M slots)
Of the older tests, test_multi_piece_add / _in_passes (a 202 Mbase library) notice histogram, distil, rehash and count_unique,
test_gpu_kmerdb's swapped-keys and large-database tests and test_gpu_db_query_scale notice kmerdb_check; none notices the other ten."""
import functools
import tempfile

import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
from oracle import unique_oracle as uo
from test_gpu_counter_passes_shapes import _class_of
from test_gpu_kmerdb import _dump, _load_status, _rc, _swap

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3, 5)
RANGES = ((2, 255), (3, 20), (1, 4))
GENOME = 12_000
FULL_MAGIC = b"TBKKMFB1"  # a full database (keep_singletons): tests/test_gpu_counter_singletons.py


@pytest.fixture
def caps(gpu):
    """set(stream_blocks, entry_blocks); (0, 0) again when the test ends, however it ends"""
    def set_caps(stream_blocks, entry_blocks):
        assert gpu.lib.tbk_count_set_grid_caps_(stream_blocks, entry_blocks) == 0
    try:
        yield set_caps
    finally:
        gpu.lib.tbk_count_set_grid_caps_(0, 0)


# ---- the library ------------------------------------------------------------------------------------------------------------
def _reads(rng, genome):
    """About 8x of `genome` in reads of 0 to 400 bases (1 % substitutions, 0.2 % N, one read in sixteen lower case, half of them
    reverse-complemented), one read of 5000 and an empty read first, in the middle and last."""
    lengths = [400, 0, 1, 399]
    while sum(lengths) < 8 * len(genome) - 5000:
        lengths.append(int(rng.integers(0, 401)))
    lengths.insert(len(lengths) // 3, 5000)
    reads = []
    for i, n in enumerate(lengths):
        p = int(rng.integers(0, len(genome) - n))
        s = list(genome[p:p + n])
        for j in np.nonzero(rng.random(n) < 0.01)[0]:
            s[int(j)] = "ACGT"[int(rng.integers(0, 4))]
        for j in np.nonzero(rng.random(n) < 0.002)[0]:
            s[int(j)] = "N"
        r = "".join(s)
        if rng.random() < 0.5:
            r = _rc(r)
        if i % 16 == 7:
            r = r.lower()
        reads.append(r)
    reads.insert(len(reads) // 2, "")
    return [""] + reads + [""]


@functools.lru_cache(maxsize=None)
def _library():
    """(reads of parent A, reads of parent B): two parents of one genome of 12 000 bases, 1 site in 500 different"""
    rng = np.random.default_rng(20_261)
    base = rng.integers(0, 4, GENOME)

    def parent():
        codes = base.copy()
        at = np.nonzero(rng.random(GENOME) < 1 / 500)[0]
        codes[at] = (codes[at] + rng.integers(1, 4, at.size)) % 4
        return "".join("ACGT"[c] for c in codes)

    ga, gb = parent(), parent()
    return _reads(rng, ga), _reads(rng, gb)


def _batches(reads):
    """Two batches, a quarter and the rest: the second alone outgrows the table that the first left, so the table is rebuilt from
    a table of thousands of slots (asserted where the counters run)."""
    cut = len(reads) // 4
    return reads[:cut], reads[cut:]


@functools.lru_cache(maxsize=None)
def _oracle(k):
    a, b = _library()
    return uo.count_kmers_np(*uo.pack(a), k), uo.count_kmers_np(*uo.pack(b), k)


def _table_form(ranks, k):
    """The counting table's key of a canonical k-mer given as its lexicographic rank: base 0 in the low bits, the smaller of the
    two strands in THAT form (tbk_count_kernel's `key`); what tbk_class_of is taken of."""
    ranks = ranks.astype(np.uint64)
    mask = np.uint64((1 << (2 * k)) - 1) if k < 32 else np.uint64(0xFFFFFFFFFFFFFFFF)
    fwd = np.zeros(ranks.size, dtype=np.uint64)
    for j in range(k):
        fwd |= ((ranks >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)) << np.uint64(2 * j)
    return np.minimum(fwd, ranks ^ mask)  # (the reverse complement with base 0 low is the complement with base 0 high)


def test_the_library_is_what_the_trip_counts_rest_on():
    """With at most 5 blocks: 4 reads a trip of separate per block, 1 pass a trip of the counting kernel per block, 256 entries a
    trip of the database kernels per block - every batch, and every class database at passes = 3, is more than twice that."""
    a, b = _library()
    most = max(CAPS)
    for reads in (a, b):
        lengths = [len(r) for r in reads]
        assert reads[0] == reads[-1] == "" and "" in reads[len(reads) // 2 - 1:len(reads) // 2 + 2]
        assert min(lengths) == 0 and 5000 in lengths and {1, 399, 400} <= set(lengths) and max(l for l in lengths if l != 5000) == 400
        assert len(reads) > 250 and 90_000 < sum(lengths) < 110_000
        assert sum(r != r.upper() for r in reads) >= len(reads) // 20 and sum("N" in r for r in reads) > 20
        assert len(reads) > 4 * most * 2
        assert (sum(lengths) + len(reads)) // 2048 > 2 * most
        for batch in _batches(reads):
            assert len(batch) > 4 * most and (sum(map(len, batch)) + len(batch)) // 2048 > most
    for k in (15, 21, 32):
        for keys, counts in _oracle(k):
            solid = keys[counts >= 2]
            per_class = np.bincount(_class_of(_table_form(solid, k), 3).astype(np.int64), minlength=3)
            assert per_class.min() > 2 * most * 256, (k, per_class)
            assert int((counts == 1).sum()) > 1000 and int((counts >= 2).sum()) > 10_000


# ---- one run of everything, under a cap or without ---------------------------------------------------------------------------
def _text(keys, k):
    return "".join(s + "\n" for s in uo.kmer_strings(keys, k))


def _want_file(counts, reads, k, keep):
    bases = sum(map(len, reads))
    if keep:
        keys, cnt = counts
        return kf.file_bytes(k, keys, np.minimum(cnt, 255).astype(np.uint8), uo.histogram_np(cnt).astype(np.uint64), reads=len(reads), bases=bases,
                             magic=FULL_MAGIC)
    keys, cnt, hist = kf.database_of(*counts)
    return kf.file_bytes(k, keys, cnt, hist, reads=len(reads), bases=bases)


def _run(gpu, k, passes, keep, c, tmp):
    """Count both parents from capacity 16 in two batches; histogram, the three lists, the database and its file; then the files
    loaded again, the list between the loaded databases and (for full databases) their union.  c: the cap this runs under
    (0: none) - the swapped files are tried under a cap only."""
    from trio_binning_amd import kmers

    a, b = _library()
    res = {"unique": {}, "db_unique": {}, "slots": []}
    fa, fb = str(tmp / "a.tbkdb"), str(tmp / "b.tbkdb")
    with kmers.KmerCounter(k, 16, passes=passes, keep_singletons=keep) as ca, kmers.KmerCounter(k, 16, passes=passes, keep_singletons=keep) as cb:
        for counter, reads in ((ca, a), (cb, b)):
            first, rest = _batches(reads)
            counter.add_reads(first)
            before = counter.stats()["n_slots"]
            counter.add_reads(rest)
            res["slots"].append((before, counter.stats()["n_slots"]))
        res["hist"] = [int(x) for x in ca.histogram()]
        res["distinct"] = ca.stats()["distinct"]
        for lo, hi in RANGES:
            res["unique"][lo, hi] = _dump(ca, cb, lo, hi, tmp / "unique.txt")
        with ca.database() as da, cb.database() as db:
            res["floor"] = (da.floor, db.floor)
            res["entries"] = da.entries()
            res["db_hist"] = [int(x) for x in da.histogram()]
            da.save(fa)
            db.save(fb)
    res["file_a"], res["file_b"] = open(fa, "rb").read(), open(fb, "rb").read()
    with kmers.KmerDatabase.load(fa) as la, kmers.KmerDatabase.load(fb) as lb:
        res["loaded"] = la.entries()
        if keep:
            with la.union(lb) as both:
                both.save(str(tmp / "both.tbkdb"))
            res["union"] = open(tmp / "both.tbkdb", "rb").read()
    with (kmers.load_solid_database(fa) if keep else kmers.KmerDatabase.load(fa)) as la, \
            (kmers.load_solid_database(fb) if keep else kmers.KmerDatabase.load(fb)) as lb:
        for lo, hi in RANGES:
            res["db_unique"][lo, hi] = _dump(la, lb, lo, hi, tmp / "db_unique.txt")
    if c:
        # the pair that straddles the first stride of the checking kernel, and the one that straddles the second
        n = res["entries"][0].size
        for at in (c * 256 - 1, 2 * c * 256 - 1):
            assert at + 1 < n
            bad = tmp / "swapped.tbkdb"
            bad.write_bytes(_swap(res["file_a"], at))
            rc, handle, msg = _load_status(gpu, bad)
            assert rc == gpu.TBK_ERR_FORMAT and not handle and "ascending" in msg, (at, rc, msg)
    return res


_PLAIN = {}


def _unhooked(gpu, k, passes, keep):
    """_run without the hook, once for every (k, passes, keep); called before a test sets its caps"""
    if (k, passes, keep) not in _PLAIN:
        from pathlib import Path

        with tempfile.TemporaryDirectory() as tmp:
            _PLAIN[k, passes, keep] = _run(gpu, k, passes, keep, 0, Path(tmp))
    return _PLAIN[k, passes, keep]


def _same(x, y):
    if isinstance(x, tuple) and x and isinstance(x[0], np.ndarray):
        return len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    return x == y


@pytest.mark.parametrize("c", CAPS)
@pytest.mark.parametrize("keep", [False, True], ids=["solid", "full"])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("k", [15, 21, 32])
def test_capped_grids_count_what_the_oracle_counts(gpu, caps, tmp_path, k, passes, keep, c):
    """Everything the counter and its databases answer, with every strided grid of tbk_count_kernels.hip held to c blocks.

    passes = 1: separate, count, rehash, histogram, tbk_count_unique_kernel, tbk_count_export_kernel; passes = 3: retain, the class
    form of count, distil, tbk_db_unique_kernel (tbk_db_solid_keys_kernel first when B keeps its once-seen k-mers),
    tbk_db_rank_kernel; both: tbk_kmerdb_check_kernel (the loads), tbk_kmerdb_unique_kernel (the loaded databases) and, for full
    databases, tbk_kmerdb_tally_kernel (their union)."""
    a, b = _library()
    oa, ob = _oracle(k)
    plain = _unhooked(gpu, k, passes, keep)
    caps(c, c)
    got = _run(gpu, k, passes, keep, c, tmp_path)
    caps(0, 0)
    # every counter was rebuilt (tbk_count_rehash_kernel) from a table of more than 5 blocks of slots
    for before, after in got["slots"]:
        assert before > max(CAPS) * 256 and after > before, got["slots"]
    # 1. distinct count and histogram
    assert got["distinct"] == oa[0].size and got["hist"] == [int(x) for x in uo.histogram_np(oa[1])] == got["db_hist"]
    # 2. counter.unique
    for lo, hi in RANGES:
        want = uo.unique_np(oa, ob, lo, hi)
        assert want.size > 100 and got["unique"][lo, hi] == _text(want, k), (lo, hi)
    # 3. the database and its file
    keys, cnt = got["entries"]
    if keep:
        assert got["floor"] == (1, 1) and np.array_equal(keys, oa[0]) and np.array_equal(cnt, np.minimum(oa[1], 255).astype(np.uint8))
    else:
        want_keys, want_cnt, _ = kf.database_of(*oa)
        assert got["floor"] == (2, 2) and np.array_equal(keys, want_keys) and np.array_equal(cnt, want_cnt)
    assert got["file_a"] == _want_file(oa, a, k, keep) and got["file_b"] == _want_file(ob, b, k, keep)
    # 4. loaded again (the swapped files were refused in _run)
    assert np.array_equal(got["loaded"][0], keys) and np.array_equal(got["loaded"][1], cnt)
    if keep:
        assert got["union"] == _want_file(uo.add_counts_np(oa, ob), a + b, k, True)
    # 5. the list between the loaded databases
    for lo, hi in RANGES:
        assert got["db_unique"][lo, hi] == got["unique"][lo, hi], (lo, hi)
    # and byte for byte what the unhooked counter and databases gave
    for name in plain:
        if name != "slots":
            assert _same(got[name], plain[name]), name
    assert got["slots"] == plain["slots"]


# ---- unhooked: the kernels' real steps ---------------------------------------------------------------------------------------
DB_STEP = 8192 * 256  # entries that tbk_kmerdb_unique_kernel takes in one trip


@functools.lru_cache(maxsize=None)
def _crafted():
    """A: the canonical ranks of every 21-mer of the genome of tests/test_gpu_db_query_scale.py (2 199 978 of them), counter
    2 + rank % 254 - so [7, 9] selects three counters of 254, about 1 %; B: every third key of A."""
    k, n_bases = 21, 2_200_000
    rng = np.random.default_rng(2200)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n_bases).astype(np.uint8)]
    rank, clean = ref.window_ranks(genome, np.array([0, n_bases], dtype=np.uint64), k)
    assert clean[:n_bases - k + 1].all()
    ranks = np.unique(rank[:n_bases - k + 1])
    counters = (2 + ranks % np.uint64(254)).astype(np.uint8)
    return k, ranks, counters


def _crafted_file(k, keys, counters):
    hist = np.bincount(counters, minlength=256).astype(np.uint64)
    hist[0] = keys.size
    return kf.file_bytes(k, keys, counters, hist, reads=1, bases=2_200_000)


def test_database_subtraction_past_one_stride(gpu, tmp_path):
    """tbk_kmerdb_unique_kernel with its own grid on 2 199 978 entries: the wave append on a second trip, entries selected on both
    sides of 8192 x 256 and, on both sides, entries in range that B holds."""
    from trio_binning_amd import kmers

    k, ranks, counters = _crafted()
    b_keys, b_counters = ranks[::3], counters[::3]
    in_range = (counters >= 7) & (counters <= 9)
    selected = in_range & ~np.isin(ranks, b_keys, assume_unique=True)
    at = np.flatnonzero(selected)
    assert ranks.size == 2_199_978 > DB_STEP and 0.008 * ranks.size < int(in_range.sum()) < 0.015 * ranks.size and at.size > 10_000
    assert at[0] < DB_STEP - 64 and at[-1] >= DB_STEP + 64 and int((at >= DB_STEP).sum()) > 100
    held = np.flatnonzero(in_range & ~selected)
    assert held[0] < DB_STEP <= held[-1] and int((held >= DB_STEP).sum()) > 100
    (tmp_path / "a.tbkdb").write_bytes(_crafted_file(k, ranks, counters))
    (tmp_path / "b.tbkdb").write_bytes(_crafted_file(k, b_keys, b_counters))
    with kmers.KmerDatabase.load(str(tmp_path / "a.tbkdb")) as da, kmers.KmerDatabase.load(str(tmp_path / "b.tbkdb")) as db:
        assert len(da) == ranks.size and len(db) == b_keys.size
        out = str(tmp_path / "unique.txt")
        n = da.unique(db, 7, 9, out)
        got = uo.read_list_np(out, k)
        assert n == got.size == at.size and np.array_equal(got, ranks[selected])


def test_table_kernels_on_a_table_of_several_strides(gpu, tmp_path):
    """Counters of capacity 3 000 000: more than 5 000 000 slots, so tbk_count_histogram_kernel and tbk_count_export_kernel
    (4096 x 256 slots a trip) take five trips and tbk_count_unique_kernel (8192 x 256) three, with their own grids."""
    from trio_binning_amd import kmers

    k = 21
    a, b = _library()
    oa, ob = _oracle(k)
    with kmers.KmerCounter(k, 3_000_000) as ca, kmers.KmerCounter(k, 3_000_000) as cb:
        for counter, reads in ((ca, a), (cb, b)):
            for batch in _batches(reads):
                counter.add_reads(batch)
            assert counter.stats()["n_slots"] > 2 * DB_STEP
        assert ca.stats()["distinct"] == oa[0].size and [int(x) for x in ca.histogram()] == [int(x) for x in uo.histogram_np(oa[1])]
        for lo, hi in RANGES:
            assert _dump(ca, cb, lo, hi, tmp_path / "unique.txt") == _text(uo.unique_np(oa, ob, lo, hi), k), (lo, hi)
        with ca.database() as da:
            keys, cnt = da.entries()
            want_keys, want_cnt, _ = kf.database_of(*oa)
            assert np.array_equal(keys, want_keys) and np.array_equal(cnt, want_cnt)
