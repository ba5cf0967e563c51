"""Count databases (tbk_kmerdb, kmers.KmerDatabase; include/tbk.h "count databases"): what a k-mer counter leaves behind as an
object of its own - exported, saved, loaded and checked, subtracted at cut-offs the caller names - and the command line around
it (--keep-databases, --min-count-* / --max-count-*, a parent given as a *.tbkdb file).

The yardstick is oracle/unique_oracle.py: count_kmers_np gives the exact content of a database (keys = lexicographic ranks,
ascending), and the test writes the file such a database must become with numpy, struct and zlib alone (tests/kmerdb_files.py).
Libraries are made as tests/test_gpu_counter_passes.py makes them."""
import ctypes as C
import functools
import gzip
import os
import struct

import numpy as np
import pytest

import kmerdb_files as kf

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGT", "TGCA")
RANGES = ((2, 255), (3, 20), (5, 5), (1, 4), (200, 255), (0, 1000), (9, 3))


def _rc(s):
    return s.translate(COMP)[::-1]


def _library(rng, genome, n_reads, read_len, err=0.01, lower=0.0, n_rate=0.001):
    reads = []
    for _ in range(n_reads):
        p = int(rng.integers(0, len(genome) - read_len))
        s = list(genome[p:p + read_len])
        for i in np.nonzero(rng.random(read_len) < err)[0]:
            s[int(i)] = "ACGT"[int(rng.integers(0, 4))]
        for i in np.nonzero(rng.random(read_len) < n_rate)[0]:
            s[int(i)] = "N"
        r = "".join(s)
        if rng.random() < 0.5:
            r = _rc(r)
        if rng.random() < lower:
            r = r.lower()
        reads.append(r)
    return reads


def _two_parents(rng, glen, snp=1 / 200):
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, glen))
    def mutate():
        s = list(base)
        for i in np.nonzero(rng.random(glen) < snp)[0]:
            s[int(i)] = "ACGT"[(("ACGT".index(s[int(i)])) + int(rng.integers(1, 4))) % 4]
        return "".join(s)
    return mutate(), mutate()


def _random_dna(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _add_in_batches(counter, reads, cuts):
    i = j = 0
    while i < len(reads):
        step = cuts[j % len(cuts)]
        counter.add_reads(reads[i:i + step])
        i, j = i + step, j + 1


def _oracle_counts(reads, k):
    from oracle import unique_oracle as uo

    return uo.count_kmers_np(*uo.pack(reads), k)


def _oracle_file(reads, k, counts=None):
    """The bytes of the file the database of `reads` must become."""
    keys, cnt, hist = kf.database_of(*(counts or _oracle_counts(reads, k)))
    return kf.file_bytes(k, keys, cnt, hist, reads=len(reads), bases=sum(map(len, reads)))


def _oracle_db(counts, k):
    """oracle.unique_oracle.database() of numpy counts: {k-mer: capped counter} of the k-mers seen at least twice."""
    from oracle import unique_oracle as uo

    keys, cnt, _ = kf.database_of(*counts)
    return dict(zip(uo.kmer_strings(keys, k), cnt.tolist()))


def _dump(a, b, lo, hi, path):
    n = a.unique(b, lo, hi, str(path))
    text = open(path).read()
    assert text.count("\n") == n and (not text or text.endswith("\n"))
    return text


def _count(reads, k, passes=1, cuts=(250,)):
    from trio_binning_amd import kmers

    c = kmers.KmerCounter(k, 400_000, passes=passes)
    _add_in_batches(c, reads, cuts)
    return c


def _database(reads, k, passes=1, cuts=(250,)):
    with _count(reads, k, passes, cuts) as c:
        return c.database()


@functools.lru_cache(maxsize=None)
def _case(k):
    rng = np.random.default_rng(100 + k)
    ga, gb = _two_parents(rng, glen=8_000 if k > 5 else 600)
    reads_a = _library(rng, ga, 900, 150, lower=0.1) + ["", "ACGT", "N" * 40, ga[:k - 1], ga[:k], ga[:k]]
    reads_b = _library(rng, gb, 700, 150)
    na, nb = _oracle_counts(reads_a, k), _oracle_counts(reads_b, k)
    return {"a": reads_a, "b": reads_b, "na": na, "nb": nb, "dba": _oracle_db(na, k), "dbb": _oracle_db(nb, k)}


# ---- 1. content equals the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 16, 21, 31, 32])
def test_content_equals_oracle(gpu, k):
    case = _case(k)
    want_keys, want_counts, want_hist = kf.database_of(*case["na"])
    with _count(case["a"], k) as c:
        hist = c.histogram()
        with c.database() as db:
            assert db.k == k and len(db) == want_keys.size and db.device == c.device
            keys, counts = db.entries()
            assert keys.dtype == np.uint64 and counts.dtype == np.uint8
            assert (keys[1:] > keys[:-1]).all()
            assert np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts)
            assert db.histogram().tolist() == hist.tolist() == want_hist.tolist()
            st = db.stats()
            assert st == {"reads_added": len(case["a"]), "bases_added": sum(map(len, case["a"])), "bytes": 9 * want_keys.size}
            # a window of the entries, and the edges of the range
            part = db.entries(3, 5)
            assert np.array_equal(part[0], want_keys[3:8]) and np.array_equal(part[1], want_counts[3:8])
            assert db.entries(len(db))[0].size == 0
            with pytest.raises(ValueError):
                db.entries(len(db) - 1, 2)


# ---- 2. the same database from every route ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 21, 32])
def test_same_file_from_every_route(gpu, tmp_path, k):
    case = _case(k)
    want = _oracle_file(case["a"], k, case["na"])
    for passes, cuts in ((1, (250, 1, 333, 97, 225)), (2, (300, 123)), (7, (1000,))):
        path = tmp_path / f"p{passes}.tbkdb"
        with _database(case["a"], k, passes, cuts) as db:
            db.save(str(path))
        assert not os.path.exists(str(path) + ".tmp")
        got = path.read_bytes()
        assert len(got) == 2096 + 9 * struct.unpack_from("<Q", got, 16)[0]
        assert got == want, f"passes = {passes}: the saved file differs from the one written from the oracle's arrays"


# ---- 3. round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32])
def test_round_trip_and_unique(gpu, tmp_path, k):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    case = _case(k)
    with _count(case["a"], k) as ca, _count(case["b"], k) as cb:
        live = {r: (_dump(ca, cb, r[0], r[1], tmp_path / "live_a.txt"), _dump(cb, ca, r[0], r[1], tmp_path / "live_b.txt")) for r in RANGES}
        with ca.database() as da, cb.database() as db:
            da.save(str(tmp_path / "a.tbkdb"))
            db.save(str(tmp_path / "b.tbkdb"))
    first = (tmp_path / "a.tbkdb").read_bytes()
    with kmers.KmerDatabase.load(str(tmp_path / "a.tbkdb")) as da, kmers.KmerDatabase.load(str(tmp_path / "b.tbkdb")) as db, \
            kmers.KmerCounter(k, 1000) as nothing:
        da.save(str(tmp_path / "a2.tbkdb"))
        assert (tmp_path / "a2.tbkdb").read_bytes() == first
        assert da.histogram().tolist() == kf.database_of(*case["na"])[2].tolist()
        for lo, hi in RANGES:
            text_a, text_b = _dump(da, db, lo, hi, tmp_path / "a.txt"), _dump(db, da, lo, hi, tmp_path / "b.txt")
            assert (text_a, text_b) == live[(lo, hi)]
            assert text_a.split("\n")[:-1] == uo.unique_kmers(case["dba"], case["dbb"], lo, hi)
            assert text_b.split("\n")[:-1] == uo.unique_kmers(case["dbb"], case["dba"], lo, hi)
        assert live[(9, 3)] == ("", "") and len(live[(2, 255)][0]) > 100 * (k + 1)
        assert _dump(da, da, 2, 255, tmp_path / "self.txt") == ""
        with nothing.database() as empty:
            assert len(empty) == 0
            assert _dump(da, empty, 3, 20, tmp_path / "all.txt").split("\n")[:-1] == uo.unique_kmers(case["dba"], {}, 3, 20)
            assert _dump(empty, da, 2, 255, tmp_path / "none.txt") == ""


# ---- 4. export does not disturb a one-pass counter --------------------------------------------------------------
def test_export_leaves_a_one_pass_counter_as_it_was(gpu, tmp_path):
    from trio_binning_amd import _lib

    k = 21
    case = _case(k)
    with _count(case["a"], k) as ca, _count(case["b"], k) as cb:
        before = (ca.histogram().tolist(), ca.stats()["distinct"], _dump(ca, cb, 2, 255, tmp_path / "x.txt"), _dump(cb, ca, 3, 20, tmp_path / "y.txt"))
        with ca.database() as da, ca.database() as again:  # twice: the second reads the same table
            assert np.array_equal(da.entries()[0], again.entries()[0]) and np.array_equal(da.entries()[1], again.entries()[1])
            after = (ca.histogram().tolist(), ca.stats()["distinct"], _dump(ca, cb, 2, 255, tmp_path / "x.txt"), _dump(cb, ca, 3, 20, tmp_path / "y.txt"))
            assert after == before
        # exporting finishes the counter
        bases, offsets = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTA", dtype=np.uint8), np.array([0, 25], dtype=np.uint64)
        rc = _lib.lib.tbk_counter_add_batch(ca._h, bases.ctypes.data, offsets.ctypes.data, 1)
        assert rc == _lib.TBK_ERR_INVALID and "finished" in _lib.last_error()
        assert ca.stats()["finished"] and ca.histogram().tolist() == before[0]


# ---- 5. saturation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [1, 3])
def test_counter_past_255_is_stored_as_255(gpu, passes):
    reads = ["A" * 200, "a" * 150, "ACGTTGCATT", "ACGTTGCATT"]  # AAAAA 342 times; the 5-mers of the last read twice
    with _database(reads, 5, passes) as db:
        keys, counts = db.entries()
        want_keys, want_counts, want_hist = kf.database_of(*_oracle_counts(reads, 5))
        assert np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts)
        assert int(keys[0]) == 0 and int(counts[0]) == 255 and int(db.histogram()[255]) == 1
        assert db.histogram().tolist() == want_hist.tolist()


# ---- 6. sizes at which kernels go wrong ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_tiny_databases(gpu, tmp_path, n):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    k = 21
    r = _random_dna(np.random.default_rng(9), 100)
    reads = [r] + ([r[:k + n - 1]] if n else [])  # the first n k-mers of r a second time
    want = _oracle_file(reads, k)
    path = tmp_path / "tiny.tbkdb"
    with _database(reads, k) as db:
        assert len(db) == n
        db.save(str(path))
    assert path.read_bytes() == want and len(want) == 2096 + 9 * n
    assert kmers.database_file_info(str(path))["n"] == n
    with kmers.KmerDatabase.load(str(path)) as db, kmers.KmerCounter(k, 1000) as nothing, nothing.database() as empty:
        assert len(db) == n and db.entries()[0].size == n
        text = _dump(db, empty, 2, 255, tmp_path / "all.txt")
        assert text.split("\n")[:-1] == uo.kmer_strings(kf.database_of(*_oracle_counts(reads, k))[0], k)
        assert _dump(db, db, 2, 255, tmp_path / "self.txt") == ""


@functools.lru_cache(maxsize=None)
def _large():
    """About 3e5 keys: a 300 kb random genome (one of 200 kb holds 2e5 21-mers at the most) read in pieces of 1 kb that overlap
    by k - 1, every piece counted twice; the partner is its first half.  More than 256 blocks of 256 keys, more than the 1024
    blocks of the checking kernel's grid, several tiles of the radix sort.  The files are made once, from the library."""
    k = 21
    g = _random_dna(np.random.default_rng(31), 300_000)
    reads = [g[i:i + 1000 + k - 1] for i in range(0, len(g), 1000)] * 2
    half = reads[:150] * 2
    counts, counts_half = _oracle_counts(reads, k), _oracle_counts(half, k)
    with _database(reads, k, cuts=(170,)) as db:
        keys, cnt = db.entries()
        hist = db.histogram()
    return {"k": k, "reads": reads, "half": half, "counts": counts, "counts_half": counts_half, "keys": keys, "cnt": cnt, "hist": hist}


def test_large_database(gpu, tmp_path):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    big = _large()
    k = big["k"]
    want_keys, want_counts, want_hist = kf.database_of(*big["counts"])
    assert want_keys.size > 290_000
    assert np.array_equal(big["keys"], want_keys) and np.array_equal(big["cnt"], want_counts) and big["hist"].tolist() == want_hist.tolist()
    with _database(big["reads"], k, passes=3, cuts=(211,)) as db, _database(big["half"], k) as dh:
        db.save(str(tmp_path / "big.tbkdb"))
        dh.save(str(tmp_path / "half.tbkdb"))
    assert (tmp_path / "big.tbkdb").read_bytes() == _oracle_file(big["reads"], k, big["counts"])
    with kmers.KmerDatabase.load(str(tmp_path / "big.tbkdb")) as db, kmers.KmerDatabase.load(str(tmp_path / "half.tbkdb")) as dh:
        assert np.array_equal(db.entries()[0], want_keys)
        for lo, hi in ((2, 255), (3, 255)):
            text = _dump(db, dh, lo, hi, tmp_path / "u.txt")
            want = uo.unique_np(big["counts"], big["counts_half"], lo, hi)
            assert text.split("\n")[:-1] == uo.kmer_strings(want, k)
        assert uo.unique_np(big["counts"], big["counts_half"], 2, 255).size > 100_000
        assert _dump(dh, db, 2, 255, tmp_path / "none.txt") == ""


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _files():
    """The sound k = 21 files of the two libraries, as the oracle's arrays give them (test_same_file_from_every_route holds the
    library's own files to exactly these bytes)."""
    case = _case(21)
    return _oracle_file(case["a"], 21, case["na"]), _oracle_file(case["b"], 21, case["nb"])


def _keys_at(data, i):
    return 2096 + 8 * i


def _swap(data, i):
    """keys i and i + 1 exchanged"""
    at = _keys_at(data, i)
    return kf.patched(data, at, data[at + 8:at + 16] + data[at:at + 8])


@functools.lru_cache(maxsize=None)
def _small_damage():
    data = _files()[0]
    n = struct.unpack_from("<Q", data, 16)[0]
    counters = 2096 + 8 * n
    hist = list(struct.unpack_from("<256Q", data, 40))
    assert hist[2] >= 1 and n > 1000
    moved = kf.with_crc(kf.patched(data, 40 + 16, struct.pack("<QQ", hist[2] - 1, hist[3] + 1)))  # rows still sum to n
    last = struct.unpack_from("<Q", data, _keys_at(data, n - 1))[0]
    assert last < 1 << 42
    return dict(kf.header_refusals(data) + [
        ("truncated_in_keys", data[:2096 + 8 * 100 + 3]),
        ("truncated_in_counters", data[:-7]),
        ("tallies_disagree", moved),
        ("counter_0", kf.patched(data, counters + 77, b"\0")),
        ("counter_1", kf.patched(data, counters + n - 1, b"\1")),
        ("equal_neighbours", kf.patched(data, _keys_at(data, 500), data[_keys_at(data, 499):_keys_at(data, 500)])),
        ("swapped_at_0", _swap(data, 0)),
        ("swapped_at_the_end", _swap(data, n - 2)),
        ("bit_42_set", kf.patched(data, _keys_at(data, n - 1), struct.pack("<Q", last | 1 << 42))),  # (still the largest key: only the bits give it away)
    ])


_SMALL = ["truncated_in_header", "one_byte_too_many", "wrong_magic", "wrong_header_size", "k_0", "k_33", "header_byte_flipped", "n_changed",
          "rows_do_not_sum_to_n", "row_0_too_small", "pad_not_zero", "truncated_in_keys", "truncated_in_counters", "tallies_disagree",
          "counter_0", "counter_1", "equal_neighbours", "swapped_at_0", "swapped_at_the_end", "bit_42_set"]


def _load_status(_lib, path):
    h = C.c_void_p()
    rc = _lib.lib.tbk_kmerdb_load(str(path).encode(), 0, C.byref(h))
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib.tbk_kmerdb_destroy(h)
    return rc, h.value, _lib.last_error()


def _good_load_and_unique(tmp_path):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    case = _case(21)
    (tmp_path / "good_a.tbkdb").write_bytes(_files()[0])
    (tmp_path / "good_b.tbkdb").write_bytes(_files()[1])
    with kmers.KmerDatabase.load(str(tmp_path / "good_a.tbkdb")) as da, kmers.KmerDatabase.load(str(tmp_path / "good_b.tbkdb")) as db:
        assert _dump(da, db, 3, 20, tmp_path / "good.txt").split("\n")[:-1] == uo.unique_kmers(case["dba"], case["dbb"], 3, 20)


@pytest.mark.parametrize("name", _SMALL)
def test_damaged_file_is_refused(gpu, tmp_path, name):
    damage = _small_damage()
    assert sorted(damage) == sorted(_SMALL)
    bad = tmp_path / (name + ".tbkdb")
    bad.write_bytes(damage[name])
    rc, handle, msg = _load_status(gpu, bad)
    assert rc == gpu.TBK_ERR_FORMAT and not handle and name + ".tbkdb" in msg, (rc, msg)
    _good_load_and_unique(tmp_path)


@pytest.mark.parametrize("at", [255, 65535, 262143])
def test_swapped_keys_across_a_block_boundary_are_refused(gpu, tmp_path, at):
    """keys `at` and `at + 1` of the large file exchanged: the pair straddles two blocks of the checking kernel (and 65535 | 65536
    lies past the first 256 blocks, 262143 | 262144 where the grid of 1024 blocks starts over), every other neighbour pair is in order."""
    big = _large()
    data = kf.file_bytes(big["k"], big["keys"], big["cnt"], big["hist"], reads=len(big["reads"]), bases=sum(map(len, big["reads"])))
    assert data == _oracle_file(big["reads"], big["k"], big["counts"])
    good, bad = tmp_path / "big.tbkdb", tmp_path / "swapped.tbkdb"
    good.write_bytes(data)
    bad.write_bytes(_swap(data, at))
    rc, handle, msg = _load_status(gpu, bad)
    assert rc == gpu.TBK_ERR_FORMAT and not handle and "ascending" in msg, (rc, msg)
    assert _load_status(gpu, good)[0] == gpu.TBK_OK
    _good_load_and_unique(tmp_path)


def test_missing_file_and_mismatched_databases(gpu, tmp_path):
    from trio_binning_amd import kmers

    rc, handle, msg = _load_status(gpu, tmp_path / "absent.tbkdb")
    assert rc == gpu.TBK_ERR_IO and not handle and "absent.tbkdb" in msg
    with pytest.raises(IOError):
        kmers.KmerDatabase.load(str(tmp_path / "absent.tbkdb"))
    _good_load_and_unique(tmp_path)
    with _database(_case(21)["a"][:50], 21) as d21, _database(_case(31)["a"][:50], 31) as d31:
        n = C.c_uint64(5)
        rc = gpu.lib.tbk_kmerdb_unique(d21._h, d31._h, 2, 255, str(tmp_path / "no.txt").encode(), C.byref(n))
        assert rc == gpu.TBK_ERR_INVALID and "different k" in gpu.last_error()
        assert not os.path.exists(tmp_path / "no.txt")


# ---- 8. the command line ---------------------------------------------------------------------------------------------
def _fastq(path, reads, gz=False):
    text = "".join(f"@r{i} x\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads))
    with (gzip.open if gz else open)(path, "wt") as fh:
        fh.write(text)
    return str(path)


def _outputs(out, scratch):
    return {name: open(os.path.join(d, name), "rb").read()
            for d, name in ((out, "hapA_only_kmers.txt"), (out, "hapB_only_kmers.txt"), (scratch, "haplotypeA.histogram"), (scratch, "haplotypeB.histogram"))}


def _cutoffs(err):
    import re

    found = re.findall(r"Using counts in range \[(\d+),(\d+)\]", err)
    assert len(found) == 2, err
    return [tuple(map(int, f)) for f in found]


def test_cli_every_route_writes_the_same_files(gpu, tmp_path, capsys):
    from oracle import unique_oracle as uo
    from trio_binning_amd import find_unique_kmers as fu

    k = 21
    rng = np.random.default_rng(277)  # (the reference's rule gives both parents [5,35] here: some 4000 k-mers in each list)
    ga, gb = _two_parents(rng, glen=20_000)
    reads_a, reads_b = _library(rng, ga, 3500, 150), _library(rng, gb, 3500, 150)
    fa = _fastq(tmp_path / "a1.fastq", reads_a[:2000]) + "," + _fastq(tmp_path / "a2.fastq.gz", reads_a[2000:], gz=True)
    fb = _fastq(tmp_path / "b.fastq", reads_b)
    dirs = {}
    for name in ("plain", "keep", "files", "mixed"):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
    common = lambda name: ["-k", str(k), "-o", str(dirs[name]), "-s", str(dirs[name]), "--capacity", "1500000"]
    # (a) today's path, then the same keeping the databases
    fu.main(common("plain") + [fa, fb])
    (min_a, max_a), (min_b, max_b) = _cutoffs(capsys.readouterr().err)
    plain = _outputs(dirs["plain"], dirs["plain"])
    assert not [f for f in os.listdir(dirs["plain"]) if f.endswith(".tbkdb")]
    dba, dbb = _oracle_db(_oracle_counts(reads_a, k), k), _oracle_db(_oracle_counts(reads_b, k), k)
    assert plain["hapA_only_kmers.txt"].decode().split() == uo.unique_kmers(dba, dbb, min_a, max_a) and len(plain["hapA_only_kmers.txt"]) > 1000
    assert plain["hapB_only_kmers.txt"].decode().split() == uo.unique_kmers(dbb, dba, min_b, max_b) and len(plain["hapB_only_kmers.txt"]) > 1000
    fu.main(common("keep") + ["--keep-databases", fa, fb])
    assert _cutoffs(capsys.readouterr().err) == [(min_a, max_a), (min_b, max_b)]
    assert _outputs(dirs["keep"], dirs["keep"]) == plain
    kept_a, kept_b = str(dirs["keep"] / "haplotypeA.tbkdb"), str(dirs["keep"] / "haplotypeB.tbkdb")
    assert open(kept_a, "rb").read() == _oracle_file(reads_a, k) and os.path.isfile(kept_b)
    # (c) one parent from its file, the other counted in three passes
    fu.main(common("mixed") + ["--passes", "3", kept_a, fb])
    err = capsys.readouterr().err
    assert _cutoffs(err) == [(min_a, max_a), (min_b, max_b)] and "Loading the k-mer database of haplotype A" in err
    assert _outputs(dirs["mixed"], dirs["mixed"]) == plain
    # (a) again: from the two files alone, the read files gone, the first run's cut-offs given by hand
    for p in (fa + "," + fb).split(","):
        os.remove(p)
    fu.main(common("files") + ["--min-count-a", str(min_a), "--max-count-a", str(max_a), "--min-count-b", str(min_b), "--max-count-b", str(max_b),
                               kept_a, kept_b])
    err = capsys.readouterr().err
    assert _cutoffs(err) == [(min_a, max_a), (min_b, max_b)] and "WARNING" not in err
    assert _outputs(dirs["files"], dirs["files"]) == plain
    # (d) a database of another k, or half a pair of cut-offs: a message, and nothing is counted
    with _database(reads_a[:200], 16) as d16:
        d16.save(str(tmp_path / "k16.tbkdb"))
    with pytest.raises(SystemExit) as ei:
        fu.main(common("files") + [str(tmp_path / "k16.tbkdb"), kept_b])
    assert "16-mers" in str(ei.value.code)
    with pytest.raises(SystemExit):
        fu.main(common("files") + ["--min-count-a", "3", kept_a, kept_b])
    assert "--min-count-a and --max-count-a go together" in capsys.readouterr().err
    assert _outputs(dirs["files"], dirs["files"]) == plain


def test_cli_keeps_the_databases_when_no_cutoffs_are_found(gpu, tmp_path, capsys):
    """Both parents at about 3x: the histograms fall from row 2 on, the reference's rule finds no minimum.  With --keep-databases
    the error comes only once both databases are on disk, stderr says where they are and how to dump again, and doing so works."""
    from oracle import unique_oracle as uo
    from trio_binning_amd import find_unique_kmers as fu

    k = 21
    rng = np.random.default_rng(79)
    ga, gb = _two_parents(rng, glen=20_000)
    reads_a, reads_b = _library(rng, ga, 400, 150), _library(rng, gb, 400, 150)
    dba, dbb = _oracle_db(_oracle_counts(reads_a, k), k), _oracle_db(_oracle_counts(reads_b, k), k)
    for db in (dba, dbb):
        with pytest.raises(uo.HistogramError):
            uo.analyze_histogram_rows(uo.histogram_rows(db))
    fa, fb = _fastq(tmp_path / "a.fastq.gz", reads_a, gz=True), _fastq(tmp_path / "b.fastq", reads_b)
    out = tmp_path / "out"
    out.mkdir()
    common = ["-k", str(k), "-o", str(out), "-s", str(tmp_path), "--capacity", "500000"]
    kept_a, kept_b = str(out / "haplotypeA.tbkdb"), str(out / "haplotypeB.tbkdb")
    seen = []

    def analyze(rows, histogram_path=""):
        seen.append((histogram_path, os.path.isfile(kept_a), os.path.isfile(kept_b)))
        return real(rows, histogram_path)

    real, fu.analyze_histogram = fu.analyze_histogram, analyze
    try:
        with pytest.raises(fu.HistogramError) as ei:
            fu.main(common + ["--keep-databases", fa, fb])
    finally:
        fu.analyze_histogram = real
    # A's failure was held back: B was still counted and analyzed, each after its database was on disk
    assert [s[1:] for s in seen] == [(True, False), (True, True)]
    assert str(ei.value) == fu.HistogramError(str(tmp_path / "haplotypeA.histogram")).message
    err = capsys.readouterr().err
    assert kept_a in err and kept_b in err and "--min-count-a MIN --max-count-a MAX --min-count-b MIN --max-count-b MAX" in err
    assert not os.path.exists(out / "hapA_only_kmers.txt")
    assert open(kept_a, "rb").read() == _oracle_file(reads_a, k) and open(kept_b, "rb").read() == _oracle_file(reads_b, k)
    # without the option the first parent's error ends the run at once, as ever
    with pytest.raises(fu.HistogramError):
        fu.main(common + [fa, fb])
    capsys.readouterr()
    os.remove(fa)
    os.remove(fb)
    fu.main(common + ["--min-count-a", "2", "--max-count-a", "6", "--min-count-b", "3", "--max-count-b", "255", kept_a, kept_b])
    err = capsys.readouterr().err
    assert "Using counts in range [2,6]" in err and "Using counts in range [3,255]" in err and "WARNING" not in err
    assert open(out / "hapA_only_kmers.txt").read().split() == uo.unique_kmers(dba, dbb, 2, 6)
    assert open(out / "hapB_only_kmers.txt").read().split() == uo.unique_kmers(dbb, dba, 3, 255)
    assert len(uo.unique_kmers(dba, dbb, 2, 6)) > 50
