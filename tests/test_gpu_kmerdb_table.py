"""Two count databases straight to a k-mer list in HBM (tbk_kmerdb_unique_table, kmers.KmerDatabase.unique_set) and the command
line on top of it (classify-by-kmers reads.fq haplotypeA.tbkdb haplotypeB.tbkdb).

The list must be what tbk_kmerdb_unique would write and create_kmer_hash_set would read back: the same keys, in the same -
lexicographic - order.  For crafted databases (tests/kmerdb_files.py) the expected keys come from numpy alone: the range
mask, ~np.isin against the partner's ranks, and rank -> packed key base by base.  Sizes sit on both sides of a wave (64), a
block round (256) and a tile of the compaction (1024 entries: TBK_DBT_TILE in csrc/tbk_compact_host.h); the launches take
one block per tile, so there is no grid stride to wrap - a database of several hundred tiles stands in for it.  Counted
libraries are those of tests/test_gpu_kmerdb.py; their lists are checked against the text route and the CPU oracle."""
import gzip
import os
from unittest.mock import patch

import numpy as np
import pytest

import kmerdb_files as kf
from test_gpu_kmerdb import RANGES, _case, _database, _fastq, _library, _rc, _two_parents

pytestmark = pytest.mark.gpu

TILE = 1024
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 293 * TILE + 3)
KS = (2, 5, 16, 17, 21, 31, 32)
EDGE = 4          # ranks kept free below and above A's for the partners that lie wholly below / above it
B_KINDS = ("disjoint", "every_second", "first_and_last", "below", "above", "equal")


def _room(k):
    """ranks A and its interleaved partner may use: EDGE .. 4^k - EDGE - 1"""
    return (1 << (2 * k)) - 2 * EDGE


def _cases():
    """every k at every size it has room for (the several-hundred-tile database at k = 21 and 32 only), and the fullest k = 2 and 5 allow"""
    return [(k, n) for k in KS for n in SIZES if 2 * n <= _room(k) and (n < 100 * TILE or k in (21, 32))] + [(2, 4), (5, 500)]


def packed_keys(ranks, k):
    """rank (base 0 in the top bits of the 2k) -> key (base i at bits 2i..2i+1), base by base"""
    ranks = np.asarray(ranks, dtype=np.uint64)
    out = np.zeros_like(ranks)
    for i in range(k):
        out |= ((ranks >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)) << np.uint64(2 * i)
    return out


def _distinct_ranks(rng, k, m):
    """m distinct ranks in EDGE .. 4^k - EDGE - 1, ascending; for k = 32 they spread over all 64 bits"""
    room = _room(k)
    if room <= 1 << 22:
        got = rng.choice(room, size=m, replace=False).astype(np.uint64)
    else:
        got = np.zeros(0, dtype=np.uint64)
        while got.size < m:
            got = np.unique(np.concatenate([got, rng.integers(0, room, size=m + m // 8 + 16, dtype=np.uint64)]))
        got = rng.permutation(got)[:m]
    return np.sort(got) + np.uint64(EDGE)


def _counters(rng, n):
    """2..255, half of them among the small values the narrow ranges select"""
    return np.where(rng.random(n) < 0.5, rng.integers(2, 25, n), rng.integers(2, 256, n)).astype(np.uint8)


def _write_db(path, k, keys, counts):
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 3
    hist[0] = keys.size + 3
    with open(path, "wb") as fh:
        fh.write(kf.file_bytes(k, keys, counts, hist, reads=1, bases=k))
    return str(path)


def _partners(rng, k, a, rest):
    top = (1 << (2 * k)) - 1
    low = np.array([0, 1, 3], dtype=np.uint64)
    return {
        "disjoint": rest,
        "every_second": a[::2],
        "first_and_last": np.unique(a[[0, -1]]),
        "below": low,
        "above": np.uint64(top) - low[::-1],
        "equal": a,
    }


def _expected(a, ca, absent, lo, hi, k):
    """absent = ~np.isin(a, b): the entries of A the partner does not hold"""
    mask = (ca >= max(2, lo)) & (ca <= min(255, hi)) & absent
    return packed_keys(a[mask], k)


def _check_set(da, db, lo, hi, want, k, what):
    if want.size == 0:
        with pytest.raises(ValueError, match="empty k-mer list"):
            da.unique_set(db, lo, hi)
        return
    with da.unique_set(db, lo, hi) as hs:
        assert (hs.num_kmers, hs.k, hs.device, hs.origin) == (want.size, k, da.device, "databases"), what
        got = hs.keys()
        assert got.dtype == np.uint64 and np.array_equal(got, want), (what, int(np.argmax(got != want)) if got.size == want.size else got.size)


# the cases that also go through today's route: the dump as text, then the list parser and the list loader
TEXT_ROUTE = {(21, 3 * TILE + 17): "every_second", (32, TILE + 1): "disjoint", (5, 65): "first_and_last"}


@pytest.mark.parametrize("k,n_a", _cases())
def test_crafted_databases(gpu, tmp_path, k, n_a):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(1000 * k + n_a)
    both = _distinct_ranks(rng, k, 2 * n_a)
    pick = np.zeros(2 * n_a, dtype=bool)
    pick[rng.permutation(2 * n_a)[:n_a]] = True
    a, rest = both[pick], both[~pick]
    ca = _counters(rng, n_a)
    assert (a[1:] > a[:-1]).all() and int(a[0]) >= EDGE and int(a[-1]) <= (1 << (2 * k)) - 1 - EDGE
    if k == 32 and n_a >= 63:
        assert int(a[-1]) >> 63 == 1 and int(a[0]) >> 63 == 0
    seen = {"sets": 0, "empty": 0}
    with kmers.KmerDatabase.load(_write_db(tmp_path / "a.tbkdb", k, a, ca)) as da:
        for kind, b in _partners(rng, k, a, rest).items():
            with kmers.KmerDatabase.load(_write_db(tmp_path / (kind + ".tbkdb"), k, b, _counters(rng, b.size))) as db:
                absent = ~np.isin(a, b)
                for lo, hi in RANGES:
                    want = _expected(a, ca, absent, lo, hi, k)
                    assert kind != "equal" and (lo, hi) != (9, 3) or want.size == 0
                    seen["empty" if want.size == 0 else "sets"] += 1
                    _check_set(da, db, lo, hi, want, k, (kind, lo, hi))
                if TEXT_ROUTE.get((k, n_a)) == kind:
                    for lo, hi in ((2, 255), (3, 20)):
                        path = str(tmp_path / "dump.txt")
                        n = da.unique(db, lo, hi, path)
                        keys, k_text = kmers.parse_kmer_list(path)
                        with da.unique_set(db, lo, hi) as hs, kmers.HashSet.from_file(path) as from_text:
                            assert n == hs.num_kmers == from_text.num_kmers > 0 and k_text == hs.k == from_text.k == k
                            assert np.array_equal(hs.keys(), keys) and np.array_equal(from_text.keys(), keys)
                # the databases are as they were
                assert np.array_equal(da.entries()[0], a) and np.array_equal(da.entries()[1], ca) and np.array_equal(db.entries()[0], b)
    assert seen["empty"] >= len(RANGES) + len(B_KINDS) - 1 and (seen["sets"] > 0 or n_a == 1)


def test_a_tile_selected_whole_and_its_neighbours_not_at_all(gpu, tmp_path):
    """Tile 1 of four (entries 1024 .. 2047) holds the only counters 7, the others 9: [7,7] takes every entry of that tile and
    none of its neighbours', [9,9] the reverse, and one entry on either side of each edge moves with its counter."""
    from trio_binning_amd import kmers

    k, n = 21, 3 * TILE + 17
    rng = np.random.default_rng(5)
    a = _distinct_ranks(rng, k, n)
    b = np.array([1, 2], dtype=np.uint64)
    db_path = _write_db(tmp_path / "b.tbkdb", k, b, _counters(rng, 2))
    for first, last in ((TILE, 2 * TILE), (TILE - 1, 2 * TILE), (TILE, 2 * TILE + 1), (TILE + 1, 2 * TILE - 1), (0, TILE), (3 * TILE, n)):
        ca = np.full(n, 9, dtype=np.uint8)
        ca[first:last] = 7
        with kmers.KmerDatabase.load(_write_db(tmp_path / "a.tbkdb", k, a, ca)) as da, kmers.KmerDatabase.load(db_path) as db:
            _check_set(da, db, 7, 7, packed_keys(a[first:last], k), k, (first, last, 7))
            _check_set(da, db, 9, 9, packed_keys(np.concatenate([a[:first], a[last:]]), k), k, (first, last, 9))
            _check_set(da, db, 7, 9, packed_keys(a, k), k, (first, last, "all"))
            _check_set(da, db, 8, 8, np.zeros(0, dtype=np.uint64), k, (first, last, "none"))


def test_refusals_leave_no_table(gpu, tmp_path):
    import ctypes as C

    from trio_binning_amd import kmers

    rng = np.random.default_rng(6)
    a21, a16 = _distinct_ranks(rng, 21, 100), _distinct_ranks(rng, 16, 100)
    with kmers.KmerDatabase.load(_write_db(tmp_path / "a21.tbkdb", 21, a21, _counters(rng, 100))) as d21, \
            kmers.KmerDatabase.load(_write_db(tmp_path / "a16.tbkdb", 16, a16, _counters(rng, 100))) as d16:
        h = C.c_void_p(1)
        rc = gpu.lib.tbk_kmerdb_unique_table(d21._h, d16._h, 2, 255, C.byref(h))
        assert rc == gpu.TBK_ERR_INVALID and "different k" in gpu.last_error() and not h.value
        h = C.c_void_p(1)
        rc = gpu.lib.tbk_kmerdb_unique_table(d21._h, d21._h, 2, 255, C.byref(h))
        assert rc == gpu.TBK_ERR_FORMAT and "empty k-mer list" in gpu.last_error() and not h.value
        assert gpu.lib.tbk_kmerdb_unique_table(d21._h, None, 2, 255, C.byref(h)) == gpu.TBK_ERR_INVALID
        with pytest.raises(ValueError, match="different k"):
            d16.unique_set(d21, 2, 255)
        # a partner that holds nothing takes nothing away; nothing minus something is the empty list
        with kmers.KmerDatabase.load(_write_db(tmp_path / "none.tbkdb", 16, a16[:0], np.zeros(0, dtype=np.uint8))) as none:
            with d16.unique_set(none, 2, 255) as hs:
                assert np.array_equal(hs.keys(), packed_keys(a16, 16))
            with pytest.raises(ValueError, match="empty k-mer list"):
                none.unique_set(d16, 2, 255)


# ---- counted libraries: the list classifies as the text route's does, and as the oracle says ----------------------------
def _offspring(k, n=40):
    """reads of both parents' genomes (those _case(k) counted), both strands, some N, and the short ones around k"""
    rng = np.random.default_rng(100 + k)
    ga, gb = _two_parents(rng, glen=8_000 if k > 5 else 600)
    rng = np.random.default_rng(500 + k)
    reads = []
    for i in range(n):
        g = (ga, gb)[i % 2]
        length = int(rng.integers(k, min(len(g), 900)))
        p = int(rng.integers(0, len(g) - length + 1))
        s = list(g[p:p + length])
        if i % 5 == 0:
            for j in rng.integers(0, length, 3):
                s[int(j)] = "N"
        s = "".join(s)
        reads.append(_rc(s) if rng.random() < 0.5 else s)
    return reads + ["", ga[:k - 1], ga[:k], "N" * (2 * k)]


@pytest.mark.parametrize("k", [5, 21, 32])
def test_counted_libraries_classify_as_the_text_lists_do(gpu, orc, tmp_path, k):
    """List A is A minus B at [2,255]; list B is B minus A at [3,200].  At k = 5 each is taken minus the database of the other
    parent's first five reads: both full libraries hold nearly every 5-mer there is, so B minus A is empty and A minus B is
    four 5-mers that sequencing errors made and no read of either genome has - the counts would be all zero."""
    from trio_binning_amd import kmers

    case = _case(k)
    bases, offsets = kmers.pack_reads(_offspring(k))
    fa, fb = str(tmp_path / "a.txt"), str(tmp_path / "b.txt")
    part = slice(None) if k > 5 else slice(5)
    with _database(case["a"], k) as da, _database(case["b"], k) as db, \
            _database(case["b"][part], k) as minus_b, _database(case["a"][part], k) as minus_a:
        assert da.unique(minus_b, 2, 255, fa) > 0 and db.unique(minus_a, 3, 200, fb) > 0
        direct = (da.unique_set(minus_b, 2, 255), db.unique_set(minus_a, 3, 200))
    text = (kmers.HashSet.from_file(fa), kmers.HashSet.from_file(fb))
    try:
        for d, t in zip(direct, text):
            assert (d.num_kmers, d.k) == (t.num_kmers, t.k) and np.array_equal(d.keys(), t.keys())
        with kmers.Classifier(*direct) as cls:
            got = cls.classify_batch(bases, offsets)
        with kmers.Classifier(*text) as cls:
            by_text = cls.classify_batch(bases, offsets)
    finally:
        for hs in direct + text:
            hs.close()
    want = orc.count_batch(bases, offsets, orc.table_from_file(fa), orc.table_from_file(fb))
    assert np.array_equal(got, by_text) and np.array_equal(got, want)
    assert (want.sum(axis=0) > 0).all()


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio(gpu, tmp_path_factory):
    """The library of test_gpu_kmerdb.test_cli_every_route_writes_the_same_files (the reference's rule finds [5,35] for both
    parents), counted once with --keep-databases; an offspring FASTQ of reads from both parents' genomes."""
    from trio_binning_amd import find_unique_kmers as fu

    root = tmp_path_factory.mktemp("trio")
    k = 21
    rng = np.random.default_rng(277)
    ga, gb = _two_parents(rng, glen=20_000)
    reads_a, reads_b = _library(rng, ga, 3500, 150), _library(rng, gb, 3500, 150)
    fa, fb = _fastq(root / "a.fastq", reads_a), _fastq(root / "b.fastq.gz", reads_b, gz=True)
    out = root / "lists"
    out.mkdir()
    fu.main(["-k", str(k), "-o", str(out), "-s", str(out), "--capacity", "1500000", "--keep-databases", fa, fb])
    rng = np.random.default_rng(278)
    child = []
    for i in range(60):
        g = (ga, gb)[i % 2]
        length = int(rng.integers(100, 3000))
        p = int(rng.integers(0, len(g) - length))
        s = g[p:p + length]
        child.append(_rc(s) if i % 3 == 0 else s)
    child += [ga[:500] + gb[500:1000], "ACGT" * 10, "N" * 50]
    return {"k": k, "root": root, "reads": _fastq(root / "child.fastq", child),
            "list_a": str(out / "hapA_only_kmers.txt"), "list_b": str(out / "hapB_only_kmers.txt"),
            "db_a": str(out / "haplotypeA.tbkdb"), "db_b": str(out / "haplotypeB.tbkdb")}


def _classify(argv, out_dir, capsys):
    """One run of the driver: (stdout, stderr, {bin file: decompressed bytes})."""
    from trio_binning_amd.classify_by_kmers import main

    out_dir.mkdir()
    prefixes = ["--haplotype-a-out-prefix", str(out_dir / "hapA"), "--haplotype-b-out-prefix", str(out_dir / "hapB"),
                "--unclassified-out-prefix", str(out_dir / "unclassified")]
    capsys.readouterr()
    with patch("sys.argv", ["classify-by-kmers"] + argv + prefixes):
        main()
    out, err = capsys.readouterr()
    return out, err, {name: gzip.open(out_dir / name, "rb").read() for name in sorted(os.listdir(out_dir))}


def test_cli_databases_give_what_their_lists_give(trio, capsys, tmp_path):
    by_list = _classify([trio["reads"], trio["list_a"], trio["list_b"]], tmp_path / "lists", capsys)
    by_db = _classify([trio["reads"], trio["db_a"], trio["db_b"]], tmp_path / "dbs", capsys)
    assert by_db[0] == by_list[0] and by_db[0].count("\n") >= 63
    assert len(by_db[2]) == 3 and by_db[2] == by_list[2]
    assert sum(len(body) > 0 for body in by_db[2].values()) >= 2
    assert by_db[1].count("Using counts in range [5,35]") == 2 and "Using counts" not in by_list[1]


def test_cli_cutoffs_by_hand_equal_lists_dumped_again_at_them(trio, capsys, tmp_path):
    from trio_binning_amd import find_unique_kmers as fu

    cuts = ["--min-count-a", "8", "--max-count-a", "30", "--min-count-b", "6", "--max-count-b", "27"]
    again = tmp_path / "again"
    again.mkdir()
    fu.main(["-k", str(trio["k"]), "-o", str(again), "-s", str(again)] + cuts + [trio["db_a"], trio["db_b"]])
    lists = [str(again / "hapA_only_kmers.txt"), str(again / "hapB_only_kmers.txt")]
    assert open(lists[0]).read() != open(trio["list_a"]).read() and open(lists[1]).read() != open(trio["list_b"]).read()
    by_list = _classify([trio["reads"]] + lists, tmp_path / "lists", capsys)
    by_db = _classify([trio["reads"], trio["db_a"], trio["db_b"]] + cuts, tmp_path / "dbs", capsys)
    assert by_db[0] == by_list[0] and by_db[2] == by_list[2]
    assert "Using counts in range [8,30]" in by_db[1] and "Using counts in range [6,27]" in by_db[1] and "[5,35]" not in by_db[1]


def test_cli_an_empty_selection_is_a_message_and_no_bin(trio, capsys, tmp_path):
    from trio_binning_amd import kmers
    from trio_binning_amd.classify_by_kmers import main

    assert int(kmers.database_file_info(trio["db_b"])["histogram"][250:].sum()) == 0
    out_dir = tmp_path / "bins"
    out_dir.mkdir()
    argv = [trio["reads"], trio["db_a"], trio["db_b"], "--min-count-b", "250", "--max-count-b", "255",
            "--haplotype-a-out-prefix", str(out_dir / "hapA"), "--haplotype-b-out-prefix", str(out_dir / "hapB"),
            "--unclassified-out-prefix", str(out_dir / "unclassified")]
    with patch("sys.argv", ["classify-by-kmers"] + argv):
        with pytest.raises(SystemExit) as ei:
            main()
    assert isinstance(ei.value.code, str) and "haplotype B" in ei.value.code and "[250,255]" in ei.value.code
    assert os.listdir(out_dir) == [] and capsys.readouterr().out == ""
    # the device is as usable as before
    with kmers.KmerDatabase.load(trio["db_a"]) as da, kmers.KmerDatabase.load(trio["db_b"]) as db, da.unique_set(db, 5, 35) as hs:
        assert hs.num_kmers == open(trio["list_a"]).read().count("\n")
