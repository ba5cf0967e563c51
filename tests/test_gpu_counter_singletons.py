"""Counters that keep the k-mers seen once (KmerCounter(keep_singletons=True)) and what their full databases allow: the union of
the databases of two halves of a library is, byte for byte, the database of the whole library, and its solid form is the file
the same counter leaves without the option.  The yardstick is oracle/unique_oracle.py (count_kmers_np, add_counts_np,
histogram_np) on the reads themselves - in compressed space on tests/hpc_ref.compress_np of them - and the files are written
with numpy alone (tests/kmerdb_files.py).  Then the command lines: find-unique-kmers --keep-singletons and a parent given as a
database plus more reads, merge_databases, classify-by-kmers and assembly-qv on full databases."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

import db_query_ref as ref
import hpc_ref
import kmerdb_files as kf
from test_gpu_kmerdb import _add_in_batches, _fastq, _library, _oracle_counts, _random_dna, _rc
from test_gpu_kmerdb_table import _classify

pytestmark = pytest.mark.gpu

FULL = {False: b"TBKKMFB1", True: b"TBKKMFH1"}
SOLID = {False: b"TBKKMDB1", True: b"TBKKMDH1"}


@functools.lru_cache(maxsize=None)
def _halves():
    """R1 and R2: reads of about 100 bases with substitution errors over a genome of 4000, and blocks of one read many times"""
    rng = np.random.default_rng(2024)
    genome = _random_dna(rng, 4000)
    often, very_often, once = _random_dna(rng, 100), _random_dna(rng, 90), _random_dna(rng, 80)
    r1 = _library(rng, genome, 500, 100, err=0.02, lower=0.1) + [often] * 130 + [very_often] * 300 + ["", "N" * 30, genome[:20], once]
    r2 = _library(rng, genome, 450, 104, err=0.02) + [_rc(often)] * 130 + [genome[:21], _rc(once)]
    return r1, r2, genome


@functools.lru_cache(maxsize=None)
def _oracle(k, compress):
    """(counts of R1, of R2, of both; bases the counter is to report for R1, R2) in the space the counter works in"""
    from oracle import unique_oracle as uo

    r1, r2, _ = _halves()
    packed = [uo.pack(r) for r in (r1, r2)]
    if compress:
        packed = [hpc_ref.compress_np(b, o, True) for b, o in packed]
    n1, n2 = (uo.count_kmers_np(b, o, k) for b, o in packed)
    return n1, n2, uo.add_counts_np(n1, n2), tuple(int(o[-1]) for _, o in packed)


def _full_file(counts, k, reads, bases, compress):
    from oracle import unique_oracle as uo

    keys, cnt = counts
    hist = uo.histogram_np(cnt).astype(np.uint64)
    return kf.file_bytes(k, keys, np.minimum(cnt, 255).astype(np.uint8), hist, reads=reads, bases=bases, magic=FULL[compress])


def _solid_file(counts, k, reads, bases, compress):
    keys, cnt, hist = kf.database_of(*counts)
    return kf.file_bytes(k, keys, cnt, hist, reads=reads, bases=bases, magic=SOLID[compress])


def _count(reads, k, passes, compress, keep):
    from trio_binning_amd import kmers

    c = kmers.KmerCounter(k, 300_000, passes=passes, compress=compress, keep_singletons=keep)
    _add_in_batches(c, reads, (170, 333))
    return c


def _saved(db, path):
    db.save(str(path))
    return open(path, "rb").read()


@pytest.mark.parametrize("compress", [False, True], ids=["plain", "compress"])
@pytest.mark.parametrize("k", [21, 31])
def test_the_union_of_two_halves_is_the_count_of_both(gpu, tmp_path, k, compress):
    from oracle import unique_oracle as uo

    r1, r2, _ = _halves()
    n1, n2, n12, (bases1, bases2) = _oracle(k, compress)
    # the input holds what the old databases could not see: without these the test could pass with their blind spot intact
    for keys, cnt in (n1, n2):
        assert int((cnt == 1).sum()) >= 100
    in_both = np.intersect1d(n1[0], n2[0])
    c1, c2 = n1[1][np.searchsorted(n1[0], in_both)], n2[1][np.searchsorted(n2[0], in_both)]
    assert ((c1 < 255) & (c2 < 255) & (c1 + c2 > 255)).any()  # below 255 in both halves, their sum past it
    assert (n1[1] >= 255).any()                                # at 255 already in one half
    assert ((c1 == 1) & (c2 == 1)).any()                       # seen once in each half: in neither of the old databases
    want = {"r1": _full_file(n1, k, len(r1), bases1, compress), "r2": _full_file(n2, k, len(r2), bases2, compress),
            "both": _full_file(n12, k, len(r1) + len(r2), bases1 + bases2, compress),
            "solid": _solid_file(n12, k, len(r1) + len(r2), bases1 + bases2, compress)}
    files = {}
    for passes in (1, 3):
        with _count(r1, k, passes, compress, True) as ca, _count(r2, k, passes, compress, True) as cb, \
                _count(r1 + r2, k, passes, compress, True) as cab, _count(r1 + r2, k, passes, compress, False) as plain:
            # histogram and subtraction answer as they do without the option
            assert np.array_equal(ca.histogram(), uo.histogram_np(n1[1]).astype(np.uint64)), passes
            assert np.array_equal(cab.histogram(), plain.histogram())
            n = ca.unique(cb, 2, 255, str(tmp_path / "dump.txt"))
            only = uo.unique_np(n1, n2, 2, 255)
            assert n == only.size > 0 and open(tmp_path / "dump.txt").read() == "".join(s + "\n" for s in uo.kmer_strings(only, k)), passes
            with ca.database() as d1, cb.database() as d2, cab.database() as d12, plain.database() as dp:
                assert (d1.floor, d2.floor, d12.floor, dp.floor) == (1, 1, 1, 2) and d12.compressed is compress
                keys, counts = d12.entries()
                assert np.array_equal(keys, n12[0]) and np.array_equal(counts, np.minimum(n12[1], 255).astype(np.uint8))  # the oracle's counts capped at 255
                assert len(d12) == n12[0].size == int(d12.histogram()[0]) == cab.stats()["distinct"] and cab.stats()["database_bytes"] in (0, 9 * n12[0].size)
                assert _saved(d1, tmp_path / "r1.tbkdb") == want["r1"] and _saved(d2, tmp_path / "r2.tbkdb") == want["r2"], passes
                whole = _saved(d12, tmp_path / "both.tbkdb")
                assert whole == want["both"], passes
                with d1.union(d2) as united:
                    assert _saved(united, tmp_path / "united.tbkdb") == whole, passes           # union(db(R1), db(R2)) is db(R1 + R2)
                with d2.union(d1) as united:
                    assert _saved(united, tmp_path / "united.tbkdb") == whole, passes
                without = _saved(dp, tmp_path / "plain.tbkdb")
                assert without == want["solid"], passes
                with d12.solid() as solid:
                    assert _saved(solid, tmp_path / "solid.tbkdb") == without, passes           # and its solid form the file without the option
                with d1.union(d2) as united, united.solid() as solid:
                    assert _saved(solid, tmp_path / "solid.tbkdb") == without, passes
                files[passes] = whole
            if passes == 3:
                assert cab.stats()["database_bytes"] == 9 * n12[0].size  # 9 bytes for every distinct k-mer
    assert files[1] == files[3]  # the database is the same whatever `passes` was


# ---- the command lines ----------------------------------------------------------------------------------------------------------
K = 21
CUTS = ["--min-count-a", "3", "--max-count-a", "60", "--min-count-b", "3", "--max-count-b", "60"]


def _find(out, argv):
    from trio_binning_amd import find_unique_kmers as fu

    out.mkdir(exist_ok=True)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        fu.main(["-k", str(K), "-o", str(out), "-s", str(out), "--capacity", "400000"] + CUTS + argv)
    return {name: open(os.path.join(str(out), name), "rb").read()
            for name in ("hapA_only_kmers.txt", "hapB_only_kmers.txt", "haplotypeA.histogram", "haplotypeB.histogram")}


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    """Parent A in two lanes (two files each), parent B in one; a run that keeps solid databases and one that keeps full ones"""
    root = tmp_path_factory.mktemp("singletons")
    rng = np.random.default_rng(99)
    base = _random_dna(rng, 5000)
    ga = base
    gb = "".join("ACGT"[("ACGT".index(c) + 1) % 4] if rng.random() < 0.01 else c for c in base)
    once = _random_dna(rng, 150)  # a read of its own, in lane 2 alone: k-mers the reads hold once
    lanes = {"a1": _library(rng, ga, 500, 120, err=0.01), "a2": _library(rng, ga, 450, 120, err=0.01) + [once], "b": _library(rng, gb, 900, 120, err=0.01)}
    files = {"a1": _fastq(root / "a1x.fastq", lanes["a1"][:200]) + "," + _fastq(root / "a1y.fastq.gz", lanes["a1"][200:], gz=True),
             "a2": _fastq(root / "a2x.fastq.gz", lanes["a2"][:300], gz=True) + "," + _fastq(root / "a2y.fastq", lanes["a2"][300:]),
             "b": _fastq(root / "b.fastq", lanes["b"])}
    counts_a = _oracle_counts(lanes["a1"] + lanes["a2"], K)
    w = {"root": root, "lanes": lanes, "files": files, "ga": ga, "gb": gb, "once": once, "counts_a": counts_a}
    w["solid"] = _find(root / "solid", ["--keep-databases", files["a1"] + "," + files["a2"], files["b"]])
    w["full"] = _find(root / "full", ["--keep-databases", "--keep-singletons", files["a1"] + "," + files["a2"], files["b"]])
    return w


def _db(world, run, hap):
    return str(world["root"] / run / "haplotype{}.tbkdb".format(hap))


def test_keep_singletons_changes_the_databases_and_nothing_else(world):
    from trio_binning_amd import kmers

    assert world["full"] == world["solid"]  # lists and histogram files, byte for byte
    assert world["solid"]["hapA_only_kmers.txt"].count(b"\n") > 20 and world["solid"]["hapB_only_kmers.txt"].count(b"\n") > 20
    reads = world["lanes"]["a1"] + world["lanes"]["a2"]
    bases = sum(map(len, reads))
    assert open(_db(world, "full", "A"), "rb").read() == _full_file(world["counts_a"], K, len(reads), bases, False)
    assert open(_db(world, "solid", "A"), "rb").read() == _solid_file(world["counts_a"], K, len(reads), bases, False)
    assert [kmers.database_file_info(_db(world, run, "B"))["floor"] for run in ("solid", "full")] == [2, 1]
    assert int((world["counts_a"][1] == 1).sum()) > 100


def test_a_kept_full_database_and_a_new_lane_are_one_count_of_both(world, tmp_path):
    """lane 1 alone, kept full; then `haplotypeA.tbkdb,<lane 2's files>` as the parent: the lists of one run over both lanes,
    and the united database that run keeps is the one a count of both lanes leaves"""
    first = tmp_path / "lane1"
    _find(first, ["--keep-databases", "--keep-singletons", world["files"]["a1"], world["files"]["b"]])
    kept = str(first / "haplotypeA.tbkdb")
    for tag, parent_a, parent_b in (("db_first", kept + "," + world["files"]["a2"], _db(world, "full", "B")),
                                    ("reads_first", world["files"]["a2"] + "," + kept, world["files"]["b"])):
        again = _find(tmp_path / tag, ["--keep-databases", parent_a, parent_b])
        assert again == world["solid"], tag
        assert open(tmp_path / tag / "haplotypeA.tbkdb", "rb").read() == open(_db(world, "full", "A"), "rb").read(), tag
    # passes change nothing, and without --keep-databases nothing is kept
    again = _find(tmp_path / "passes", ["--passes", "3", kept + "," + world["files"]["a2"], _db(world, "solid", "B")])
    assert again == world["solid"] and not (tmp_path / "passes" / "haplotypeA.tbkdb").exists()


def test_a_mixed_list_with_a_solid_database_ends_before_anything_is_counted(world, tmp_path, capsys):
    from unittest.mock import patch

    from trio_binning_amd import find_unique_kmers as fu

    with patch.object(fu, "count_library", side_effect=AssertionError("counted")):
        with pytest.raises(SystemExit) as ei:
            fu.main(["-k", str(K), "-o", str(tmp_path), _db(world, "solid", "A") + "," + world["files"]["a2"], world["files"]["b"]])
    err = capsys.readouterr().err
    assert ei.value.code == 2 and _db(world, "solid", "A") in err and "without the k-mers seen once" in err


def test_merge_databases(world, tmp_path, capsys):
    from trio_binning_amd import merge_databases as md

    # --solid on one input is a plain conversion: the file the run without --keep-singletons kept
    md.main(["--solid", "-o", str(tmp_path / "solid.tbkdb"), _db(world, "full", "A")])
    assert open(tmp_path / "solid.tbkdb", "rb").read() == open(_db(world, "solid", "A"), "rb").read()
    # two lanes counted apart, united: the full database of both; with --solid the plain one
    lanes = []
    for lane in ("a1", "a2"):
        _find(tmp_path / lane, ["--keep-databases", "--keep-singletons", world["files"][lane], world["files"]["b"]])
        lanes.append(str(tmp_path / lane / "haplotypeA.tbkdb"))
    md.main(["-o", str(tmp_path / "united.tbkdb")] + lanes)
    assert open(tmp_path / "united.tbkdb", "rb").read() == open(_db(world, "full", "A"), "rb").read()
    md.main(["-o", str(tmp_path / "united_solid.tbkdb"), "--solid"] + lanes[::-1])
    assert open(tmp_path / "united_solid.tbkdb", "rb").read() == open(_db(world, "solid", "A"), "rb").read()
    assert "k-mers of {} reads written".format(len(world["lanes"]["a1"]) + len(world["lanes"]["a2"])) in capsys.readouterr().err


def test_classify_by_kmers_takes_full_databases_as_their_solid_form(world, tmp_path, capsys):
    rng = np.random.default_rng(5)
    long_reads = []
    for i in range(40):
        g = (world["ga"], world["gb"])[i % 2]
        p = int(rng.integers(0, len(g) - 1500))
        long_reads.append(g[p:p + int(rng.integers(200, 1500))])
    reads = _fastq(tmp_path / "long.fastq", long_reads)
    by_solid = _classify(CUTS + [reads, _db(world, "solid", "A"), _db(world, "solid", "B")], tmp_path / "by_solid", capsys)
    by_full = _classify(CUTS + [reads, _db(world, "full", "A"), _db(world, "full", "B")], tmp_path / "by_full", capsys)
    assert by_full[0] == by_solid[0] and by_full[0].count("\n") >= 40 and by_full[2] == by_solid[2]
    mixed = _classify(CUTS + [reads, _db(world, "full", "A"), _db(world, "solid", "B")], tmp_path / "mixed", capsys)
    assert mixed[0] == by_solid[0] and mixed[2] == by_solid[2]


def test_assembly_qv_counts_presence_on_a_full_database(world, tmp_path, capsys):
    from trio_binning_amd import assembly_qv

    keys, counts = world["counts_a"]
    by_rank = dict(zip(keys.tolist(), counts.tolist()))
    contigs = [("ga", world["ga"]), ("piece", ref.revcomp(world["ga"][100:900]) + "N" + world["gb"][:700].lower()), ("once", ref.revcomp(world["once"]))]
    fa = tmp_path / "asm.fa"
    fa.write_text("".join(">{}\n{}\n".format(name, s) for name, s in contigs))
    want = {1: [0, 0], 2: [0, 0]}  # clean, found: a Python count of presence and of counter >= 2
    for _, s in contigs:
        for km in ref.window_kmers(s, K):
            if km is not None:
                c = by_rank.get(ref.lex_rank(km), 0)
                for lo in (1, 2):
                    want[lo][0] += 1
                    want[lo][1] += c >= lo
    assert want[1][1] > want[2][1] + 20 and want[1][1] < want[1][0]
    totals = {}
    for lo in (1, 2):
        capsys.readouterr()
        assembly_qv.main([str(fa), _db(world, "full", "A"), "--min-count", str(lo)])
        row = capsys.readouterr().out.splitlines()[-1].split("\t")
        assert row[0] == "#total"
        totals[lo] = (int(row[2]), int(row[3]), int(row[6]))
        assert [int(row[2]), int(row[3])] == want[lo], lo
    absent = {lo: totals[lo][0] - totals[lo][1] for lo in (1, 2)}
    assert absent[1] < absent[2]                                                   # fewer absent windows when presence counts
    assert totals[1][2] == keys.size and totals[2][2] == int((counts >= 2).sum())  # solid: every distinct k-mer, or those seen twice
    # on the solid database --min-count 2 says what it says on the full one, and 1 stays refused
    capsys.readouterr()
    assembly_qv.main([str(fa), _db(world, "solid", "A"), "--min-count", "2"])
    row = capsys.readouterr().out.splitlines()[-1].split("\t")
    assert (int(row[2]), int(row[3]), int(row[6])) == totals[2]
    with pytest.raises(SystemExit):
        assembly_qv.main([str(fa), _db(world, "solid", "A"), "--min-count", "1"])
    assert "--keep-singletons" in capsys.readouterr().err
