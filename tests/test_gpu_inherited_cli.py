"""The child on both command lines: find-unique-kmers --child (read files, or the database a --keep-databases run left) and
classify-by-kmers --child-database.  The lists must be the oracle's inherited sets - of each parent's k-mers within its
cut-offs that the other parent lacks, those the child's library holds at least twice and at least --min-count-child times
(oracle.unique_oracle.count_kmers_np on the three libraries) - and the classifier built from three databases must write what
the one built from those lists writes."""
import os
import re

import numpy as np
import pytest

import kmerdb_files as kf
from test_gpu_kmerdb import _fastq, _library, _oracle_counts, _oracle_file, _rc, _two_parents
from test_gpu_kmerdb_inherited import _inherited_np, _second_haplotype
from test_gpu_kmerdb_table import _classify

pytestmark = pytest.mark.gpu

K = 21


def _ranges(err):
    """((min, max) of A, (min, max) of B, the child's minimum) as the run's stderr states them"""
    parents = re.findall(r"Using counts in range \[(\d+),(\d+)\]\.", err)
    child = re.findall(r"Using counts in range \[(\d+),255\] for the child\.", err)
    assert len(parents) == 2 and len(child) == 1, err
    return tuple(map(int, parents[0])), tuple(map(int, parents[1])), int(child[0])


def _lists(out):
    return tuple(open(os.path.join(str(out), name), "rb").read() for name in ("hapA_only_kmers.txt", "hapB_only_kmers.txt"))


def _text(ranks):
    from oracle import unique_oracle as uo

    return "".join(s + "\n" for s in uo.kmer_strings(ranks, K)).encode()


@pytest.fixture(scope="module")
def trio(gpu, tmp_path_factory):
    """Both parents at about 26x over two haplotypes each, the child at about 26x over the first haplotype of each parent; one
    run of find-unique-kmers --child --keep-databases on the read files, and long reads of the child's two haplotypes."""
    from trio_binning_amd import find_unique_kmers as fu

    root = tmp_path_factory.mktemp("inherited")
    rng = np.random.default_rng(311)
    ga, gb = _two_parents(rng, glen=20_000)
    ga2, gb2 = _second_haplotype(rng, ga), _second_haplotype(rng, gb)
    reads = {"a": _library(rng, ga, 1750, 150) + _library(rng, ga2, 1750, 150),
             "b": _library(rng, gb, 1750, 150) + _library(rng, gb2, 1750, 150),
             "child": _library(rng, ga, 1750, 150, err=0.005) + _library(rng, gb, 1750, 150, err=0.005)}
    files = {"a": _fastq(root / "a.fastq", reads["a"]), "b": _fastq(root / "b.fastq.gz", reads["b"], gz=True),
             "child": _fastq(root / "c1.fastq", reads["child"][:2000]) + "," + _fastq(root / "c2.fastq.gz", reads["child"][2000:], gz=True)}
    out = root / "counted"
    out.mkdir()
    return {"root": root, "reads": reads, "files": files, "out": out, "fu": fu,
            "counts": {name: _oracle_counts(r, K) for name, r in reads.items()},
            "common": lambda where: ["-k", str(K), "-o", str(where), "-s", str(where), "--capacity", "1500000"],
            "long_reads": _long_reads(root, rng, ga, gb)}


def _long_reads(root, rng, ga, gb):
    long_reads = []
    for i in range(60):
        g = (ga, gb)[i % 2]
        length = int(rng.integers(100, 3000))
        p = int(rng.integers(0, len(g) - length))
        s = g[p:p + length]
        long_reads.append(_rc(s) if i % 3 == 0 else s)
    return _fastq(root / "long.fastq", long_reads + [ga[:500] + gb[500:1000], "ACGT" * 10, "N" * 50])


@pytest.fixture(scope="module")
def counted(trio):
    """the --child run on read files, keeping the databases: (its two lists, its cut-offs)"""
    import contextlib
    import io

    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        trio["fu"].main(trio["common"](trio["out"]) + ["--keep-databases", "--child", trio["files"]["child"], trio["files"]["a"], trio["files"]["b"]])
    return {"lists": _lists(trio["out"]), "ranges": _ranges(err.getvalue()), "err": err.getvalue(),
            "dbs": [str(trio["out"] / name) for name in ("haplotypeA.tbkdb", "haplotypeB.tbkdb", "child.tbkdb")]}


def test_child_reads_and_the_kept_child_database_write_the_oracles_lists(trio, counted, tmp_path, capsys):
    from oracle import unique_oracle as uo
    from trio_binning_amd import find_unique_kmers as fu

    (lo_a, hi_a), (lo_b, hi_b), child_min = counted["ranges"]
    na, nb, nc = (trio["counts"][name] for name in ("a", "b", "child"))
    # the child's cut-off is the minimum the reference's rule finds on its rows; its histogram file holds those 255 rows
    hist = kf.database_of(*nc)[2]
    rows = [(c, 0 if c == 1 else int(hist[c])) for c in range(1, 256)]
    assert child_min == fu.analyze_histogram(rows)[0] >= 2
    assert open(trio["out"] / "child.histogram").read() == "".join("{}\t{}\n".format(c, n) for c, n in rows)
    assert open(counted["dbs"][2], "rb").read() == _oracle_file(trio["reads"]["child"], K, nc)
    want_a = _inherited_np(na, nb, nc, lo_a, hi_a, child_min, 255)
    want_b = _inherited_np(nb, na, nc, lo_b, hi_b, child_min, 255)
    assert counted["lists"] == (_text(want_a), _text(want_b))
    # what the child lacks is gone from both lists, and much is left
    for want, both in ((want_a, uo.unique_np(na, nb, lo_a, hi_a)), (want_b, uo.unique_np(nb, na, lo_b, hi_b))):
        assert 1000 < want.size < both.size - 500
    assert "# of unique k-mers the child inherited in haplotype A: {}".format(want_a.size) in counted["err"]
    assert "# of unique k-mers the child inherited in haplotype B: {}".format(want_b.size) in counted["err"]
    # the same from the three kept databases, nothing counted; and from the parents' read files beside the child's database in passes
    for name, argv in (("dbs", ["--child", counted["dbs"][2]] + counted["dbs"][:2]),
                       ("mixed", ["--passes", "3", "--child", counted["dbs"][2], trio["files"]["a"], counted["dbs"][1]])):
        out = tmp_path / name
        out.mkdir()
        capsys.readouterr()
        fu.main(trio["common"](out) + argv)
        err = capsys.readouterr().err
        assert _ranges(err) == counted["ranges"] and "Loading the k-mer database of the child" in err
        assert _lists(out) == counted["lists"]
        assert open(out / "child.histogram").read() == open(trio["out"] / "child.histogram").read()
        assert not os.path.exists(out / "child.tbkdb")


def test_min_count_child_by_hand_is_honoured(trio, counted, tmp_path, capsys):
    from trio_binning_amd import find_unique_kmers as fu

    (lo_a, hi_a), (lo_b, hi_b), child_min = counted["ranges"]
    by_hand = child_min + 9
    na, nb, nc = (trio["counts"][name] for name in ("a", "b", "child"))
    capsys.readouterr()
    fu.main(trio["common"](tmp_path) + ["--min-count-child", str(by_hand), "--child", counted["dbs"][2]] + counted["dbs"][:2])
    assert _ranges(capsys.readouterr().err) == ((lo_a, hi_a), (lo_b, hi_b), by_hand)
    want_a = _inherited_np(na, nb, nc, lo_a, hi_a, by_hand, 255)
    want_b = _inherited_np(nb, na, nc, lo_b, hi_b, by_hand, 255)
    assert _lists(tmp_path) == (_text(want_a), _text(want_b))
    assert 0 < len(_text(want_a)) < len(counted["lists"][0]) and 0 < len(_text(want_b)) < len(counted["lists"][1])


def test_classify_from_three_databases_equals_classify_from_the_inherited_lists(trio, counted, tmp_path, capsys):
    lists = [str(trio["out"] / "hapA_only_kmers.txt"), str(trio["out"] / "hapB_only_kmers.txt")]
    by_list = _classify([trio["long_reads"]] + lists, tmp_path / "lists", capsys)
    by_db = _classify([trio["long_reads"]] + counted["dbs"][:2] + ["--child-database", counted["dbs"][2]], tmp_path / "dbs", capsys)
    assert by_db[0] == by_list[0] and by_db[0].count("\n") >= 63
    assert len(by_db[2]) == 3 and by_db[2] == by_list[2] and sum(len(body) > 0 for body in by_db[2].values()) >= 2
    assert _ranges(by_db[1]) == counted["ranges"]
    sizes = [text.count(b"\n") for text in counted["lists"]]
    for hap, n in zip("AB", sizes):
        assert "Found {} {}-mers unique to haplotype {} and inherited by the child".format(n, K, hap) in by_db[1]
    # by hand as well
    by_hand = _classify([trio["long_reads"]] + counted["dbs"][:2] + ["--child-database", counted["dbs"][2], "--min-count-child", str(counted["ranges"][2])],
                        tmp_path / "hand", capsys)
    assert by_hand[0] == by_db[0] and by_hand[2] == by_db[2]
    # without the child the lists are larger, by different shares: the scores' scaling factor moves, and the score columns with it
    without = _classify([trio["long_reads"]] + counted["dbs"][:2], tmp_path / "without", capsys)
    found = [int(n) for n in re.findall(r"Found (\d+) 21-mers unique to haplotype [AB] \(", without[1])]
    assert len(found) == 2 and found[0] > sizes[0] and found[1] > sizes[1]
    assert found[0] * sizes[1] != found[1] * sizes[0]  # (each count is scaled by max(nA, nB) / n of its own list)
    rows_with, rows_without = ([line.split("\t") for line in text.splitlines()] for text in (by_db[0], without[0]))
    assert len(rows_with) == len(rows_without) and [r[0] for r in rows_with] == [r[0] for r in rows_without]
    assert [r[1:] for r in rows_with] != [r[1:] for r in rows_without]


def test_a_child_without_a_minimum_is_held_until_its_database_is_kept(trio, counted, tmp_path, capsys):
    """The child at about 3x: its histogram falls from row 2 on and the reference's rule finds no minimum.  With --keep-databases
    the error comes once child.tbkdb is on disk, and stderr names it and --min-count-child; without, it ends the run at once."""
    from trio_binning_amd import find_unique_kmers as fu

    rng = np.random.default_rng(312)
    ga_reads, gb_reads = trio["reads"]["child"][:1750], trio["reads"]["child"][1750:]
    thin = [ga_reads[int(i)] for i in rng.choice(1750, 200, replace=False)] + [gb_reads[int(i)] for i in rng.choice(1750, 200, replace=False)]
    nc = _oracle_counts(thin, K)
    hist = kf.database_of(*nc)[2]
    with pytest.raises(fu.HistogramError):
        fu.analyze_histogram([(c, 0 if c == 1 else int(hist[c])) for c in range(1, 256)])
    reads = _fastq(tmp_path / "thin.fastq", thin)
    out = tmp_path / "out"
    out.mkdir()
    (lo_a, hi_a), (lo_b, hi_b), _ = counted["ranges"]
    capsys.readouterr()
    with pytest.raises(fu.HistogramError) as ei:
        fu.main(trio["common"](out) + ["--child", reads] + counted["dbs"][:2])
    assert str(ei.value) == fu.HistogramError(str(out / "child.histogram")).message
    assert not os.path.exists(out / "child.tbkdb") and not os.path.exists(out / "hapA_only_kmers.txt")
    capsys.readouterr()
    with pytest.raises(fu.HistogramError) as ei:
        fu.main(trio["common"](out) + ["--keep-databases", "--child", reads] + counted["dbs"][:2])
    assert str(ei.value) == fu.HistogramError(str(out / "child.histogram")).message
    err = capsys.readouterr().err
    kept = str(out / "child.tbkdb")
    assert open(kept, "rb").read() == _oracle_file(thin, K, nc) and not os.path.exists(out / "hapA_only_kmers.txt")
    advice = "--min-count-a {} --max-count-a {} --min-count-b {} --max-count-b {} --child {} --min-count-child MIN {} {}".format(
        lo_a, hi_a, lo_b, hi_b, kept, counted["dbs"][0], counted["dbs"][1])
    assert advice in err and "kept in {}, {} and {}".format(counted["dbs"][0], counted["dbs"][1], kept) in err
    # and the advice works
    fu.main(trio["common"](out) + advice.replace("MIN", "2").split())
    na, nb = trio["counts"]["a"], trio["counts"]["b"]
    want = (_inherited_np(na, nb, nc, lo_a, hi_a, 2, 255), _inherited_np(nb, na, nc, lo_b, hi_b, 2, 255))
    assert _lists(out) == (_text(want[0]), _text(want[1])) and want[0].size > 100 and want[1].size > 100
