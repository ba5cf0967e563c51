"""import_database and dump_database on a device: two parents' counted dumps - written by tests/dump_ref.py from the oracle's
counts, as `kmc -ci1 -cs255` and `kmc_dump` would print them - imported with --floor 2 must lead find-unique-kmers to the lists
it writes from databases kept by counting the reads; a kept database dumped and imported again must be the same file; a
refusal shows the file and the line."""
import contextlib
import io
import os

import numpy as np
import pytest

import dump_ref as ref
from test_gpu_kmerdb import _fastq, _library, _oracle_counts, _two_parents

pytestmark = pytest.mark.gpu

K = 21
CUTS = ["--min-count-a", "8", "--max-count-a", "60", "--min-count-b", "9", "--max-count-b", "55"]


def _run(main, argv):
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        main(argv)
    return err.getvalue()


def _lists(out):
    return tuple(open(os.path.join(str(out), name), "rb").read() for name in ("hapA_only_kmers.txt", "hapB_only_kmers.txt"))


@pytest.fixture(scope="module")
def parents(gpu, tmp_path_factory):
    """two parents at about 26x, counted once with --keep-databases; the oracle's counts of the same reads as dumps"""
    from trio_binning_amd import find_unique_kmers as fu

    root = tmp_path_factory.mktemp("dump_cli")
    rng = np.random.default_rng(1601)
    ga, gb = _two_parents(rng, glen=12_000)
    reads = {"a": _library(rng, ga, 2100, 150), "b": _library(rng, gb, 2100, 150)}
    files = {"a": _fastq(root / "a.fastq", reads["a"]), "b": _fastq(root / "b.fastq", reads["b"])}
    counted = root / "counted"
    counted.mkdir()
    _run(fu.main, ["-k", str(K), "-o", str(counted), "-s", str(counted), "--capacity", "1500000", "--keep-databases"] + CUTS + [files["a"], files["b"]])
    dumps = {}
    for name in "ab":
        keys, counts = _oracle_counts(reads[name], K)
        path = root / "{}.dump.txt".format(name)
        path.write_bytes(ref.format(keys, np.minimum(counts, 255), K))
        dumps[name] = str(path)
    return {"root": root, "reads": reads, "dumps": dumps, "fu": fu, "lists": _lists(counted),
            "dbs": {name: str(counted / "haplotype{}.tbkdb".format(name.upper())) for name in "ab"}}


def test_imported_dumps_give_the_lists_of_counted_reads(parents, tmp_path):
    from trio_binning_amd import import_database

    assert all(len(l) > 21 * 50 for l in parents["lists"]), "the cut-offs select something"
    dbs = {}
    for name in "ab":
        dbs[name] = str(tmp_path / "{}.tbkdb".format(name))
        reads = parents["reads"][name]
        err = _run(import_database.main, ["-o", dbs[name], "--floor", "2", "--reads", str(len(reads)), "--bases", str(sum(map(len, reads))), parents["dumps"][name]])
        assert "\033[92mImporting 1 counted dump...\033[0m" in err and "written to " + dbs[name] in err
        # with the reads and bases stated, the file is the one that counting the reads left
        with open(dbs[name], "rb") as got, open(parents["dbs"][name], "rb") as want:
            assert got.read() == want.read()
    out = tmp_path / "imported"
    out.mkdir()
    _run(parents["fu"].main, ["-k", str(K), "-o", str(out), "-s", str(out)] + CUTS + [dbs["a"], dbs["b"]])
    assert _lists(out) == parents["lists"]


def test_two_lanes_on_one_command_line(parents, tmp_path):
    """a parent's dump split into two files (its lanes' k-mers, here every other line) makes the same database"""
    from trio_binning_amd import import_database

    lines = open(parents["dumps"]["a"], "rb").read().split(b"\n")[:-1]
    halves = []
    for i in range(2):
        path = tmp_path / "lane{}.txt".format(i)
        path.write_bytes(b"".join(l + b"\n" for l in lines[i::2]))
        halves.append(str(path))
    reads = parents["reads"]["a"]
    out = str(tmp_path / "lanes.tbkdb")
    _run(import_database.main, ["-o", out, "-k", str(K), "--floor", "2", "--reads", str(len(reads)), "--bases", str(sum(map(len, reads))), ",".join(halves)])
    with open(out, "rb") as got, open(parents["dbs"]["a"], "rb") as want:
        assert got.read() == want.read()


def test_dump_database_round_trip(parents, tmp_path):
    from trio_binning_amd import dump_database, import_database, kmers

    info = kmers.database_file_info(parents["dbs"]["b"])
    text = str(tmp_path / "b.txt")
    err = _run(dump_database.main, [parents["dbs"]["b"], "-o", text])
    assert "Dumping k-mers with counts in range [2,255]" in err and "{} 21-mers written to {}".format(info["n"], text) in err
    keys, counts = _oracle_counts(parents["reads"]["b"], K)
    with open(text, "rb") as fh:
        assert fh.read() == ref.format(keys, np.minimum(counts, 255), K, 2, 255)
    # the solid dump does not say how many k-mers were seen once: the entries come back, rows 0 and 1 are the dump's own
    back = str(tmp_path / "back.tbkdb")
    _run(import_database.main, ["-o", back, "--reads", str(info["reads_added"]), "--bases", str(info["bases_added"]), text])
    again = kmers.database_file_info(back)
    assert (again["floor"], again["n"], again["k"]) == (2, info["n"], K) and np.array_equal(again["histogram"][2:], info["histogram"][2:])
    with open(back, "rb") as got, open(parents["dbs"]["b"], "rb") as want:
        assert got.read()[2096:] == want.read()[2096:]
    # a full database, kept with the k-mers seen once, comes back byte for byte
    with kmers.KmerCounter(K, 1 << 20, keep_singletons=True) as counter:
        counter.add_reads(parents["reads"]["b"][:500])
        with counter.database() as db:
            full = str(tmp_path / "full.tbkdb")
            db.save(full)
            st = db.stats()
    _run(dump_database.main, [full, "-o", text, "--min-count", "1"])
    _run(import_database.main, ["-o", back, "--reads", str(st["reads_added"]), "--bases", str(st["bases_added"]), text])
    with open(back, "rb") as got, open(full, "rb") as want:
        assert got.read() == want.read()
    # a range
    err = _run(dump_database.main, [full, "-o", text, "--min-count", "3", "--max-count", "7"])
    keys, counts = _oracle_counts(parents["reads"]["b"][:500], K)
    with open(text, "rb") as fh:
        assert fh.read() == ref.format(keys, np.minimum(counts, 255), K, 3, 7)


def test_a_refusal_shows_file_and_line(parents, tmp_path):
    from trio_binning_amd import import_database

    lines = open(parents["dumps"]["a"], "rb").read().split(b"\n")
    lines[1234] = lines[1234].replace(b"\t", b"\t-")
    bad = tmp_path / "bad.txt"
    bad.write_bytes(b"\n".join(lines))
    out = str(tmp_path / "bad.tbkdb")
    with pytest.raises(ValueError) as exc:
        _run(import_database.main, ["-o", out, parents["dumps"]["b"] + "," + str(bad)])
    assert "{}: line 1235: ".format(bad) in str(exc.value) and ref.NOT_DIGITS in str(exc.value)
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
