"""The hetmers command without a GPU: every refusal of its command line comes from the arguments and from crafted headers
(tests/kmerdb_files.py) alone, before a database is loaded - ``kmers.KmerDatabase.load`` and the library's device entry points
are patched to fail the test if they are reached; the default cut-offs come from the header's histogram; and the matrix and
pairs files come back through their readers as they were written."""
import contextlib
import os
from unittest.mock import patch

import numpy as np
import pytest

import db_hetmer_ref as ref
import kmerdb_files as kf
from test_host_kmerdb_full import FULL_HPC, full_file

DEVICE_ENTRIES = ("tbk_kmerdb_load", "tbk_kmerdb_solid", "tbk_kmerdb_hetmers")


@contextlib.contextmanager
def no_device():
    from trio_binning_amd import _lib, kmers

    def reached(*args, **kw):
        raise AssertionError("the device was touched: KmerDatabase.load")

    with contextlib.ExitStack() as stack:
        stack.enter_context(patch.object(kmers.KmerDatabase, "load", reached))
        for name in DEVICE_ENTRIES:
            stack.enter_context(patch.object(_lib.lib, name, side_effect=AssertionError("the device was touched: " + name)))
        yield


def spectrum_file(k=21, magic=kf.MAGIC):
    """A solid file whose histogram falls to 60 k-mers at counter 5, rises to a peak at 25 and first drops below 60 at counter 49:
    the cut-offs find-unique-kmers chooses from it are (5, 49)."""
    hist = np.zeros(256, dtype=np.uint64)
    hist[2:7] = (900, 400, 150, 60, 80)
    for c in range(7, 50):
        hist[c] = 1000 - 40 * abs(c - 25)
    assert hist[48] == 80 and hist[49] == 40
    counts = np.repeat(np.arange(256), hist.astype(np.int64)).astype(np.uint8)
    keys = np.arange(counts.size, dtype=np.uint64) * np.uint64(3)
    hist[1] = 5000
    hist[0] = counts.size + 5000
    return kf.file_bytes(k, keys, counts, hist, reads=10, bases=1000, magic=magic)


@pytest.fixture()
def dbs(tmp_path):
    files = {
        "child": spectrum_file(),
        "a": spectrum_file(),
        "b": kf.sound(k=21, n=40, seed=3)[0],  # (a histogram no cut-offs are found in)
        "full": full_file(k=21, seed=2)[0],
        "even": kf.sound(k=16, n=30, seed=4)[0],
        "k31": kf.sound(k=31, n=30, seed=5)[0],
        "hpc": full_file(k=21, seed=2, magic=FULL_HPC)[0],
        "damaged": kf.sound(k=21, n=40, seed=3)[0][:-3],
    }
    out = {"dir": str(tmp_path)}
    for name, data in files.items():
        out[name] = str(tmp_path / (name + ".tbkdb"))
        open(out[name], "wb").write(data)
    out["list"] = str(tmp_path / "hapA.txt")
    open(out["list"], "w").write("ACGTACGTACGTACGTACGTA\n")
    return out


def test_default_cutoffs_come_from_the_headers_histogram(built, dbs, capsys):
    from trio_binning_amd import hetmers as hm

    with no_device():
        args = hm.parse_args([dbs["child"]])
        assert args.range == (5, 49) and args.parents is None and args.info["k"] == 21
        args = hm.parse_args([dbs["child"], "--min-count", "7", "--max-count", "255"])
        assert args.range == (7, 255)
        args = hm.parse_args([dbs["b"], "--min-count", "1", "--max-count", "1"])  # by hand: the histogram is not asked
        assert args.range == (1, 1)
        args = hm.parse_args([dbs["child"], "--parent-a", dbs["a"], "--parent-b", dbs["b"], "--min-count-b", "3", "--max-count-b", "900"])
        assert args.range == (5, 49) and args.parents.ranges == {"A": (5, 49), "B": (3, 255)} and args.parents.paths == {"A": dbs["a"], "B": dbs["b"]}
        with pytest.raises(AssertionError, match="the device was touched: KmerDatabase.load"):
            hm.main([dbs["child"], "--matrix", dbs["dir"] + "/m.tsv"])
    assert not os.path.exists(dbs["dir"] + "/m.tsv") and capsys.readouterr().out == ""


def test_hetmers_refuses_from_the_command_line_and_the_headers(built, dbs, capsys):
    from trio_binning_amd import hetmers as hm

    child = dbs["child"]
    cases = (
        ([dbs["list"]], 2, ["hapA.txt", "not a count database"]),
        ([child, "--parent-a", dbs["list"], "--parent-b", dbs["a"]], 2, ["hapA.txt", "not a count database"]),
        ([child, "--parent-a", dbs["a"]], 2, ["--parent-a and --parent-b go together"]),
        ([child, "--parent-b", dbs["a"]], 2, ["--parent-a and --parent-b go together"]),
        ([child, "--min-count", "3"], 2, ["--min-count and --max-count go together"]),
        ([child, "--max-count", "30"], 2, ["--min-count and --max-count go together"]),
        ([child, "--min-count", "0", "--max-count", "30"], 2, ["1 <= min <= max <= 255"]),
        ([child, "--min-count", "3", "--max-count", "256"], 2, ["1 <= min <= max <= 255"]),
        ([child, "--min-count", "31", "--max-count", "30"], 2, ["1 <= min <= max <= 255"]),
        ([child, "--min-count-a", "3", "--max-count-a", "30"], 2, ["--min-count-a", "--parent-a and --parent-b"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["a"], "--min-count-b", "3"], 2, ["--min-count-b and --max-count-b go together"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["a"], "--min-count-a", "9", "--max-count-a", "3"], 2, ["1 <= min <= max"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["a"], "--min-count-b", "256", "--max-count-b", "300"], 2, ["a counter is at most 255"]),
        ([child, "--matrix", child], 2, ["names an input"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["b"], "--pairs", dbs["dir"] + "/./b.tbkdb"], 2, ["names an input"]),
        ([child, "--matrix", dbs["dir"] + "/t.tsv", "--pairs", dbs["dir"] + "/t.tsv"], 2, ["--matrix and --pairs name one file"]),
        # the headers
        ([dbs["dir"] + "/missing.tbkdb"], 1, ["missing.tbkdb", "does not exist"]),
        ([dbs["damaged"]], 1, ["damaged.tbkdb"]),
        ([dbs["even"]], 1, ["16-mers", "middle base", "its own mirror under reverse complement", "odd k"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["k31"]], 1, ["21-mers", "31-mers"]),
        ([child, "--parent-a", dbs["hpc"], "--parent-b", dbs["a"]], 1, ["homopolymer-compressed", "plain"]),
        ([dbs["hpc"], "--parent-a", dbs["a"], "--parent-b", dbs["a"], "--min-count", "2", "--max-count", "9"], 1, ["homopolymer-compressed", "plain"]),
        ([dbs["b"]], 1, ["could not find min and max counts", "b.tbkdb", "--min-count and --max-count"]),
        ([child, "--parent-a", dbs["a"], "--parent-b", dbs["b"]], 1, ["could not find min and max counts", "b.tbkdb", "--min-count-b"]),
    )
    with no_device():
        for argv, code, words in cases:
            with pytest.raises(SystemExit) as ei:
                hm.main(argv)
            err = capsys.readouterr().err
            text = err if code == 2 else str(ei.value.code)
            assert (ei.value.code == 2) == (code == 2) and all(w in text for w in words), (argv, ei.value.code, err)
    assert capsys.readouterr().out == ""
    assert not [name for name in os.listdir(dbs["dir"]) if name.endswith(".tsv") or name.endswith(".tmp")]


def test_matrix_and_pairs_files_come_back_as_written(built, tmp_path):
    from trio_binning_amd import hetmers as hm, kmers

    rng = np.random.default_rng(6)
    spec = np.zeros((256, 256), dtype=np.uint64)
    for _ in range(300):
        i = int(rng.integers(1, 256))
        spec[i, int(rng.integers(i, 256))] += np.uint64(int(rng.integers(1, 1 << 40)))
    spec[255, 255] = np.uint64((1 << 63) + 5)
    path = str(tmp_path / "het.tsv")
    hm.write_matrix(path, spec, 21, (3, 80), "child.tbkdb")
    assert np.array_equal(hm.read_matrix(path), spec) and not os.path.exists(path + ".tmp")
    lines = open(path).read().splitlines()
    assert lines[0].startswith("#") and all(w in lines[0] for w in ("k = 21", "3,80", "child.tbkdb")) and len(lines) == 1 + np.count_nonzero(spec)
    assert all(len(line.split("\t")) == 3 for line in lines[1:])
    hm.write_matrix(path, np.zeros((256, 256), dtype=np.uint64), 21, (3, 80), "child.tbkdb")  # replaced whole; an empty matrix is its comment
    assert not hm.read_matrix(path).any() and len(open(path).read().splitlines()) == 1
    open(path, "a").write("3\t2\n")
    with pytest.raises(ValueError, match="line 2"):
        hm.read_matrix(path)

    for k in (1, 21, 31):
        records = np.zeros(50, dtype=kmers.HETMER_PAIR_DTYPE)
        records["minor"] = rng.integers(0, 1 << (2 * k), 50, dtype=np.uint64)
        records["major"] = rng.integers(0, 1 << (2 * k), 50, dtype=np.uint64)
        records["c_minor"], records["c_major"] = rng.integers(1, 256, 50), rng.integers(1, 256, 50)
        records["cls_minor"], records["cls_major"] = rng.integers(0, 4, 50), rng.integers(0, 4, 50)
        want = [(ref.kmer_of(r["minor"], k), int(r["c_minor"]), ref.kmer_of(r["major"], k), int(r["c_major"])) for r in records]
        assert hm.kmers_of_ranks(records["minor"], k) == [w[0] for w in want]
        path = str(tmp_path / "pairs{}.tsv".format(k))
        hm.write_pairs(path, records, k, False)
        assert hm.read_pairs(path) == want and not os.path.exists(path + ".tmp")
        hm.write_pairs(path, records, k, True)
        assert hm.read_pairs(path) == [w + (hm.CLASSES[int(r["cls_minor"])], hm.CLASSES[int(r["cls_major"])]) for w, r in zip(want, records)]
    hm.write_pairs(path, records[:0], 31, True)
    assert hm.read_pairs(path) == [] and os.path.getsize(path) == 0
    open(path, "w").write("ACG\t3\tAGG\n")
    with pytest.raises(ValueError, match="line 1"):
        hm.read_pairs(path)


def test_report_lines():
    from trio_binning_amd import hetmers as hm

    origin = np.arange(16, dtype=np.uint64).reshape(4, 4)
    result = {"candidates": 1000, "pairs": 120, "partners": np.array([700, 240, 36, 24], dtype=np.uint64), "origin": origin}
    alone = dict(line.split("\t") for line in hm.report(result, 21, False, (5, 49)))
    assert alone == {"k": "21", "space": "plain", "range": "5,49", "candidates": "1000", "candidates_with_0_partners": "700",
                     "candidates_with_1_partners": "240", "candidates_with_2_partners": "36", "candidates_with_3_partners": "24", "pairs": "120",
                     "candidates_in_pairs_share": "0.240000"}
    trio = dict(line.split("\t") for line in hm.report(result, 21, True, (5, 49), ((2, 40), (3, 60))))
    assert trio["space"] == "compressed" and trio["range_a"] == "2,40" and trio["range_b"] == "3,60"
    assert trio["pairs_minor_a_only_major_b_only"] == "6" and trio["pairs_minor_b_only_major_a_only"] == "9" and trio["pairs_minor_both_major_neither"] == "12"
    assert trio["pairs_split_between_parents"] == "15" and trio["pairs_split_between_parents_share"] == "0.125000"
    assert trio["pairs_inside_one_parent"] == "15" and trio["pairs_with_a_member_in_neither"] == str(0 + 1 + 2 + 3 + 4 + 8 + 12)
    empty = {"candidates": 0, "pairs": 0, "partners": np.zeros(4, dtype=np.uint64), "origin": np.zeros((4, 4), dtype=np.uint64)}
    assert dict(line.split("\t") for line in hm.report(empty, 21, False, (1, 255), ((1, 255), (1, 255))))["pairs_split_between_parents_share"] == "nan"
