"""The child's options on both command lines (find-unique-kmers --child / --min-count-child, classify-by-kmers --child-database /
--min-count-child): what is refused from the arguments and the files' headers alone, and the pass planner's third database.
No GPU: every refusal must come before anything is counted or loaded - those entry points are replaced by ones that fail the
test, as in tests/test_host_classify_db_args.py."""
import os
from unittest.mock import patch

import pytest

import kmerdb_files as kf
from conftest import DATA


def _rising(k, seed):
    """A sound file whose histogram has the reference's minimum at 4 (rows 2.. fall, rise from 5 on, fall below row 4 at 12)."""
    import numpy as np

    per_row = {2: 9, 3: 5, 4: 2, 5: 4, 6: 7, 7: 9, 8: 8, 9: 6, 10: 4, 11: 3, 12: 1}
    counts = np.concatenate([np.full(n, c, dtype=np.uint8) for c, n in per_row.items()])
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(1 << min(2 * k, 40), size=counts.size, replace=False).astype(np.uint64))
    counts = rng.permutation(counts)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 7
    hist[0] = counts.size + 7
    return kf.file_bytes(k, keys, counts, hist, reads=11, bases=1234)


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    """Sound database files - scattered counters (no cut-offs to find) at k = 21 three times and k = 16, one with a histogram
    that has them - a text list, and drivers in which touching the device is a failure."""
    import trio_binning_amd.classify_by_kmers as cbk
    import trio_binning_amd.find_unique_kmers as fu
    from trio_binning_amd import kmers

    paths = {}
    for name, k, seed in (("a21", 21, 1), ("b21", 21, 2), ("c21", 21, 4), ("c16", 16, 3)):
        paths[name] = str(tmp_path / (name + ".tbkdb"))
        with open(paths[name], "wb") as fh:
            fh.write(kf.sound(k=k, n=5, seed=seed)[0])
    paths["rising21"] = str(tmp_path / "rising21.tbkdb")
    with open(paths["rising21"], "wb") as fh:
        fh.write(_rising(21, 5))
    paths["list"] = os.path.join(DATA, "hapA.txt")
    paths["reads"] = os.path.join(DATA, "test.fastq")
    paths["bins"] = tmp_path / "bins"
    paths["bins"].mkdir()
    paths["out"] = tmp_path / "out"
    paths["out"].mkdir()

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers, "create_kmer_hash_set", touched)
    monkeypatch.setattr(kmers.HashSet, "from_file", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique_set", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique", touched)
    monkeypatch.setattr(kmers, "KmerCounter", touched)
    monkeypatch.setattr(kmers, "device_mem_info", touched)
    monkeypatch.setattr(cbk, "make_classifier", touched)
    monkeypatch.setattr(fu, "count_library", touched)
    return paths


def _classify_exit(files, argv):
    import trio_binning_amd.classify_by_kmers as cbk

    prefixes = ["--haplotype-a-out-prefix", str(files["bins"] / "hapA"), "--haplotype-b-out-prefix", str(files["bins"] / "hapB"),
                "--unclassified-out-prefix", str(files["bins"] / "unclassified")]
    with patch("sys.argv", ["classify-by-kmers"] + argv + prefixes):
        with pytest.raises(SystemExit) as ei:
            cbk.main()
    assert os.listdir(files["bins"]) == []
    return ei.value.code


def _find_exit(files, argv):
    import trio_binning_amd.find_unique_kmers as fu

    with pytest.raises(SystemExit) as ei:
        fu.main(["-k", "21", "-o", str(files["out"]), "-s", str(files["out"])] + argv)
    assert os.listdir(files["out"]) == []
    return ei.value.code


# ---- find-unique-kmers ------------------------------------------------------------------------------------------------
def test_find_min_count_child_without_a_child_is_refused(files, capsys):
    code = _find_exit(files, ["--min-count-child", "3", files["a21"], files["b21"]])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-child" in err and "--child" in err.replace("--min-count-child", "")


@pytest.mark.parametrize("value", ["0", "-4"])
def test_find_min_count_child_below_1_is_refused(files, capsys, value):
    code = _find_exit(files, ["--child", files["c21"], "--min-count-child", value, files["a21"], files["b21"]])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-child" in err and "1 <= min" in err


def test_find_a_child_database_of_another_k_is_refused(files, capsys):
    code = _find_exit(files, ["--child", files["c16"], files["a21"], files["b21"]])
    assert isinstance(code, str) and files["c16"] in code and "16-mers" in code and "-k 21" in code
    # read files for the parents change nothing: the child's header is read before anything is counted
    code = _find_exit(files, ["--child", files["c16"], "--min-count-child", "3", files["reads"], files["reads"]])
    assert isinstance(code, str) and files["c16"] in code and "16-mers" in code
    assert capsys.readouterr().out == ""


def test_find_a_sound_child_passes_the_checks_and_reaches_the_loader(files, capsys):
    """With nothing left to refuse the next thing the driver does is load the first parent's database."""
    import trio_binning_amd.find_unique_kmers as fu

    argv = ["-k", "21", "-o", str(files["out"]), "-s", str(files["out"]), "--child", files["c21"], "--min-count-child", "3",
            "--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9", files["a21"], files["b21"]]
    args = fu.parse_args(argv)
    assert args.child == files["c21"] and args.min_count_child == 3
    with pytest.raises(AssertionError, match="device was touched"):
        fu.main(argv)
    assert fu.parse_args(argv[:6] + argv[-2:]).child is None


# ---- the pass planner ---------------------------------------------------------------------------------------------------
def test_choose_passes_with_three_databases():
    """budget = free * 4 // 5; one pass needs 4 * table(1); P passes need store + 3 * table(P) + databases * 9 * (capacity // 8),
    table(P) = ceil(capacity / P) * 80 // 3, store = ceil(bases / 2).

    capacity 1e9, bases 2e10, free 66.25e9: budget 53e9; 4 * table(1) = 106.7e9 does not fit; store 1e10; a database 1.125e9.
      table(2) = 13 333 333 333: 3 * table(2) = 40e9; two databases leave 53 - 10 - 2.25 = 40.75e9: P = 2;
      three leave 53 - 10 - 3.375 = 39.625e9 < 40e9, and 3 * table(3) = 3 * 8 888 888 906 = 26.7e9 fits: P = 3.
    capacity 1e7, bases 1.5e8, free 1e9: budget 8e8; 4 * table(1) = 4 * 266 666 666 > 8e8; store 7.5e7; a database 11.25e6;
      3 * table(2) = 3 * 133 333 333 = 4e8 <= 8e8 - 7.5e7 - 33.75e6: P = 2 with two databases and with three."""
    from trio_binning_amd.find_unique_kmers import choose_passes

    big = (1_000_000_000, 20_000_000_000, 66_250_000_000)
    small = (10_000_000, 150_000_000, 1_000_000_000)
    assert choose_passes(*big, databases=3) == 3 and choose_passes(*small, databases=3) == 2
    # without the keyword: today's values, those of two databases
    assert choose_passes(*big) == choose_passes(*big, databases=2) == 2
    assert choose_passes(*small) == choose_passes(*small, databases=2) == 2
    # where one pass fits nothing is left behind to plan for
    assert choose_passes(1_000_000, 10_000_000, 1_000_000_000, databases=3) == choose_passes(1_000_000, 10_000_000, 1_000_000_000) == 1
    # the edge itself: 3 * table(2) + store + three databases = 53 375 000 000 - 1 exactly fits a budget of that size
    edge = 3 * 13_333_333_333 + 10_000_000_000 + 3 * 9 * 125_000_000
    assert choose_passes(1_000_000_000, 20_000_000_000, edge * 5 // 4 + 1, databases=3) == 2
    assert choose_passes(1_000_000_000, 20_000_000_000, (edge - 1) * 5 // 4, databases=3) == 3


# ---- classify-by-kmers --------------------------------------------------------------------------------------------------
def test_classify_a_child_database_with_text_lists_is_a_parser_error(files, capsys):
    code = _classify_exit(files, [files["reads"], files["list"], os.path.join(DATA, "hapB.txt"), "--child-database", files["c21"]])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--child-database" in err and "k-mer list" in err


def test_classify_a_child_database_of_another_k_is_refused(files, capsys):
    cuts = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]
    code = _classify_exit(files, [files["reads"], files["a21"], files["b21"], "--child-database", files["c16"]] + cuts)
    assert isinstance(code, str) and "21-mers" in code and "16-mers" in code and files["c16"] in code
    assert capsys.readouterr().out == ""


def test_classify_min_count_child_needs_the_database_and_a_value_from_1_on(files, capsys):
    cuts = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]
    code = _classify_exit(files, [files["reads"], files["a21"], files["b21"], "--min-count-child", "3"] + cuts)
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-child" in err and "--child-database" in err
    code = _classify_exit(files, [files["reads"], files["a21"], files["b21"], "--child-database", files["c21"], "--min-count-child", "0"] + cuts)
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-child" in err and "1 <= min" in err


def test_classify_a_child_histogram_without_a_minimum_names_its_option(files, capsys):
    cuts = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]
    code = _classify_exit(files, [files["reads"], files["a21"], files["b21"], "--child-database", files["c21"]] + cuts)
    assert isinstance(code, str) and files["c21"] in code and "--min-count-child" in code
    assert capsys.readouterr().out == ""


def test_classify_the_child_is_settled_from_its_header_and_reaches_the_loader(files, capsys):
    import trio_binning_amd.classify_by_kmers as cbk

    cuts = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "4", "--max-count-b", "255"]
    for extra, want in ((["--child-database", files["rising21"]], 4), (["--child-database", files["rising21"], "--min-count-child", "7"], 7),
                        (["--child-database", files["c21"], "--min-count-child", "1"], 1)):
        with patch("sys.argv", ["classify-by-kmers", files["reads"], files["a21"], files["b21"]] + cuts + extra):
            args = cbk.parse_args()
            assert args.databases.paths == {"A": files["a21"], "B": files["b21"]} and args.databases.ranges == {"A": (2, 9), "B": (4, 255)}
            assert (args.databases.child_path, args.databases.child_min) == (extra[1], want)
            with pytest.raises(AssertionError, match="device was touched"):
                cbk.main()
        out, err = capsys.readouterr()
        assert out == "" and "Using counts in range [{},255] for the child.".format(want) in err
    with patch("sys.argv", ["classify-by-kmers", files["reads"], files["a21"], files["b21"]] + cuts):
        args = cbk.parse_args()
        assert args.databases.child_path is None


def test_help_names_the_childs_options(built, capsys):
    import trio_binning_amd.classify_by_kmers as cbk
    import trio_binning_amd.find_unique_kmers as fu

    with patch("sys.argv", ["classify-by-kmers", "--help"]):
        with pytest.raises(SystemExit) as ei:
            cbk.main()
    assert ei.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--child-database" in out and "--min-count-child" in out
    with pytest.raises(SystemExit) as ei:
        fu.parse_args(["--help"])
    assert ei.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--child FILES" in out and "--min-count-child" in out and "child.tbkdb" in out
