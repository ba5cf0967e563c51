"""classify-by-kmers with count databases (*.tbkdb) in place of its two k-mer lists: what the command line refuses from the
arguments and the files' headers alone.  No GPU: every refusal here must come before anything loads a list, loads a
database or builds a classifier - those entry points are replaced by ones that fail the test."""
import os
from unittest.mock import patch

import pytest

import kmerdb_files as kf
from conftest import DATA


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    """Sound database files (k = 21 twice, k = 16), a text list, and a driver in which touching the device is a failure."""
    import trio_binning_amd.classify_by_kmers as cbk
    from trio_binning_amd import kmers

    paths = {}
    for name, k, seed in (("a21", 21, 1), ("b21", 21, 2), ("c16", 16, 3)):
        paths[name] = str(tmp_path / (name + ".tbkdb"))
        with open(paths[name], "wb") as fh:
            fh.write(kf.sound(k=k, n=5, seed=seed)[0])
    paths["list"] = os.path.join(DATA, "hapA.txt")
    paths["reads"] = os.path.join(DATA, "test.fastq")
    paths["bins"] = tmp_path / "bins"
    paths["bins"].mkdir()

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers, "create_kmer_hash_set", touched)
    monkeypatch.setattr(kmers.HashSet, "from_file", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique_set", touched)
    monkeypatch.setattr(kmers, "device_mem_info", touched)
    monkeypatch.setattr(cbk, "make_classifier", touched)
    return paths


def _exit(files, argv):
    """Run the driver; it must leave through SystemExit.  Returns the exit's code (a message or a number)."""
    import trio_binning_amd.classify_by_kmers as cbk

    prefixes = ["--haplotype-a-out-prefix", str(files["bins"] / "hapA"), "--haplotype-b-out-prefix", str(files["bins"] / "hapB"),
                "--unclassified-out-prefix", str(files["bins"] / "unclassified")]
    with patch("sys.argv", ["classify-by-kmers"] + argv + prefixes):
        with pytest.raises(SystemExit) as ei:
            cbk.main()
    assert os.listdir(files["bins"]) == []
    return ei.value.code


@pytest.mark.parametrize("order", ["list_first", "database_first"])
def test_a_list_beside_a_database_is_refused(files, capsys, order):
    pair = [files["list"], files["b21"]] if order == "list_first" else [files["a21"], files["list"]]
    code = _exit(files, [files["reads"]] + pair)
    assert isinstance(code, str) and pair[0] in code and pair[1] in code and "k-mer list" in code and "count database" in code
    assert capsys.readouterr().out == ""


def test_databases_of_different_k_are_refused(files, capsys):
    code = _exit(files, [files["reads"], files["a21"], files["c16"]])
    assert isinstance(code, str) and "21-mers" in code and "16-mers" in code and files["a21"] in code and files["c16"] in code
    code = _exit(files, [files["reads"], files["c16"], files["b21"], "--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"])
    assert isinstance(code, str) and "21-mers" in code and "16-mers" in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("half", [["--min-count-a", "3"], ["--max-count-a", "30"], ["--min-count-b", "3"], ["--max-count-b", "30"],
                                  ["--min-count-a", "3", "--max-count-a", "30", "--max-count-b", "9"]])
def test_half_a_pair_of_cutoffs_is_a_parser_error(files, capsys, half):
    code = _exit(files, [files["reads"], files["a21"], files["b21"]] + half)
    hap = "b" if "--max-count-b" in half or "--min-count-b" in half else "a"
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-{0} and --max-count-{0} go together".format(hap) in err


def test_cutoffs_out_of_order_are_a_parser_error(files, capsys):
    code = _exit(files, [files["reads"], files["a21"], files["b21"], "--min-count-a", "9", "--max-count-a", "3"])
    assert code == 2 and "need 1 <= min <= max" in capsys.readouterr().err


@pytest.mark.parametrize("hap", ["a", "b"])
def test_cutoffs_with_text_lists_are_a_parser_error(files, capsys, hap):
    code = _exit(files, [files["reads"], files["list"], os.path.join(DATA, "hapB.txt"), "--min-count-" + hap, "3", "--max-count-" + hap, "30"])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count-" + hap in err and "k-mer list" in err


def test_a_histogram_without_cutoffs_names_the_four_options(files, capsys):
    """kmerdb_files.sound() scatters five counters over 2..255: the reference's rule finds no minimum and maximum there."""
    from trio_binning_amd import find_unique_kmers as fu

    hist = kf.sound(k=21, n=5, seed=1)[3]
    with pytest.raises(fu.HistogramError):
        fu.analyze_histogram([(c, 0 if c == 1 else int(hist[c])) for c in range(1, 256)])
    code = _exit(files, [files["reads"], files["a21"], files["b21"]])
    assert isinstance(code, str) and files["a21"] in code
    for option in ("--min-count-a", "--max-count-a", "--min-count-b", "--max-count-b"):
        assert option in code
    assert capsys.readouterr().out == ""


def test_cutoffs_by_hand_pass_the_checks_and_reach_the_loader(files, capsys):
    """With both pairs given nothing is left to refuse: the next thing the driver does is load the databases."""
    import trio_binning_amd.classify_by_kmers as cbk

    argv = [files["reads"], files["a21"], files["b21"], "--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "4", "--max-count-b", "255"]
    with patch("sys.argv", ["classify-by-kmers"] + argv):
        args = cbk.parse_args()
        assert args.databases.paths == {"A": files["a21"], "B": files["b21"]} and args.databases.ranges == {"A": (2, 9), "B": (4, 255)}
        with pytest.raises(AssertionError, match="device was touched"):
            cbk.main()
    out, err = capsys.readouterr()
    assert out == "" and "Using counts in range [2,9]." in err and "Using counts in range [4,255]." in err


def test_help_lists_what_it_listed_and_the_new_options(built, capsys):
    from trio_binning_amd.classify_by_kmers import main

    with patch("sys.argv", ["classify-by-kmers", "--help"]):
        with pytest.raises(SystemExit) as ei:
            main()
    assert ei.value.code == 0
    out, _ = capsys.readouterr()
    assert "Classify reads into bins" in out
    out = " ".join(out.split())
    for flag, default in (("--haplotype-a-out-prefix", "hapA"), ("--haplotype-b-out-prefix", "hapB"),
                          ("--unclassified-out-prefix", "unclassified"), ("--no-gzip-output", "False")):
        assert flag in out and f"default: {default}" in out
    for word in ("reads", "haplotype_a_kmers", "haplotype_b_kmers", "one per line", "fasta/q format", ".tbkdb",
                 "--min-count-a", "--max-count-a", "--min-count-b", "--max-count-b"):
        assert word in out, word
