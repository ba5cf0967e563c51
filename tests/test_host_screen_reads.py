"""What of python -m trio_binning_amd.screen_reads needs no device: the refusals it makes from its arguments and the database's
header alone, the parsing of the shares, the rule on hand-made records - held to tests/screen_ref.py's, which is written with
fractions - the summary and the --table lines, and the new symbol's signature."""
import os
from fractions import Fraction

import numpy as np
import pytest

import kmerdb_files as kf
import screen_ref as sr
from conftest import DATA, ROOT


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "cloud.tbkdb"), "full": str(tmp_path / "full.tbkdb"), "hpc": str(tmp_path / "hpc.tbkdb"),
             "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"), "table": str(tmp_path / "table.tsv"),
             "bam": str(tmp_path / "reads.bam")}
    _, keys, counts, hist = kf.sound(k=21, n=5, seed=1)
    full_hist = np.bincount(counts, minlength=256).astype(np.uint64)  # (a full database's row 1 counts entries, row 0 all of them)
    full_hist[0] = counts.size
    for name, magic, rows in (("db", kf.MAGIC, hist), ("hpc", b"TBKKMDH1", hist), ("full", b"TBKKMFB1", full_hist)):
        with open(paths[name], "wb") as fh:
            fh.write(kf.file_bytes(21, keys, counts, rows, reads=11, bases=1234, magic=magic))
    with open(paths["bam"], "wb") as fh:
        fh.write(b"not read: the arguments are judged by the name")

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.DatabaseQuery, "__init__", touched)
    monkeypatch.chdir(tmp_path)  # (a bin that a refused run opened would lie here)
    return paths


def _exit(files, argv):
    from trio_binning_amd import screen_reads

    with pytest.raises(SystemExit) as ei:
        screen_reads.main(argv + ["--table", files["table"]])
    assert not os.path.exists(files["table"]) and not os.path.exists(files["table"] + ".tmp")
    assert not [name for name in os.listdir(".") if name.startswith(("matched", "unmatched", "unjudged"))]
    return ei.value.code


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["reads", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "reads" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("screen_reads: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("screen_reads: ") and files["list"] in code
    assert "is not a count database (*.tbkdb)" in code and "k-mer list holds no counts" in code
    assert capsys.readouterr().out == ""


def test_a_compressed_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["hpc"]])
    assert isinstance(code, str) and code.startswith("screen_reads: ") and files["hpc"] in code
    assert "holds homopolymer-compressed k-mers (find-unique-kmers --compress): coverage along a read is not defined in compressed space. " \
           "Give a plain database." in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("options, word", [
    (["--min-count", "0"], "--min-count"), (["--min-count", "256"], "--min-count"), (["--min-count", "-2"], "--min-count"),
    (["--max-count", "256"], "--max-count"), (["--max-count", "0"], "--max-count"), (["--min-count", "10", "--max-count", "9"], "--max-count"),
    (["--min-hits", "-1"], "--min-hits"), (["--min-stretch", "-1"], "--min-stretch"), (["--min-hits", str(1 << 63)], "--min-hits"),
    (["--min-share", "1.1"], "--min-share"), (["--min-share", "-0.1"], "--min-share"), (["--min-share", "1e-3"], "--min-share"),
    (["--min-share", "0.1234567891"], "--min-share"), (["--min-share", "half"], "--min-share"), (["--min-share", "1/2"], "--min-share"),
    (["--min-share", ""], "--min-share"), (["--min-share", "0.5\n"], "--min-share"), (["--min-covered", "2"], "--min-covered"),
    (["--min-covered", "+0.5"], "--min-covered"), (["--min-covered", "0.0000000001"], "--min-covered"), (["--min-covered", "nan"], "--min-covered")])
def test_values_out_of_bounds_are_refused(files, capsys, options, word):
    code = _exit(files, [files["fa"], files["db"]] + options)
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and word in err


def test_bam_output_needs_bam_input(files, capsys):
    code = _exit(files, [files["fa"], files["db"], "--bam-output"])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--bam-output keeps BAM records whole" in err and files["fa"] in err
    code = _exit(files, [files["bam"], files["db"], "--bam-output", "--no-gzip-output"])
    assert code == 2 and "exclude each other" in capsys.readouterr().err


def test_sound_arguments_reach_the_database(files, capsys):
    """the fixture's tripwire is what a sound command line meets first: nothing above was refused for another reason"""
    from trio_binning_amd import screen_reads

    args = screen_reads.parse_args([files["fa"], files["db"]])
    assert args.info["k"] == 21 and (args.min_count, args.max_count, args.min_hits, args.min_stretch, args.table) == (1, 255, 1, 0, None)
    assert (args.share, args.covered, args.threshold) == (0, 0, 2)  # a solid database: the bound in force is its floor
    assert (args.matched_out_prefix, args.unmatched_out_prefix, args.unjudged_out_prefix) == ("matched", "unmatched", "unjudged")
    assert screen_reads.parse_args([files["fa"], files["full"]]).threshold == 1
    args = screen_reads.parse_args([files["bam"], files["full"], "--min-count", "255", "--max-count", "255", "--min-share", "1", "--min-covered",
                                    "0.999999999", "--min-hits", "0", "--min-stretch", "40", "--bam-output"])
    assert (args.threshold, args.max_count, args.share, args.covered, args.min_hits, args.min_stretch) == (255, 255, 1, Fraction(999999999, 10 ** 9), 0, 40)
    assert screen_reads.parse_args([files["fa"], files["db"], "--min-count", "1", "--max-count", "1"]).threshold == 2  # empty after the floor: valid
    with pytest.raises(AssertionError, match="the device was touched"):
        screen_reads.main([files["fa"], files["db"], "--table", files["table"]])
    assert not os.path.exists(files["table"] + ".tmp") and not os.path.exists(files["table"])


def test_help_says_that_no_verdict_is_computed(built, capsys):
    from trio_binning_amd import screen_reads

    with pytest.raises(SystemExit) as ei:
        screen_reads.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "No verdict about the library is computed" in text and "held / clean >= --min-share" in text


# ---- the shares ------------------------------------------------------------------------------------------------------------------------
def test_shares_are_parsed_exactly(built):
    from trio_binning_amd import screen_reads

    for text, want in (("0", Fraction(0)), ("1", Fraction(1)), ("0.5", Fraction(1, 2)), (".25", Fraction(1, 4)), ("1.0", Fraction(1)),
                       ("0.1", Fraction(1, 10)), ("0.333333333", Fraction(333333333, 10 ** 9)), ("0.000000001", Fraction(1, 10 ** 9)),
                       ("1.000000000", Fraction(1)), ("00.50", Fraction(1, 2))):
        assert screen_reads.parse_share(text) == want, text
    assert screen_reads.parse_share("0.1") != 0.1  # (no float: 0.1 is not a tenth)
    for text in ("1.000000001", "2", "-0", "-0.5", "+1", "1e0", "0.5e-1", "", ".", "1.", "0.1234567890", "0,5", " 0.5", "0.5 ", "inf", "nan", "1/2", "0x1"):
        with pytest.raises(ValueError):
            screen_reads.parse_share(text)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def _decide(recs, lengths, **rule):
    from trio_binning_amd import screen_reads

    share, covered = rule.pop("min_share", "0"), rule.pop("min_covered", "0")
    got = screen_reads.decide(sr.as_array(recs), np.array(lengths, dtype=np.int64), min_share=screen_reads.parse_share(share),
                              min_covered=screen_reads.parse_share(covered), **rule)
    want = "".join(sr.bin_of(rec, n, min_share=share, min_covered=covered, **rule) for rec, n in zip(recs, lengths))
    assert isinstance(got, bytes) and got.decode() == want, (recs, rule)
    return want


def test_the_rule_on_hand_made_records(built):
    from trio_binning_amd import kmers, screen_reads

    assert kmers.READ_EVIDENCE == sr.READ_EVIDENCE and kmers.READ_EVIDENCE.names == sr.FIELDS
    #        clean held covered longest stretches
    recs = [(80, 40, 60, 30, 3), (0, 0, 0, 0, 0), (80, 0, 0, 0, 0), (80, 1, 21, 21, 1), (80, 80, 100, 100, 1), (3, 1, 3, 3, 1), (3, 2, 5, 5, 1)]
    lengths = [100, 15, 100, 100, 100, 9, 9]
    assert _decide(recs, lengths) == "AUBAAAA"  # the defaults: one hit matches; no clean window is unjudged whatever the rule
    assert _decide(recs, lengths, min_hits=0) == "AUAAAAA"
    assert _decide(recs, lengths, min_hits=2) == "AUBBABA"
    assert _decide(recs, lengths, min_hits=41) == "BUBBABB"
    # a share met exactly - 40 * 2 == 1 * 80 - and one missed by one window: 39 of 80
    assert _decide(recs, lengths, min_share="0.5") == "AUBBABA"
    assert _decide([(80, 39, 60, 30, 3), (80, 40, 60, 30, 3), (80, 41, 60, 30, 3)], [100] * 3, min_share="0.5") == "BAA"
    assert _decide([(3, 1, 3, 3, 1)] * 2, [9, 9], min_share="0.333333333") == "AA" and _decide([(3, 1, 3, 3, 1)], [9], min_share="0.333333334") == "B"
    assert _decide(recs, lengths, min_share="1") == "BUBBABB"
    assert _decide(recs, lengths, min_hits=0, min_share="1") == "BUBBABB"  # 0 of 80 is no share of 1
    # covered / length: 60 of 100 exactly, and one base short
    assert _decide(recs, lengths, min_covered="0.6") == "AUBBABB"
    assert _decide([(80, 40, 59, 30, 3), (80, 40, 60, 30, 3)], [100, 100], min_covered="0.6") == "BA"
    assert _decide([(80, 40, 60, 30, 3)] * 2, [100, 101], min_covered="0.6") == "AB"  # the same bases of a longer read
    assert _decide(recs, lengths, min_covered="1") == "BUBBABB"
    # the longest stretch
    assert _decide(recs, lengths, min_stretch=30) == "AUBBABB" and _decide(recs, lengths, min_stretch=31) == "BUBBABB"
    assert _decide(recs, lengths, min_stretch=21, min_share="0.0125") == "AUBAABB"  # 1 of 80 exactly
    assert _decide(recs, lengths, min_hits=2, min_share="0.5", min_covered="0.55", min_stretch=5) == "AUBBABA"
    # nothing at all, and numbers that no 64-bit product holds
    assert screen_reads.decide(sr.as_array([]), np.zeros(0, dtype=np.int64)) == b""
    big = 1 << 62
    assert _decide([(big, big // 2, big, big, 1), (big, big // 2 - 1, big, big, 1)], [big + 31] * 2, min_share="0.5", min_covered="0.999999999") == "AB"
    with pytest.raises(ValueError):
        screen_reads.decide(sr.as_array(recs), np.array(lengths[:-1]))


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def test_the_summary_and_the_table(built):
    from trio_binning_amd import screen_reads

    recs = [(80, 40, 60, 30, 3), (0, 0, 0, 0, 0), (80, 0, 0, 0, 0)]
    names, sequences = ["m64011_1/1/ccs", "short one", "r3"], ["A" * 100, "ACGTN", "C" * 100]
    bins = screen_reads.decide(sr.as_array(recs), np.array([100, 5, 100]))
    assert bins == b"AUB"
    assert screen_reads.table_lines(names, [100, 5, 100], sr.as_array(recs), bins) == sr.table(names, sequences, recs, "AUB") == \
        "m64011_1/1/ccs\t100\t80\t40\t60\t30\t3\tmatched\nshort one\t5\t0\t0\t0\t0\t0\tunjudged\nr3\t100\t80\t0\t0\t0\t0\tunmatched\n"
    assert screen_reads.TABLE_COLUMNS == ("name", "length", "clean", "held", "covered", "longest", "stretches", "bin")

    class Args:
        threshold, max_count, min_hits, min_share, min_covered, min_stretch = 2, 200, 1, "0.50", ".25", 7

    tally = {ord("A"): [1, 100], ord("B"): [1, 100], ord("U"): [1, 5]}
    assert screen_reads.summary_lines(tally, Args) == sr.summary(sequences, "AUB", 2, 200, 1, "0.50", ".25", 7) == \
        "#matched\t1\t100\n#unmatched\t1\t100\n#unjudged\t1\t5\n#rule\t2\t200\t1\t0.50\t.25\t7\n"  # the shares as given
    assert screen_reads.RULE_COLUMNS == ("#rule", "min_count", "max_count", "min_hits", "min_share", "min_covered", "min_stretch")


# ---- the symbol and the documents --------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_header(built):
    from trio_binning_amd import _lib

    assert _lib.HAS_DB_EVIDENCE and hasattr(_lib.lib, "tbk_kmerdb_query_evidence")
    assert _lib.lib.tbk_kmerdb_query_evidence(None, None, None, 0, 1, 255, None) == _lib.TBK_ERR_INVALID  # a NULL session, before any device
    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    assert "tbk_kmerdb_query_evidence(" in header and "typedef struct tbk_read_evidence" in header and "read evidence" in header
    assert "#define TBK_ABI_VERSION 1" in header
    for document, word in (("README.md", "screen_reads"), ("DESIGN.md", "screen_reads"), ("INTEGRATION.md", "tbk_kmerdb_query_evidence"),
                           (os.path.join("tools", "README.md"), "measure_screen.py")):
        assert word in open(os.path.join(ROOT, document)).read(), document
