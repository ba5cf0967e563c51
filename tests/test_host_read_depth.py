"""What of python -m trio_binning_amd.read_depth needs no device: the refusals it makes from its arguments and the database's
header alone, the rule on hand-made records - held to tests/read_depth_ref.py's, which is written in Python integers - and on
arrays cut into uneven batches, the --table, --spectrum and summary lines, and the new symbol's signature."""
import os

import numpy as np
import pytest

import kmerdb_files as kf
import read_depth_ref as rd
from conftest import DATA, ROOT


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "library.tbkdb"), "full": str(tmp_path / "full.tbkdb"), "hpc": str(tmp_path / "hpc.tbkdb"),
             "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"), "table": str(tmp_path / "table.tsv"),
             "spectrum": str(tmp_path / "depth.tsv"), "bam": str(tmp_path / "reads.bam")}
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
    from trio_binning_amd import read_depth

    with pytest.raises(SystemExit) as ei:
        read_depth.main(argv + ["--table", files["table"], "--spectrum", files["spectrum"]])
    for side in (files["table"], files["spectrum"]):
        assert not os.path.exists(side) and not os.path.exists(side + ".tmp")
    assert not [name for name in os.listdir(".") if name.startswith(("kept", "dropped", "unjudged"))]
    return ei.value.code


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["reads", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "reads" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("read_depth: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("read_depth: ") and files["list"] in code
    assert "is not a count database (*.tbkdb)" in code and "k-mer list holds no counts" in code
    assert capsys.readouterr().out == ""


def test_a_compressed_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["hpc"]])
    assert isinstance(code, str) and code.startswith("read_depth: ") and files["hpc"] in code
    assert "holds homopolymer-compressed k-mers (find-unique-kmers --compress)" in code and "out of scope here. Give a plain database." in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("options, word", [
    (["--min-count", "0"], "--min-count"), (["--min-count", "256"], "--min-count"), (["--min-count", "-2"], "--min-count"),
    (["--min-depth", "-1"], "--min-depth"), (["--min-depth", "256"], "--min-depth"), (["--max-depth", "256"], "--max-depth"),
    (["--max-depth", "-1"], "--max-depth"), (["--min-depth", "10", "--max-depth", "9"], "--min-depth"),
    (["--target", "0"], "--target"), (["--target", "256"], "--target"), (["--target", "-3"], "--target"), (["--target", "2.5"], "--target"),
    (["--seed", "7"], "--seed without --target"), (["--seed", "0"], "--seed without --target"),
    (["--target", "30", "--seed", "-1"], "--seed"), (["--target", "30", "--seed", str(1 << 64)], "--seed"),
    (["--by", "mean"], "--by"), (["--by", "present_median"], "--by")])
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
    from trio_binning_amd import read_depth

    args = read_depth.parse_args([files["fa"], files["db"]])
    assert args.info["k"] == 21 and (args.min_count, args.by, args.min_depth, args.max_depth, args.target, args.seed) == (1, "median", 0, 255, None, 0)
    assert (args.threshold, args.table, args.spectrum) == (2, None, None)  # a solid database: the bound in force is its floor
    assert (args.kept_out_prefix, args.dropped_out_prefix, args.unjudged_out_prefix) == ("kept", "dropped", "unjudged")
    assert read_depth.parse_args([files["fa"], files["full"]]).threshold == 1
    args = read_depth.parse_args([files["bam"], files["full"], "--min-count", "255", "--by", "present-median", "--min-depth", "255", "--max-depth", "255",
                                  "--target", "255", "--seed", str((1 << 64) - 1), "--bam-output"])
    assert (args.threshold, args.by, args.min_depth, args.max_depth, args.target, args.seed) == (255, "present-median", 255, 255, 255, (1 << 64) - 1)
    assert read_depth.parse_args([files["fa"], files["db"], "--min-depth", "7", "--max-depth", "7", "--target", "1"]).target == 1
    with pytest.raises(AssertionError, match="the device was touched"):
        read_depth.main([files["fa"], files["db"], "--table", files["table"], "--spectrum", files["spectrum"]])
    for side in (files["table"], files["spectrum"]):
        assert not os.path.exists(side + ".tmp") and not os.path.exists(side)


def test_help_says_what_the_rule_is(built, capsys):
    from trio_binning_amd import read_depth

    with pytest.raises(SystemExit) as ei:
        read_depth.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "No verdict about the library is computed" in text and "u * s >= T * 2^32" in text
    assert "lower bound" in " ".join(read_depth.decide.__doc__.split())  # a saturated read is thinned as if its depth were 255


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def _records(rng, n):
    """n records that need not come from any sequence: the rule looks at one field and at clean == 0"""
    recs = []
    for i in range(n):
        six = sorted(int(v) for v in rng.integers(0, 256, 5)) + [int(rng.integers(0, 256))]
        if i % 7 == 3:
            six = [255] * 6
        recs.append((0,) * 10 if i % 11 == 5 else (int(rng.integers(1, 5000)), 3, 2, 1, *six))
    return recs


def _decide(recs, ordinals=None, **rule):
    from trio_binning_amd import read_depth

    ordinals = list(range(len(recs))) if ordinals is None else ordinals
    got = read_depth.decide(rd.as_array(recs), np.array(ordinals, dtype=np.uint64), **rule)
    want = "".join(rd.bin_of(rec, i, **rule) for rec, i in zip(recs, ordinals))
    assert isinstance(got, bytes) and got.decode() == want, rule
    return want


def test_the_draws_are_splitmix64(built):
    from trio_binning_amd import read_depth

    assert read_depth.draws(0, np.arange(3)).tolist() == [3793791033, 1853398634, 113532184]
    ordinals = [0, 1, 2, 1000, (1 << 32) - 1, 1 << 32, (1 << 63) + 5, (1 << 64) - 2]
    for seed in (0, 1, 12345, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        got = read_depth.draws(seed, np.array(ordinals, dtype=np.uint64))
        assert got.dtype == np.uint64 and got.tolist() == [rd.draw(seed, i) for i in ordinals], seed


def test_the_rule_on_hand_made_records(built):
    from trio_binning_amd import kmers, read_depth

    assert kmers.READ_DEPTH == rd.READ_DEPTH and kmers.READ_DEPTH.names == rd.FIELDS + ("pad",)
    assert set(read_depth.STATISTICS) == set(rd.STATISTICS) and all(rd.FIELDS[rd.STATISTICS[b]] == f for b, f in read_depth.STATISTICS.items())
    #       clean present saturated sum  lowest q1 median q3 highest present_median
    recs = [(80, 80, 0, 2400,             20, 28, 30, 33, 90, 30), (0,) * 10, (80, 10, 0, 300, 0, 0, 0, 0, 40, 30), (80, 80, 70, 20000, 9, 255, 255, 255, 255, 255),
            (5, 5, 0, 500, 100, 100, 100, 100, 100, 100), (1, 1, 0, 31, 31, 31, 31, 31, 31, 31)]
    assert _decide(recs) == "AUAAAA"  # the defaults keep every judged read; no clean window is unjudged whatever the rule
    assert _decide(recs, min_depth=1) == "AUBAAA"
    assert _decide(recs, min_depth=1, by="present-median") == "AUAAAA"
    assert _decide(recs, min_depth=30, max_depth=31) == "AUBBBA" and _decide(recs, min_depth=31, max_depth=31) == "BUBBBA"
    assert _decide(recs, max_depth=254) == "AUABAA" and _decide(recs, max_depth=254, by="lowest") == "AUAAAA"
    assert _decide(recs, by="q1", min_depth=29) == "BUBAAA" and _decide(recs, by="q3", max_depth=32) == "BUABBA"
    assert _decide(recs, by="highest", max_depth=40) == "BUABBA"
    # --target 88 and 89 at the fifth read: u(0, 4) of 2^32 against T / 100; the reads at or below the target are never drawn for
    u4 = rd.draw(0, 4)
    edge = u4 * 100 // (1 << 32)  # the largest T that still drops the read
    assert 1 <= edge < 100
    assert _decide(recs, target=edge)[4] == "B" and _decide(recs, target=edge + 1)[4] == "A"
    assert _decide(recs, target=255) == "AUAAAA"  # 255 is not above 255: a saturated read is never thinned further than that
    saturated = "B" if rd.draw(0, 3) * 255 >= 100 << 32 else "A"
    assert _decide(recs, target=100) == "AUA" + saturated + "AA"  # the fifth read is at the target: not drawn for
    assert _decide(recs, target=30, min_depth=1, max_depth=200)[1:4] == "UBB"
    assert read_depth.decide(rd.as_array([]), np.zeros(0, dtype=np.uint64)) == b""
    with pytest.raises(ValueError):
        read_depth.decide(rd.as_array(recs), np.arange(5, dtype=np.uint64))


@pytest.mark.parametrize("by", sorted(rd.STATISTICS))
def test_the_rule_against_the_reference(built, by):
    rng = np.random.default_rng(2800)
    recs = _records(rng, 3000)
    for rule in ({}, {"min_depth": 20, "max_depth": 200}, {"target": 40}, {"target": 40, "seed": 99}, {"target": 1, "seed": (1 << 64) - 1},
                 {"target": 254, "min_depth": 3}, {"target": 120, "max_depth": 250, "seed": 1 << 63}):
        want = _decide(recs, by=by, **rule)
        assert "U" in want and "A" in want
    assert _decide(recs, by=by, target=40) != _decide(recs, by=by, target=40, seed=99)  # another seed thins other reads
    thinned = _decide(recs, by=by, target=40)
    assert "B" in thinned and all(b == "A" for b, rec in zip(thinned, recs) if rec[0] and rec[rd.STATISTICS[by]] <= 40)


def test_batches_of_uneven_size_decide_as_one_array(built):
    from trio_binning_amd import read_depth

    rng = np.random.default_rng(2801)
    recs = _records(rng, 1000)
    arr = rd.as_array(recs)
    for rule in ({"target": 40}, {"target": 40, "seed": 7, "by": "q3"}, {"min_depth": 9, "target": 100, "by": "present-median"}):
        whole = read_depth.decide(arr, np.arange(1000, dtype=np.uint64), **rule)
        assert whole.decode() == rd.bins_of(recs, **rule) and b"B" in whole
        for cuts in ((1, 2, 5, 400, 401, 999), (3, 6, 9, 12), (500,), tuple(range(1, 1000, 37))):
            edges = (0,) + cuts + (1000,)
            parts = [read_depth.decide(arr[a:b], np.arange(a, b, dtype=np.uint64), **rule) for a, b in zip(edges, edges[1:])]
            assert b"".join(parts) == whole, (rule, cuts)
        assert read_depth.decide(arr[10:20], np.arange(10, dtype=np.uint64), **rule) == rd.bins_of(recs[10:20], **rule).encode()  # the ordinals decide


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def test_the_summary_the_table_and_the_spectrum(built):
    from trio_binning_amd import read_depth

    recs = [(80, 80, 0, 2400, 20, 28, 30, 33, 90, 30), (0,) * 10, (80, 10, 0, 300, 0, 0, 0, 0, 40, 30), (96, 96, 90, 24000, 9, 255, 255, 255, 255, 255),
            (60, 60, 0, 1800, 29, 30, 30, 30, 31, 30)]
    names, sequences = ["m64011_1/1/ccs", "short one", "r3", "chloroplast", "r5"], ["A" * 100, "ACGTN", "C" * 100, "G" * 116, "T" * 80]
    lengths = [len(s) for s in sequences]
    arr = rd.as_array(recs)
    bins = read_depth.decide(arr, np.arange(5, dtype=np.uint64), min_depth=1, max_depth=254)
    assert bins == b"AUBBA" == rd.bins_of(recs, min_depth=1, max_depth=254).encode()
    assert read_depth.table_lines(names, lengths, arr, bins) == rd.table(names, sequences, recs, "AUBBA") == \
        "m64011_1/1/ccs\t100\t80\t80\t0\t2400\t20\t28\t30\t33\t90\t30\tkept\nshort one\t5\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\tunjudged\n" \
        "r3\t100\t80\t10\t0\t300\t0\t0\t0\t0\t40\t30\tdropped\nchloroplast\t116\t96\t96\t90\t24000\t9\t255\t255\t255\t255\t255\tdropped\n" \
        "r5\t80\t60\t60\t0\t1800\t29\t30\t30\t30\t31\t30\tkept\n"
    assert read_depth.TABLE_COLUMNS == ("name", "length", "clean", "present", "saturated", "sum", "lowest", "q1", "median", "q3", "highest", "present_median", "bin")

    # the spectrum: the judged reads by their statistic; two batches add up
    rows = read_depth.spectrum_rows(arr[:2], lengths[:2], bins[:2]) + read_depth.spectrum_rows(arr[2:], lengths[2:], bins[2:])
    text = read_depth.spectrum_lines(rows)
    assert text == rd.spectrum(sequences, recs, "AUBBA") and text.count("\n") == 256
    lines = text.splitlines()
    assert lines[0] == "0\t1\t100\t0\t0" and lines[30] == "30\t2\t180\t2\t180" and lines[255] == "255\t1\t116\t0\t0" and lines[1] == "1\t0\t0\t0\t0"
    by_q1 = read_depth.spectrum_lines(read_depth.spectrum_rows(arr, lengths, bins, "q1"))
    assert by_q1 == rd.spectrum(sequences, recs, "AUBBA", "q1") and by_q1.splitlines()[28] == "28\t1\t100\t1\t100"
    assert read_depth.SPECTRUM_COLUMNS == ("depth", "reads", "bases", "kept_reads", "kept_bases")

    class Args:
        threshold, by, min_depth, max_depth, target, seed = 2, "median", 1, 254, None, 0

    tally = {ord("A"): [2, 180], ord("B"): [2, 216], ord("U"): [1, 5]}
    assert read_depth.summary_lines(tally, Args) == rd.summary(sequences, "AUBBA", 2, "median", 1, 254) == \
        "#kept\t2\t180\n#dropped\t2\t216\n#unjudged\t1\t5\n#rule\t2\tmedian\t1\t254\t-\t0\n"
    Args.target, Args.seed, Args.by = 60, 11, "present-median"
    assert read_depth.summary_lines(tally, Args) == rd.summary(sequences, "AUBBA", 2, "present-median", 1, 254, 60, 11)
    assert read_depth.summary_lines(tally, Args).endswith("#rule\t2\tpresent-median\t1\t254\t60\t11\n")
    assert read_depth.RULE_COLUMNS == ("#rule", "min_count", "by", "min_depth", "max_depth", "target", "seed")
    assert read_depth.BINS == ("kept", "dropped", "unjudged")


# ---- the symbol and the documents --------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_header(built):
    from trio_binning_amd import _lib

    assert _lib.HAS_DB_READ_DEPTH and hasattr(_lib.lib, "tbk_kmerdb_query_read_depth") and hasattr(_lib.lib, "tbk_kmerdb_query_read_depth_times_")
    assert _lib.lib.tbk_kmerdb_query_read_depth(None, None, None, 0, 1, None) == _lib.TBK_ERR_INVALID  # a NULL session, before any device
    assert "query is NULL" in _lib.last_error()
    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    assert "tbk_kmerdb_query_read_depth(" in header and "typedef struct tbk_read_depth" in header and "---- read depth" in header
    assert header.index("---- read evidence") < header.index("---- read depth") < header.index("tbk_host_threads")
    assert "floor(j (clean - 1) / 4)" in header and "present_median" in header and "No byte per base comes home" in header
    assert "#define TBK_ABI_VERSION 1" in header
    for document, word in (("README.md", "trio_binning_amd.read_depth"), ("DESIGN.md", "tbk_read_depth.hip"), ("INTEGRATION.md", "tbk_kmerdb_query_read_depth"),
                           (os.path.join("tools", "README.md"), "measure_read_depth.py"), (os.path.join("profiles", "r28", "README.md"), "tbk_read_depth_kernel")):
        assert word in open(os.path.join(ROOT, document)).read(), document
