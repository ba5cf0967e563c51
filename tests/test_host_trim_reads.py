"""What of python -m trio_binning_amd.trim_reads needs no device: the refusals it makes from its arguments and the database's
header alone, its bins, tables and summary on hand-made records - held to tests/pieces_ref.py's - the bin writer's cut of a batch's
records (seq.BinWriter.write_pieces, with the host's encoder) against the reference's text, byte for byte, and the new symbols'
signatures."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

import kmerdb_files as kf
import pieces_ref as pr
import screen_ref as sr
from conftest import DATA, ROOT


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "cloud.tbkdb"), "full": str(tmp_path / "full.tbkdb"), "hpc": str(tmp_path / "hpc.tbkdb"),
             "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"), "table": str(tmp_path / "table.tsv"),
             "bed": str(tmp_path / "pieces.bed"), "bam": str(tmp_path / "reads.bam")}
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
    from trio_binning_amd import trim_reads

    with pytest.raises(SystemExit) as ei:
        trim_reads.main(argv + ["--table", files["table"], "--bed", files["bed"]])
    for name in ("table", "bed"):
        assert not os.path.exists(files[name]) and not os.path.exists(files[name] + ".tmp")
    assert not [name for name in os.listdir(".") if name.startswith(("kept", "dropped", "unjudged"))]
    return ei.value.code


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["reads", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "reads" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("trim_reads: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("trim_reads: ") and files["list"] in code
    assert "is not a count database (*.tbkdb)" in code and "k-mer list holds no counts" in code
    assert capsys.readouterr().out == ""


def test_a_compressed_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["hpc"]])
    assert isinstance(code, str) and code.startswith("trim_reads: ") and files["hpc"] in code
    assert "holds homopolymer-compressed k-mers (find-unique-kmers --compress): the coordinates of a piece are not defined in compressed space. " \
           "Give a plain database." in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("options, word", [
    (["--min-count", "0"], "--min-count"), (["--min-count", "256"], "--min-count"), (["--min-count", "-2"], "--min-count"),
    (["--max-count", "256"], "--max-count"), (["--max-count", "0"], "--max-count"), (["--min-count", "10", "--max-count", "9"], "--max-count"),
    (["--min-length", "0"], "--min-length"), (["--min-length", "-5"], "--min-length"), (["--min-length", str(1 << 63)], "--min-length"),
    (["--min-length", "1.5"], "--min-length"), (["--keep", "both"], "--keep"), (["--keep", "COVERED"], "--keep"), (["--pieces", "first"], "--pieces"),
    (["--bam-output"], "--bam-output")])
def test_values_out_of_bounds_are_refused(files, capsys, options, word):
    code = _exit(files, [files["fa"], files["db"]] + options)
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and word in err


def test_sound_arguments_reach_the_database(files, capsys):
    """the fixture's tripwire is what a sound command line meets first: nothing above was refused for another reason"""
    from trio_binning_amd import trim_reads

    args = trim_reads.parse_args([files["fa"], files["db"]])
    assert args.info["k"] == 21 and (args.min_count, args.max_count, args.keep, args.pieces, args.min_length, args.table, args.bed) == \
        (1, 255, "covered", "longest", 1, None, None)
    assert args.threshold == 2  # a solid database: the bound in force is its floor
    assert (args.kept_out_prefix, args.dropped_out_prefix, args.unjudged_out_prefix) == ("kept", "dropped", "unjudged")
    assert trim_reads.parse_args([files["fa"], files["full"]]).threshold == 1
    args = trim_reads.parse_args([files["bam"], files["full"], "--min-count", "255", "--max-count", "255", "--keep", "uncovered", "--pieces", "all",
                                  "--min-length", "500", "--no-gzip-output"])
    assert (args.threshold, args.max_count, args.keep, args.pieces, args.min_length, args.no_gzip_output) == (255, 255, "uncovered", "all", 500, True)
    assert trim_reads.parse_args([files["fa"], files["db"], "--min-count", "1", "--max-count", "1"]).threshold == 2  # empty after the floor: valid
    with pytest.raises(AssertionError, match="the device was touched"):
        trim_reads.main([files["fa"], files["db"], "--table", files["table"], "--bed", files["bed"]])
    for name in ("table", "bed"):
        assert not os.path.exists(files[name] + ".tmp") and not os.path.exists(files[name])


def test_help_says_that_no_verdict_is_computed(built, capsys):
    from trio_binning_amd import trim_reads

    with pytest.raises(SystemExit) as ei:
        trim_reads.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "No verdict about the library is computed" in text and "name:F-E" in text and "so nothing vanishes" in text


# ---- bins, tables and summary ------------------------------------------------------------------------------------------------------------
def test_the_bins_the_tables_and_the_summary(built):
    from trio_binning_amd import kmers, trim_reads

    assert kmers.READ_PIECE == pr.READ_PIECE and kmers.READ_PIECE.itemsize == 24 and kmers.READ_PIECE.names == ("read", "first", "end")
    records = [("m64011_1/1/ccs c", "A" * 100, ""), ("short", "ACGTN", ""), ("r3", "C" * 100, ""), ("r4", "G" * 50, ""), ("none", "T" * 30, "")]
    #           clean held covered longest stretches
    evidence = [(80, 40, 60, 30, 3), (0, 0, 0, 0, 0), (80, 0, 0, 0, 0), (30, 30, 50, 50, 1), (10, 0, 0, 0, 0)]
    # the library's answer for some rule: read 1 has a piece and no clean window (the uncovered side of a short read)
    found = [(0, 0, 30), (0, 45, 60), (1, 0, 5), (3, 0, 50)]
    bins, kept = trim_reads.decide(sr.as_array(evidence), pr.as_array(found))
    assert bins == b"AUBAB" and kept.tobytes() == pr.as_array([(0, 0, 30), (0, 45, 60), (3, 0, 50)]).tobytes()
    want = [p for p in found if p[0] != 1]
    names = [header.split(" ")[0] for header, _, _ in records]
    lengths = [len(s) for _, s, _ in records]
    count, total = trim_reads.per_read(kept, 5)
    assert count.tolist() == [2, 0, 0, 1, 0] and total.tolist() == [45, 0, 0, 50, 0]
    assert trim_reads.table_lines(names, lengths, sr.as_array(evidence), count, total, bins) == pr.table(records, want, evidence, "AUBAB") == \
        "m64011_1/1/ccs\t100\t80\t40\t60\t2\t45\tkept\nshort\t5\t0\t0\t0\t0\t0\tunjudged\nr3\t100\t80\t0\t0\t0\t0\tdropped\n" \
        "r4\t50\t30\t30\t50\t1\t50\tkept\nnone\t30\t10\t0\t0\t0\t0\tdropped\n"
    assert trim_reads.bed_lines(names, kept) == pr.bed(records, want) == "m64011_1/1/ccs\t0\t30\nm64011_1/1/ccs\t45\t60\nr4\t0\t50\n"
    assert trim_reads.TABLE_COLUMNS == ("name", "length", "clean", "held", "covered", "pieces", "kept_bases", "bin")

    class Args:
        threshold, max_count, keep, pieces, min_length = 2, 200, "covered", "all", 15

    tally = {ord("A"): [2, 150], ord("B"): [2, 130], ord("U"): [1, 5]}
    assert trim_reads.summary_lines(tally, 3, 95, Args) == pr.summary(records, want, "AUBAB", 2, 200, "covered", "all", 15) == \
        "#kept\t2\t3\t95\n#dropped\t2\t130\n#unjudged\t1\t5\n#cut\t55\n#rule\t2\t200\tcovered\tall\t15\n"
    assert trim_reads.RULE_COLUMNS == ("#rule", "min_count", "max_count", "keep", "pieces", "min_length")
    bins, kept = trim_reads.decide(sr.as_array([]), pr.as_array([]))
    assert bins == b"" and kept.size == 0


# ---- the writer ----------------------------------------------------------------------------------------------------------------------------
def _records(rng, n, quality):
    """(header, sequence, quality) of n records: FASTQ with quality, FASTA without; some headers carry a comment"""
    out = []
    for i in range(n):
        length = rng.choice((1, 2, 7, 60, 150, 400))
        sequence = "".join(rng.choice("ACGTN") for _ in range(length))
        header = "read{}/{}".format(i, length) + (" a comment" if i % 3 == 0 else "")
        out.append((header, sequence, "".join(rng.choice("!#5I~") for _ in range(length)) if quality else ""))
    return out


def _source(path, records):
    with open(path, "w") as fh:
        for header, sequence, quality in records:
            fh.write("@{}\n{}\n+\n{}\n".format(header, sequence, quality) if quality else ">{}\n{}\n".format(header, sequence))


def _some_pieces(rng, records, bins):
    """pieces for the 'A' records: none, the whole record, one at offset 0, one that ends at L, or several - and some for other
    records too, which the writer must pass over"""
    found = []
    for i, ((_, sequence, _), code) in enumerate(zip(records, bins)):
        n = len(sequence)
        kind = i % 6 if code == "A" else rng.choice((0, 1))
        if kind == 1:
            found.append((i, 0, n))
        elif kind == 2 and n > 1:
            found.append((i, 0, rng.randrange(1, n)))
        elif kind == 3 and n > 1:
            found.append((i, rng.randrange(1, n), n))
        elif kind >= 4 and n >= 7:
            cuts = sorted(rng.sample(range(0, n + 1), 6))
            found += [(i, cuts[0], cuts[1]), (i, cuts[2], cuts[3]), (i, cuts[4], cuts[5])] if kind == 4 else [(i, cuts[0], cuts[1]), (i, cuts[1], cuts[5])]
    return [p for p in found if p[2] > p[1]]


def _read(path, gz):
    with (gzip.open(path, "rb") if gz else open(path, "rb")) as fh:
        return fh.read().decode()


@pytest.mark.parametrize("gz", [True, False])
@pytest.mark.parametrize("quality", [True, False])
@pytest.mark.parametrize("suffix", [True, False])
def test_writer_bytes_equal_the_reference(built, tmp_path, gz, quality, suffix):
    """two batch sizes: the second batch is appended to the first, and the pieces' read numbers count from the batch's first read"""
    from trio_binning_amd import seq

    rng = random.Random(31 + 2 * quality + suffix)
    records = _records(rng, 120, quality)
    bins = "".join(rng.choice("AAABU") for _ in records)
    found = _some_pieces(rng, records, bins)
    whole = [p for p in found if bins[p[0]] == "A" and (p[1], p[2]) == (0, len(records[p[0]][1]))]
    assert whole and any(p[1] == 0 and p not in whole for p in found) and any(p[2] == len(records[p[0]][1]) and p[1] for p in found)
    assert any(bins[i] == "A" and not [p for p in found if p[0] == i] for i in range(len(records)))  # 'A' reads without a piece
    assert max(sum(1 for p in found if p[0] == i) for i in range(len(records))) == 3
    want = pr.bins_text(records, found, bins, suffix)
    for p in whole:  # the whole record is the same bytes with and without the suffix
        assert pr.piece_text(*records[p[0]], p[1], p[2], suffix) == pr.record_text(*records[p[0]])
    src = tmp_path / ("in.fq" if quality else "in.fa")
    _source(src, records)
    for max_reads in (0, 7):
        w = seq.BinWriter(str(tmp_path / "ka"), str(tmp_path / "kb"), str(tmp_path / "ku"), ".fq" if quality else ".fa", gz, threads=3)
        done = 0
        with seq.BatchReader(str(src)) as r:
            b = seq.Batch()
            while r.next_batch(b, 0 if max_reads else 1 << 30, max_reads):
                mine = pr.as_array([(i - done, f, e) for i, f, e in found if done <= i < done + b.n_reads])
                w.write_pieces(b, mine, bins[done:done + b.n_reads].encode(), suffix)
                done += b.n_reads
            b.close()
        w.close()
        assert done == len(records)
        assert tuple(_read(name, gz) for name in w.names) == want, max_reads


def test_writer_takes_a_record_with_an_empty_quality(built, tmp_path):
    """a FASTQ record whose quality line is missing reads as one without quality values and is written as FASTA, whole or cut"""
    from trio_binning_amd import seq

    src = tmp_path / "odd.fq"
    src.write_text("@q1 x\nACGTACGT\n+\nIIIIJJJJ\n>fa c\nGGGGCC\n@q2\nTTTT\n+\n!!!!\n@noq\nACGTAC\n+\n")
    records = [("q1 x", "ACGTACGT", "IIIIJJJJ"), ("fa c", "GGGGCC", ""), ("q2", "TTTT", "!!!!"), ("noq", "ACGTAC", "")]
    found = [(0, 2, 5), (1, 0, 6), (2, 0, 1), (2, 1, 4), (3, 1, 6)]
    want = ("@q1:3-5\nGTA\n+\nIIJ\n>fa\nGGGGCC\n@q2:1-1\nT\n+\n!\n@q2:2-4\nTTT\n+\n!!!\n>noq:2-6\nCGTAC\n", "", "")
    assert pr.bins_text(records, found, "AAAA", True) == want
    for bins in ("AAAA", "ABUB", "UAAA"):
        w = seq.BinWriter(str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "u"), ".fq", False)
        done, seen = 0, []
        with seq.BatchReader(str(src)) as r:
            b = seq.Batch()
            while r.next_batch(b, 1 << 20, 0):
                seen += [(x.name, x.seq) for x in b.reads()]
                mine = pr.as_array([(i - done, f, e) for i, f, e in found if done <= i < done + b.n_reads])
                w.write_pieces(b, mine, bins[done:done + b.n_reads].encode(), True)
                done += b.n_reads
            b.close()
        w.close()
        assert seen == [(h.split(" ")[0], s) for h, s, _ in records]
        assert tuple(_read(name, False) for name in w.names) == pr.bins_text(records, found, bins, True), bins


def test_writer_refusals_leave_the_files_unwritten(built, tmp_path):
    from trio_binning_amd import _lib, seq

    src = tmp_path / "in.fq"
    src.write_text("@r0\nACGTACGT\n+\nIIIIJJJJ\n@r1\nACGTAC\n+\nIIIIII\n@r2\nTT\n+\n!!\n")
    plain = seq.BinWriter(str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "u"), ".fq", False)
    zipped = seq.BinWriter(str(tmp_path / "za"), str(tmp_path / "zb"), str(tmp_path / "zu"), ".fq", True)
    header = b"BAM\x01" + struct.pack("<ii", 0, 0)
    bam = seq.BinWriter(str(tmp_path / "A"), str(tmp_path / "B"), str(tmp_path / "U"), ".bam", True, bam_header=header)
    tagged = seq.BinWriter("", "", "", ".bam", True, bam_header=header, haplotag_path=str(tmp_path / "t.bam"))
    batch = seq.Batch()
    with seq.BatchReader(str(src)) as reader:
        assert reader.next_batch(batch, 1 << 20, 0) == 3
        for bad, word in (([(1, 0, 2), (0, 0, 2)], "ordered"), ([(0, 3, 5), (0, 0, 2)], "ordered"), ([(0, 0, 4), (0, 3, 6)], "overlap"),
                          ([(0, 0, 9)], "past"), ([(2, 1, 3)], "past"), ([(1, 2, 2)], "empty"), ([(1, 3, 2)], "empty"), ([(3, 0, 1)], "names read"),
                          ([(0, 0, 1 << 63)], "past")):
            for writer in (plain, zipped):
                for bins in (b"AAA", b"BUB"):  # (the pieces are judged whichever bins the reads go to)
                    with pytest.raises(ValueError, match=word):
                        writer.write_pieces(batch, pr.as_array(bad), bins, True)
        assert _lib.lib.tbk_bin_writer_write_pieces(plain._h, batch._h, None, 1, b"AAA", 0) == _lib.TBK_ERR_INVALID
        assert _lib.lib.tbk_bin_writer_write_pieces(plain._h, batch._h, None, 0, None, 0) == _lib.TBK_ERR_INVALID
        assert _lib.lib.tbk_bin_writer_write_pieces(None, batch._h, None, 0, b"AAA", 0) == _lib.TBK_ERR_INVALID
        for writer, word in ((bam, "BAM bins"), (tagged, "haplotag")):
            with pytest.raises(RuntimeError, match=word) as ei:
                writer.write_pieces(batch, pr.as_array([(0, 0, 2)]), b"AAA", True)
            assert ei.value.code == _lib.TBK_ERR_STATE
        with pytest.raises(ValueError, match="24-byte"):
            plain.write_pieces(batch, np.zeros(3, dtype=np.uint64), b"AAA")
    with seq.BatchReader(str(src), packing=True, borrowing=True) as reader:
        borrowed = seq.Batch()
        assert reader.next_batch(borrowed, 1 << 20, 0) == 3 and borrowed.borrowed
        with pytest.raises(RuntimeError, match="borrowed") as ei:
            plain.write_pieces(borrowed, pr.as_array([(0, 0, 2)]), b"AAA", True)
        assert ei.value.code == _lib.TBK_ERR_STATE
        borrowed.close()
    # nothing was written; and the writers are usable still
    plain.write_pieces(batch, pr.as_array([(0, 0, 2), (0, 4, 8)]), b"ABU", True)
    for writer in (plain, zipped, bam, tagged):
        writer.close()
    batch.close()
    assert tuple(_read(name, False) for name in plain.names) == ("@r0:1-2\nAC\n+\nII\n@r0:5-8\nACGT\n+\nJJJJ\n", "@r1\nACGTAC\n+\nIIIIII\n", "@r2\nTT\n+\n!!\n")
    assert tuple(_read(name, True) for name in zipped.names) == ("", "", "")


# ---- the symbols and the documents ---------------------------------------------------------------------------------------------------
def test_the_symbols_and_their_header(built):
    import ctypes as C

    from trio_binning_amd import _lib

    assert _lib.HAS_DB_PIECES and hasattr(_lib.lib, "tbk_kmerdb_query_pieces") and hasattr(_lib.lib, "tbk_bin_writer_write_pieces")
    ptr, count = C.c_void_p(77), C.c_uint64(77)
    # a NULL session, before any device; nothing is written
    assert _lib.lib.tbk_kmerdb_query_pieces(None, None, None, 0, 1, 255, 0, 0, 1, None, C.byref(ptr), C.byref(count)) == _lib.TBK_ERR_INVALID
    assert (ptr.value, count.value) == (77, 77)
    assert _lib.lib.tbk_kmerdb_query_pieces.argtypes[8] is C.c_uint64 and len(_lib.lib.tbk_kmerdb_query_pieces.argtypes) == 12
    assert len(_lib.lib.tbk_bin_writer_write_pieces.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    for word in ("tbk_kmerdb_query_pieces(", "typedef struct tbk_read_piece { uint64_t read, first, end; } tbk_read_piece;", "read pieces",
                 "enum { TBK_PIECES_COVERED = 0, TBK_PIECES_UNCOVERED = 1 };", "enum { TBK_PIECES_ALL = 0, TBK_PIECES_LONGEST = 1 };",
                 "tbk_bin_writer_write_pieces(", "#define TBK_ABI_VERSION 1"):
        assert word in header, word
    assert header.index("read depth:") < header.index("read pieces:")
    for document, word in (("README.md", "trim_reads"), ("DESIGN.md", "trim_reads"), ("INTEGRATION.md", "tbk_kmerdb_query_pieces"),
                           ("INTEGRATION.md", "tbk_bin_writer_write_pieces"), (os.path.join("tools", "README.md"), "measure_pieces.py")):
        assert word in open(os.path.join(ROOT, document)).read(), document
