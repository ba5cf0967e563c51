"""python -m trio_binning_amd.trim_reads on a small library - reads of a "cloud" whose k-mers the database holds, reads of the rest of
the genome, chimeras of both, a read with one stray hit, reads without a clean window - as FASTQ (plain and .gz), FASTA and BAM
(tests/bam_craft.py): the three bins after gunzip, the --table file, the --bed file and stdout byte for byte with what
tests/pieces_ref.py makes of its own pieces, for both sides, both selections and a --min-length that leaves pieces out."""
import gzip
import os
import random
from unittest.mock import patch

import numpy as np
import pytest

import bam_bins_craft as bb
import bam_craft as bc
import db_query_ref as ref
import pieces_ref as pr
import screen_ref as sr

pytestmark = pytest.mark.gpu

K = 21
COUNTER = 12
RULES = {  # name: (command line, the reference's arguments)
    "defaults": ([], {}),
    "covered_all": (["--pieces", "all", "--min-length", "40"], {"which": "all", "min_length": 40}),
    "uncovered_all": (["--keep", "uncovered", "--pieces", "all", "--min-length", "2"], {"keep": "uncovered", "which": "all", "min_length": 2}),
    "uncovered_longest": (["--keep", "uncovered", "--min-length", "150"], {"keep": "uncovered", "min_length": 150}),
}
STEMS = ("kept", "dropped", "unjudged")


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _quality(rng, n):
    return "".join(chr(33 + rng.randrange(2, 60)) for _ in range(n))


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("trim_reads")
    rng = np.random.default_rng(2029)
    genome = _seq(rng, 3000)
    cloud = genome[:1000]
    db = {km: COUNTER for km in ref.window_kmers(cloud, K)}
    reads = [("cloud1 a comment", genome[100:400]), ("rest1", genome[2000:2300]), ("edge", genome[900:1100]), ("tiny", "ACGT"),
             ("stray", genome[2400:2500] + genome[10:10 + K] + genome[2600:2700]), ("soft", genome[500:700].lower()),
             ("gaps", ("ACGTACGTAC" + "N") * 5), ("turned", ref.revcomp(genome[300:600])), ("rest2", genome[1500:1900]),
             ("chimera", genome[0:200] + genome[1200:1400] + genome[600:650]), ("error", genome[40:140] + "ACGT"["TGCA".index(genome[140])] + genome[141:400]),
             ("exactly_k", genome[40:40 + K]), ("masked", genome[200:300] + "N" + genome[301:330] + "NN" + genome[332:500]), ("cloud2", genome[0:1000])]
    path = root / "cloud.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "db": db, "db_path": str(path), "reads": reads, "genome": genome}


def _expected(world, records, rule, min_count=1, max_count=255):
    """(bins' text, table, bed, summary, bins, pieces) of `records` - (header, sequence, quality)"""
    rule = dict({"keep": "covered", "which": "longest", "min_length": 1}, **rule)
    found, evidence, bins = pr.trim(world["db"], records, K, min_count, max_count, **rule)
    text = pr.bins_text(records, found, bins, rule["which"] == "all")
    summary = pr.summary(records, found, bins, sr.threshold(min_count), max_count, rule["keep"], rule["which"], rule["min_length"])
    return text, pr.table(records, found, evidence, bins), pr.bed(records, found), summary, bins, found


def _run(argv, out_dir, capsys):
    from trio_binning_amd import trim_reads

    out_dir.mkdir()
    table, bed = out_dir / "table.tsv", out_dir / "pieces.bed"
    capsys.readouterr()
    trim_reads.main(argv + ["--table", str(table), "--bed", str(bed)] + [x for stem in STEMS for x in ("--{}-out-prefix".format(stem), str(out_dir / stem))])
    assert not os.path.exists(str(table) + ".tmp") and not os.path.exists(str(bed) + ".tmp")
    return capsys.readouterr().out, table.read_text(), bed.read_text(), sorted(p.name for p in out_dir.iterdir() if p.name not in ("table.tsv", "pieces.bed"))


def _source(records):
    return "".join("@{}\n{}\n+\n{}\n".format(h, s, q) if q else ">{}\n{}\n".format(h, s) for h, s, q in records)


def _bins(out_dir, ext, gz):
    got = []
    for stem in STEMS:
        with (gzip.open if gz else open)(out_dir / (stem + ext + (".gz" if gz else "")), "rb") as fh:
            got.append(fh.read().decode())
    return tuple(got)


def _records(world, form):
    rng = random.Random(5)
    return [(h, s, "" if form == "fa" else _quality(rng, len(s))) for h, s in world["reads"]]


def test_the_rules_fill_every_bin_and_cut_bases(world):
    """on the reference's answer alone: what each read is there for"""
    records = _records(world, "fa")
    names = [h.split(" ")[0] for h, _, _ in records]
    _, _, _, summary, bins, found = _expected(world, records, {})
    by_name = dict(zip(names, bins))
    assert by_name == {"cloud1": "A", "rest1": "B", "edge": "A", "tiny": "U", "stray": "A", "soft": "A", "gaps": "U", "turned": "A", "rest2": "B",
                       "chimera": "A", "error": "A", "exactly_k": "A", "masked": "A", "cloud2": "A"}
    mine = {names[r]: (f, e) for r, f, e in found}
    assert mine["cloud1"] == (0, 300) and mine["edge"] == (0, 100) and mine["stray"] == (100, 100 + K) and mine["chimera"] == (0, 200)
    assert mine["error"] == (101, 360) and mine["masked"] == (132, 300) and mine["exactly_k"] == (0, K) and mine["soft"] == (0, 200)
    cut = int(summary.split("\n")[3].split("\t")[1])
    assert summary.split("\n")[3].startswith("#cut\t") and cut == 100 + 200 + 250 + 101 + 132 > 0
    assert all(code in bins for code in "ABU")  # kept, dropped and unjudged are all filled
    _, _, _, _, bins, found = _expected(world, records, RULES["covered_all"][1])
    assert [(f, e) for r, f, e in found if names[r] == "chimera"] == [(0, 200), (400, 450)] and dict(zip(names, bins))["stray"] == "B"  # (21 < 40)
    assert [(f, e) for r, f, e in found if names[r] == "masked"] == [(0, 100), (132, 300)]  # [101, 130) is 29 bases
    _, _, _, _, bins, found = _expected(world, records, RULES["uncovered_all"][1])
    by_name = dict(zip(names, bins))
    assert by_name["cloud1"] == "B" and by_name["rest1"] == "A" and by_name["tiny"] == "U" and by_name["gaps"] == "U" and by_name["error"] == "B"  # (one base < 2)
    assert [(f, e) for r, f, e in found if names[r] == "chimera"] == [(200, 400)] and [(f, e) for r, f, e in found if names[r] == "masked"] == [(130, 132)]
    assert [(f, e) for r, f, e in found if names[r] == "stray"] == [(0, 100), (100 + K, 200 + K)]
    _, _, _, _, bins, found = _expected(world, records, RULES["uncovered_longest"][1])
    assert dict(zip(names, bins))["stray"] == "B" and [names[r] for r, _, _ in found] == ["rest1", "rest2", "chimera"]


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("form", ("fastq", "fastq.gz", "fa"))
def test_text_input(world, capsys, tmp_path, form, rule):
    records = _records(world, form)
    path = tmp_path / ("reads." + form)
    with (gzip.open if form.endswith(".gz") else open)(path, "wb") as fh:
        fh.write(_source(records).encode())
    options, kwargs = RULES[rule]
    text, table, bed, summary, _, _ = _expected(world, records, kwargs)
    ext = "." + form.split(".")[0]
    for gz in (True, False):
        out_dir = tmp_path / ("gz" if gz else "plain")
        out, got_table, got_bed, names = _run([str(path), world["db_path"]] + options + ([] if gz else ["--no-gzip-output"]), out_dir, capsys)
        assert out == summary and got_table == table and got_bed == bed
        assert names == sorted(stem + ext + (".gz" if gz else "") for stem in STEMS)
        assert _bins(out_dir, ext, gz) == text


def test_a_counter_range_and_several_batches(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import trim_reads

    records = _records(world, "fastq")
    path = tmp_path / "reads.fastq"
    path.write_text(_source(records))
    whole = {}
    for rule in ("covered_all", "uncovered_all"):
        whole[rule] = _run([str(path), world["db_path"]] + RULES[rule][0], tmp_path / ("whole_" + rule), capsys) + (_bins(tmp_path / ("whole_" + rule), ".fastq", True),)
    monkeypatch.setattr(trim_reads, "_BATCH_BASES", 700)  # several batches: the tallies and the tables run on, the pieces' reads count from the batch's first
    monkeypatch.setattr(trim_reads, "_BATCH_READS", 3)
    for rule in ("covered_all", "uncovered_all"):
        text, table, bed, summary, _, _ = _expected(world, records, RULES[rule][1])
        got = _run([str(path), world["db_path"]] + RULES[rule][0], tmp_path / ("batches_" + rule), capsys)
        assert got[:3] == (summary, table, bed) == whole[rule][:3]
        assert _bins(tmp_path / ("batches_" + rule), ".fastq", True) == text == whole[rule][4]
    for lo, hi in ((13, 255), (1, 11)):  # the database's one counter is 12: nothing is covered, every judged read is dropped - or kept whole
        text, table, bed, summary, bins, _ = _expected(world, records, {}, lo, hi)
        assert set(bins) == {"B", "U"} and summary.endswith("#cut\t0\n#rule\t{}\t{}\tcovered\tlongest\t1\n".format(max(lo, 2), hi)) and bed == ""
        out, got_table, got_bed, _ = _run([str(path), world["db_path"], "--min-count", str(lo), "--max-count", str(hi)], tmp_path / "range{}".format(lo), capsys)
        assert (out, got_table, got_bed) == (summary, table, bed) and _bins(tmp_path / "range{}".format(lo), ".fastq", True) == text
    text, table, bed, summary, bins, _ = _expected(world, records, {"keep": "uncovered"}, 13, 255)
    assert set(bins) == {"A", "U"} and text[0] == _source([(h.split(" ")[0], s, q) for (h, s, q), b in zip(records, bins) if b == "A"])
    out, got_table, got_bed, _ = _run([str(path), world["db_path"], "--keep", "uncovered", "--min-count", "13"], tmp_path / "kept_whole", capsys)
    assert (out, got_table, got_bed) == (summary, table, bed) and _bins(tmp_path / "kept_whole", ".fastq", True) == text


def test_the_environment_sets_the_batch_size(world, tmp_path):
    """TBK_BATCH_READS=3 in a process of its own gives the same files"""
    import subprocess
    import sys

    from conftest import ROOT

    records = _records(world, "fastq")
    path = tmp_path / "reads.fastq"
    path.write_text(_source(records))
    text, table, bed, summary, _, _ = _expected(world, records, RULES["covered_all"][1])
    argv = [sys.executable, "-m", "trio_binning_amd.trim_reads", str(path), world["db_path"], "--table", "table.tsv", "--bed", "pieces.bed"] + RULES["covered_all"][0]
    done = subprocess.run(argv, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT, TBK_BATCH_READS="3"), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout == summary and (tmp_path / "table.tsv").read_text() == table and (tmp_path / "pieces.bed").read_text() == bed
    assert _bins(tmp_path, ".fastq", True) == text


def test_bam_input(world, capsys, tmp_path):
    rng = random.Random(7)
    recs = []
    for i, (header, s) in enumerate(world["reads"]):
        name = header.split(" ")[0]
        qual = None if i % 5 == 3 else [rng.randrange(3, 90) for _ in s]
        recs.append(bc.record(name, s.upper(), qual, flag=4, tags=bb.tag_block(rng, kinetics=len(s) if i % 4 == 0 else 0) if i % 3 else b""))
        if i % 4 == 1:
            recs.append(bc.record(name + "/sup", s.upper()[:50], None, flag=0x804, tags=bb.tag_block(rng)))  # skipped by the reader
    path = tmp_path / "reads.hifi_reads.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(recs, text=b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:0a1b2c3d\tPL:PACBIO\n"), block=3000, level=1))
    records = []
    for r in bb.kept(recs):  # the records as FASTQ text, as they come out without --bam-output elsewhere
        lines = bc.text_of(r).decode().split("\n")
        records.append((lines[0][1:], lines[1], lines[3] if lines[0][0] == "@" else ""))
    assert [h for h, _, _ in records] == [h.split(" ")[0] for h, _ in world["reads"]] and any(not q for _, _, q in records)
    for rule in ("defaults", "covered_all", "uncovered_all"):
        text, table, bed, summary, _, _ = _expected(world, records, RULES[rule][1])
        out, got_table, got_bed, names = _run([str(path), world["db_path"]] + RULES[rule][0], tmp_path / rule, capsys)
        assert (out, got_table, got_bed) == (summary, table, bed) and names == ["dropped.fastq.gz", "kept.fastq.gz", "unjudged.fastq.gz"]
        assert _bins(tmp_path / rule, ".fastq", True) == text
    with pytest.raises(SystemExit):
        _run([str(path), world["db_path"], "--bam-output"], tmp_path / "refused", capsys)


def test_reads_the_database_holds_whole_are_the_records_classify_by_kmers_writes(world, capsys, tmp_path):
    """every k-mer of the reads is in the database: kept is every record untouched - the bytes classify-by-kmers writes for the same
    input into the bin of the parent that has these k-mers, with either selection (a whole record keeps its name)"""
    from trio_binning_amd.classify_by_kmers import main as classify

    genome = world["genome"]
    rng = random.Random(11)
    records = [("whole{} comment {}".format(i, i), genome[a:a + n], _quality(rng, n)) for i, (a, n) in enumerate(((0, 300), (50, 2 * K), (600, 400), (90, 250), (10, 990)))]
    path = tmp_path / "reads.fastq"
    path.write_text(_source(records))
    lists = tmp_path / "hapA.txt", tmp_path / "hapB.txt"
    lists[0].write_text("".join(km + "\n" for km in sorted(world["db"])))
    lists[1].write_text(ref.canonical(genome[2000:2000 + K]) + "\n")
    with patch("sys.argv", ["classify-by-kmers", str(path), str(lists[0]), str(lists[1])] +
               [x for hap, stem in (("haplotype-a", "hapA"), ("haplotype-b", "hapB"), ("unclassified", "unclassified")) for x in ("--{}-out-prefix".format(hap), str(tmp_path / stem))]):
        classify()
    with gzip.open(tmp_path / "hapA.fastq.gz", "rb") as fh:
        classified = fh.read().decode()
    assert classified == _source([(h.split(" ")[0], s, q) for h, s, q in records])
    for rule in ("defaults", "covered_all"):
        text, table, bed, summary, bins, _ = _expected(world, records, RULES[rule][1])
        assert bins == "AAAAA" and text == (classified, "", "") and summary.split("\n")[3] == "#cut\t0"
        out, got_table, got_bed, _ = _run([str(path), world["db_path"]] + RULES[rule][0], tmp_path / rule, capsys)
        assert (out, got_table, got_bed) == (summary, table, bed) and _bins(tmp_path / rule, ".fastq", True) == text


def test_a_failing_run_leaves_no_tmp_file(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import kmers, trim_reads

    def broken(self, *args, **kwargs):
        raise RuntimeError("made to fail")

    path = tmp_path / "reads.fa"
    path.write_text(_source(_records(world, "fa")))
    table, bed = tmp_path / "fails.tsv", tmp_path / "fails.bed"
    monkeypatch.setattr(kmers.DatabaseQuery, "pieces", broken)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match="made to fail"):
        trim_reads.main([str(path), world["db_path"], "--table", str(table), "--bed", str(bed)])
    for made in (table, bed):
        assert not made.exists() and not os.path.exists(str(made) + ".tmp")
