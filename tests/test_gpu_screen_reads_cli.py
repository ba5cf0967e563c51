"""python -m trio_binning_amd.screen_reads on a small library - reads of a "cloud" whose k-mers the database holds, reads of the rest
of the genome, reads with a part of each, a read with one stray hit, reads without a clean window - as FASTQ (plain and .gz),
FASTA and BAM (tests/bam_craft.py): stdout and the --table file byte for byte with what tests/screen_ref.py formats from its own
records, the three bins' records equal to the expected reads in input order, and BAM bins that hold the records whole."""
import gzip
import os
import random

import numpy as np
import pytest

import bam_bins_craft as bb
import bam_craft as bc
import db_query_ref as ref
import screen_ref as sr

pytestmark = pytest.mark.gpu

K = 21
COUNTER = 12
RULES = {  # name: (command line, the reference's arguments)
    "defaults": ([], {}),
    "half": (["--min-share", "0.5"], {"min_share": "0.5"}),
    "all_four": (["--min-hits", "2", "--min-share", "0.25", "--min-covered", "0.500", "--min-stretch", "60"],
                 {"min_hits": 2, "min_share": "0.25", "min_covered": "0.500", "min_stretch": 60}),
}


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _quality(rng, n):
    return "".join(chr(33 + rng.randrange(2, 60)) for _ in range(n))


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("screen_reads")
    rng = np.random.default_rng(2026)
    genome = _seq(rng, 3000)
    cloud = genome[:1000]
    db = {km: COUNTER for km in ref.window_kmers(cloud, K)}
    reads = [("cloud1", genome[100:400]), ("rest1", genome[2000:2300]), ("edge", genome[900:1100]), ("tiny", "ACGT"),
             ("stray", genome[2400:2500] + genome[10:10 + K] + genome[2600:2700]), ("soft", genome[500:700].lower()),
             ("gaps", ("ACGTACGTAC" + "N") * 5), ("turned", ref.revcomp(genome[300:600])), ("rest2", genome[1500:1900]),
             ("third", genome[950:1250]), ("exactly_k", genome[40:40 + K]), ("cloud2", genome[0:1000])]
    path = root / "cloud.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "db": db, "db_path": str(path), "reads": reads}


def _expected(world, reads, rule, min_count=1, max_count=255):
    names, sequences = [n for n, _ in reads], [s for _, s in reads]
    recs = sr.evidence(world["db"], sequences, K, min_count, max_count)
    bins = "".join(sr.bin_of(rec, len(s), **rule) for rec, s in zip(recs, sequences))
    return recs, bins, sr.table(names, sequences, recs, bins), sr.summary(sequences, bins, sr.threshold(min_count), max_count, **dict(
        {"min_hits": 1, "min_share": "0", "min_covered": "0", "min_stretch": 0}, **rule))


def _run(argv, out_dir, capsys):
    from trio_binning_amd import screen_reads

    out_dir.mkdir()
    table = out_dir / "table.tsv"
    capsys.readouterr()
    screen_reads.main(argv + ["--table", str(table), "--matched-out-prefix", str(out_dir / "matched"), "--unmatched-out-prefix", str(out_dir / "unmatched"),
                              "--unjudged-out-prefix", str(out_dir / "unjudged")])
    assert not os.path.exists(str(table) + ".tmp")
    return capsys.readouterr().out, table.read_text(), sorted(p.name for p in out_dir.iterdir() if p.name != "table.tsv")


def _text(reads, quals):
    """the records as Read.print writes them"""
    if quals is None:
        return "".join(">{}\n{}\n".format(n, s) for n, s in reads)
    return "".join("@{}\n{}\n+\n{}\n".format(n, s, q) for (n, s), q in zip(reads, quals))


def _check_text_bins(out_dir, ext, gz, reads, quals, bins):
    for code, stem in zip("ABU", ("matched", "unmatched", "unjudged")):
        path = out_dir / (stem + ext + (".gz" if gz else ""))
        with (gzip.open if gz else open)(path, "rb") as fh:
            got = fh.read().decode()
        mine = [i for i, b in enumerate(bins) if b == code]
        assert got == _text([reads[i] for i in mine], None if quals is None else [quals[i] for i in mine]), (stem, ext)
        assert mine, "no read in " + stem  # the library fills all three bins


def test_the_rules_send_reads_to_all_three_bins(world):
    """on the reference's answer alone: what each read is there for"""
    reads = world["reads"]
    by_name = lambda bins: {n: b for (n, _), b in zip(reads, bins)}  # noqa: E731
    recs, bins, _, _ = _expected(world, reads, {})
    assert by_name(bins) == {"cloud1": "A", "rest1": "B", "edge": "A", "tiny": "U", "stray": "A", "soft": "A", "gaps": "U", "turned": "A", "rest2": "B",
                             "third": "A", "exactly_k": "A", "cloud2": "A"}
    assert recs[0] == (280, 280, 300, 300, 1) and recs[4] == (201, 1, K, K, 1) and recs[2] == (180, 80, 100, 100, 1) and recs[6] == (0,) * 5
    half = by_name(_expected(world, reads, RULES["half"][1])[1])
    assert half["stray"] == "B" and half["edge"] == "B" and half["cloud1"] == "A" and half["tiny"] == "U"  # 80 of 180 windows, 1 of 201
    four = by_name(_expected(world, reads, RULES["all_four"][1])[1])
    assert four["third"] == "B" and four["edge"] == "A" and four["exactly_k"] == "B" and four["stray"] == "B"  # 30 of 280 windows; one hit; one hit


@pytest.mark.parametrize("rule", sorted(RULES))
@pytest.mark.parametrize("form", ("fastq", "fastq.gz", "fa"))
def test_text_input(world, capsys, tmp_path, form, rule):
    reads = world["reads"]
    rng = random.Random(5)
    quals = None if form == "fa" else [_quality(rng, len(s)) for _, s in reads]
    path = tmp_path / ("reads." + form)
    with (gzip.open if form.endswith(".gz") else open)(path, "wb") as fh:
        fh.write(_text(reads, quals).encode())
    options, kwargs = RULES[rule]
    _, bins, table, summary = _expected(world, reads, kwargs)
    ext = "." + form.split(".")[0]
    for gz in (True, False):
        out, got_table, names = _run([str(path), world["db_path"]] + options + ([] if gz else ["--no-gzip-output"]), tmp_path / ("gz" if gz else "plain"), capsys)
        assert out == summary and got_table == table
        assert names == sorted(stem + ext + (".gz" if gz else "") for stem in ("matched", "unmatched", "unjudged"))
        _check_text_bins(tmp_path / ("gz" if gz else "plain"), ext, gz, reads, quals, bins)


def test_a_counter_range_and_several_batches(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import screen_reads

    reads = world["reads"]
    path = tmp_path / "reads.fa"
    path.write_text(_text(reads, None))
    monkeypatch.setattr(screen_reads, "_BATCH_BASES", 700)  # several batches: the tallies and the table run on
    monkeypatch.setattr(screen_reads, "_BATCH_READS", 3)
    _, bins, table, summary = _expected(world, reads, {})
    out, got_table, _ = _run([str(path), world["db_path"]], tmp_path / "batches", capsys)
    assert out == summary and got_table == table
    _check_text_bins(tmp_path / "batches", ".fa", True, reads, None, bins)
    for lo, hi in ((13, 255), (1, 11)):  # the database's one counter is 12: nothing is held, every judged read is unmatched
        _, bins, table, summary = _expected(world, reads, {}, lo, hi)
        assert set(bins) == {"B", "U"} and summary.endswith("#rule\t{}\t{}\t1\t0\t0\t0\n".format(max(lo, 2), hi))
        out, got_table, _ = _run([str(path), world["db_path"], "--min-count", str(lo), "--max-count", str(hi)], tmp_path / "range{}".format(lo), capsys)
        assert out == summary and got_table == table
    _, bins, table, summary = _expected(world, reads, {}, 12, 12)
    out, got_table, _ = _run([str(path), world["db_path"], "--min-count", "12", "--max-count", "12"], tmp_path / "range12", capsys)
    assert out == summary and got_table == table and "A" in bins


def test_bam_input_and_bam_output(world, capsys, tmp_path):
    rng = random.Random(7)
    recs = []
    for i, (name, s) in enumerate(world["reads"]):
        qual = None if i % 5 == 3 else [rng.randrange(3, 90) for _ in s]
        recs.append(bc.record(name, s.upper(), qual, flag=4, tags=bb.tag_block(rng, kinetics=len(s) if i % 4 == 0 else 0) if i % 3 else b""))
        if i % 4 == 1:
            recs.append(bc.record(name + "/sup", s.upper()[:50], None, flag=0x804, tags=bb.tag_block(rng)))  # skipped by the reader
    text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:0a1b2c3d\tPL:PACBIO\n"
    path = tmp_path / "reads.hifi_reads.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(recs, text=text), block=3000, level=1))
    kept = bb.kept(recs)
    reads = [(r["name"], r["seq"]) for r in kept]
    assert [n for n, _ in reads] == [n for n, _ in world["reads"]]
    _, bins, table, summary = _expected(world, reads, RULES["half"][1])
    # FASTQ bins from BAM input
    out, got_table, names = _run([str(path), world["db_path"]] + RULES["half"][0], tmp_path / "text", capsys)
    assert out == summary and got_table == table and names == ["matched.fastq.gz", "unjudged.fastq.gz", "unmatched.fastq.gz"]
    for code, stem in zip("ABU", ("matched", "unmatched", "unjudged")):
        with gzip.open(tmp_path / "text" / (stem + ".fastq.gz"), "rb") as fh:
            assert fh.read() == bc.fastq_of([r for r, b in zip(kept, bins) if b == code]), stem
    # BAM bins: every record whole behind the input's header
    out, got_table, names = _run([str(path), world["db_path"], "--bam-output"] + RULES["half"][0], tmp_path / "bam", capsys)
    assert out == summary and got_table == table and names == ["matched.bam", "unjudged.bam", "unmatched.bam"]
    for code, stem in zip("ABU", ("matched", "unmatched", "unjudged")):
        header, records, data = bb.read_bam_file(str(tmp_path / "bam" / (stem + ".bam")))
        want = [r for r, b in zip(kept, bins) if b == code]
        assert header == bc.header(text=text) and records == [bc.encode(r) for r in want] and want, stem
        assert bc.parse(data) == bc.fastq_of(want)


def test_a_failing_run_leaves_no_tmp_file(world, capsys, tmp_path, monkeypatch):
    from trio_binning_amd import kmers, screen_reads

    def broken(self, *args, **kwargs):
        raise RuntimeError("made to fail")

    path = tmp_path / "reads.fa"
    path.write_text(_text(world["reads"], None))
    table = tmp_path / "fails.tsv"
    monkeypatch.setattr(kmers.DatabaseQuery, "evidence", broken)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match="made to fail"):
        screen_reads.main([str(path), world["db_path"], "--table", str(table)])
    assert not table.exists() and not os.path.exists(str(table) + ".tmp")
