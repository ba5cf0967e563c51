"""python -m trio_binning_amd.read_depth, run as a child process, on a small library - reads of a genome most of which the library
saw 30 times, with a stretch it saw 90 times and an "organelle" whose counters stopped at 255, reads of sequence it never saw, reads
with a part of each, reads without a clean window - as FASTQ (plain and .gz) and BAM (tests/bam_craft.py): stdout, the --table and
the --spectrum file byte for byte with what tests/read_depth_ref.py formats from its own records, the three bins' records equal to
the expected reads in input order, BAM bins that hold the records whole, and a thinning that is the same reads in every run, for
every batch size, and the reference's for every seed."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bam_bins_craft as bb
import bam_craft as bc
import db_query_ref as ref
import kmerdb_files as kf
import read_depth_ref as rd
from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

K = 21
STEMS = ("kept", "dropped", "unjudged")
RULES = {  # name: (command line, the reference's arguments)
    "defaults": ([], {}),
    "band": (["--min-depth", "1", "--max-depth", "254"], {"min_depth": 1, "max_depth": 254}),
    "thin": (["--target", "20"], {"target": 20}),
    "thin_seeded": (["--target", "20", "--seed", "5", "--by", "q3", "--min-depth", "1"], {"target": 20, "seed": 5, "by": "q3", "min_depth": 1}),
    "copies": (["--by", "present-median", "--min-count", "31", "--max-depth", "100"], {"by": "present-median", "max_depth": 100}),
}


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _quality(rng, n):
    return "".join(chr(33 + rng.randrange(2, 60)) for _ in range(n))


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("read_depth")
    rng = np.random.default_rng(2028)
    genome, foreign = _seq(rng, 4000), _seq(rng, 1500)
    db = {}
    for lo, hi, counter in ((0, 2000, 30), (2000, 2500, 90), (2500, 3000, 255), (3000, 4000 - K + 1, 30)):
        for w in range(lo, hi):
            db.setdefault(ref.canonical(genome[w:w + K]), counter if w % 9 else max(counter - 3, 2))  # (a library's counters scatter a little)
    erred = list(genome[1200:1500])
    for p in range(10, 300, 15):  # a noisy read: an error every 15 bases leaves no window of 21 whole
        erred[p] = "ACGT"[("ACGT".index(erred[p]) + 1) % 4]
    erred[100:160] = genome[1300:1360]  # but for one clean stretch: the windows 86 .. 139 are at the library's depth
    reads = [("lib1", genome[100:400]), ("alien1", foreign[0:300]), ("organelle1", genome[2550:2950]), ("tiny", "ACGT"), ("repeat1", genome[2050:2450]),
             ("soft", genome[500:700].lower()), ("gaps", ("ACGTACGTAC" + "N") * 5), ("turned", ref.revcomp(genome[300:600])), ("noisy", "".join(erred)),
             ("lib2", genome[3100:3500]), ("edge", genome[1900:2100]), ("organelle2", ref.revcomp(genome[2600:2900])), ("exactly_k", genome[40:40 + K]),
             ("lib3", genome[700:1100]), ("half_alien", genome[1500:1600] + foreign[400:560]), ("repeat2", genome[2100:2400]), ("lib4", genome[3400:3800]),
             ("organelle3", genome[2500:3000]), ("lib5", genome[1000:1250]), ("alien2", foreign[700:900]), ("lib6", genome[0:350]), ("lib7", genome[3600:3990]),
             ("repeat3", genome[2000:2500]), ("lib8", genome[1600:1950])]
    path = root / "library.tbkdb"
    path.write_bytes(ref.database_bytes(db, K))
    return {"root": root, "db": db, "db_path": str(path), "reads": reads}


def _expected(world, reads, rule, min_count=1):
    names, sequences = [n for n, _ in reads], [s for _, s in reads]
    recs = rd.read_depth(world["db"], sequences, K, min_count)
    bins = rd.bins_of(recs, **rule)
    whole = dict({"by": "median", "min_depth": 0, "max_depth": 255, "target": None, "seed": 0}, **rule)
    return {"recs": recs, "bins": bins, "table": rd.table(names, sequences, recs, bins), "spectrum": rd.spectrum(sequences, recs, bins, whole["by"]),
            "summary": rd.summary(sequences, bins, rd.threshold(min_count), **whole)}


def _run(argv, out_dir, env=None, fails=False):
    """the module as a child process; (stdout, table, spectrum, the names of the bins)"""
    out_dir.mkdir()
    table, spectrum = out_dir / "table.tsv", out_dir / "depth.tsv"
    child = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    p = subprocess.run([sys.executable, "-m", "trio_binning_amd.read_depth"] + argv + ["--table", str(table), "--spectrum", str(spectrum)] +
                       [option for stem in STEMS for option in ("--{}-out-prefix".format(stem), str(out_dir / stem))],
                       cwd=str(out_dir), env=child, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert not os.path.exists(str(table) + ".tmp") and not os.path.exists(str(spectrum) + ".tmp")
    if fails:
        assert p.returncode != 0 and p.stdout == "" and not table.exists() and not spectrum.exists()
        return p.stderr
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout, table.read_text(), spectrum.read_text(), sorted(q.name for q in out_dir.iterdir() if not q.name.endswith(".tsv"))


def _text(reads, quals):
    """the records as Read.print writes them"""
    if quals is None:
        return "".join(">{}\n{}\n".format(n, s) for n, s in reads)
    return "".join("@{}\n{}\n+\n{}\n".format(n, s, q) for (n, s), q in zip(reads, quals))


def _bin_texts(out_dir, ext, gz):
    texts = []
    for stem in STEMS:
        with (gzip.open if gz else open)(out_dir / (stem + ext + (".gz" if gz else "")), "rb") as fh:
            texts.append(fh.read().decode())
    return texts


def _check_text_bins(out_dir, ext, gz, reads, quals, bins):
    for code, stem, got in zip("ABU", STEMS, _bin_texts(out_dir, ext, gz)):
        mine = [i for i, b in enumerate(bins) if b == code]
        assert got == _text([reads[i] for i in mine], None if quals is None else [quals[i] for i in mine]), (stem, ext)
        assert mine, "no read in " + stem  # the library fills all three bins


def _fastq(world, tmp_path, form="fastq"):
    rng = random.Random(5)
    quals = [_quality(rng, len(s)) for _, s in world["reads"]]
    path = tmp_path / ("reads." + form)
    with (gzip.open if form.endswith(".gz") else open)(path, "wb") as fh:
        fh.write(_text(world["reads"], quals).encode())
    return path, quals


def test_the_rules_send_reads_to_all_three_bins(world):
    """on the reference's answer alone: what each read is there for"""
    reads = world["reads"]
    by_name = lambda bins: {n: b for (n, _), b in zip(reads, bins)}  # noqa: E731
    plain = _expected(world, reads, {})
    recs = dict(zip((n for n, _ in reads), plain["recs"]))
    assert set(by_name(plain["bins"]).values()) == {"A", "U"} and by_name(plain["bins"])["tiny"] == by_name(plain["bins"])["gaps"] == "U"
    assert recs["lib1"][6] == 30 and recs["organelle1"][6] == 255 and recs["organelle1"][2] > 300 and recs["repeat1"][6] == 90 and recs["alien1"][1] == 0
    assert recs["noisy"][0] == 280 and recs["noisy"][6] == 0 and recs["noisy"][9] == 30  # median 0, present_median the library's depth
    assert recs["half_alien"][6] == 0 and recs["half_alien"][9] == 30 and recs["edge"][4] < recs["edge"][8] and recs["exactly_k"][0] == 1
    band = by_name(_expected(world, reads, RULES["band"][1])["bins"])
    assert band["lib1"] == band["repeat1"] == band["soft"] == band["turned"] == "A" and band["organelle1"] == band["alien1"] == band["noisy"] == "B"
    copies = by_name(_expected(world, reads, RULES["copies"][1], 31)["bins"])
    assert copies["organelle2"] == "B" and copies["repeat2"] == "A" and copies["lib3"] == "A"  # min_count 31: the library's depth reads as 0, and 0 is kept
    for name in ("thin", "thin_seeded"):
        thin = _expected(world, reads, RULES[name][1])["bins"]
        assert set(thin) == {"A", "B", "U"}
        deep = [b for b, rec in zip(thin, plain["recs"]) if rec[0] and rec[rd.STATISTICS[RULES[name][1].get("by", "median")]] > 20]
        assert "A" in deep and "B" in deep  # some of the reads above the target stay
    assert _expected(world, reads, {"target": 20})["bins"] != _expected(world, reads, {"target": 20, "seed": 5})["bins"]


@pytest.mark.parametrize("form, rule", [("fastq", "band"), ("fastq.gz", "thin_seeded"), ("fastq.gz", "copies")])
def test_text_input(world, tmp_path, form, rule):
    reads = world["reads"]
    path, quals = _fastq(world, tmp_path, form)
    options, kwargs = RULES[rule]
    want = _expected(world, reads, kwargs, 31 if rule == "copies" else 1)
    gz = form.endswith(".gz")  # (gzip'ed bins from gzip'ed reads, plain ones from plain reads)
    out, table, spectrum, names = _run([str(path), world["db_path"]] + options + ([] if gz else ["--no-gzip-output"]), tmp_path / "out")
    assert out == want["summary"] and table == want["table"] and spectrum == want["spectrum"]
    assert names == sorted(stem + ".fastq" + (".gz" if gz else "") for stem in STEMS)
    if rule == "copies":
        assert out.endswith("#rule\t31\tpresent-median\t0\t100\t-\t0\n")
        assert "B" in want["bins"] and "U" in want["bins"]
    _check_text_bins(tmp_path / "out", ".fastq", gz, reads, quals, want["bins"])


def test_thinning_is_the_same_in_every_run_and_for_every_batch_size(world, tmp_path):
    reads = world["reads"]
    path, quals = _fastq(world, tmp_path)
    options, kwargs = RULES["thin"]
    want = _expected(world, reads, kwargs)
    runs = [_run([str(path), world["db_path"], "--no-gzip-output"] + options, tmp_path / name, env)
            for name, env in (("once", None), ("twice", None), ("batches", {"TBK_BATCH_READS": "3"}))]
    for out, table, spectrum, _ in runs:
        assert out == want["summary"] and table == want["table"] and spectrum == want["spectrum"]
    assert out.endswith("#rule\t2\tmedian\t0\t255\t20\t0\n")
    texts = [_bin_texts(tmp_path / name, ".fastq", False) for name in ("once", "twice", "batches")]
    assert texts[0] == texts[1] == texts[2]
    _check_text_bins(tmp_path / "once", ".fastq", False, reads, quals, want["bins"])


def test_bam_input_and_bam_output(world, tmp_path):
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
    options, kwargs = RULES["thin"]
    want = _expected(world, reads, kwargs)
    # FASTQ bins from BAM input
    out, table, spectrum, names = _run([str(path), world["db_path"]] + options, tmp_path / "text")
    assert out == want["summary"] and table == want["table"] and spectrum == want["spectrum"] and names == sorted(stem + ".fastq.gz" for stem in STEMS)
    for code, stem in zip("ABU", STEMS):
        with gzip.open(tmp_path / "text" / (stem + ".fastq.gz"), "rb") as fh:
            assert fh.read() == bc.fastq_of([r for r, b in zip(kept, want["bins"]) if b == code]), stem
    # BAM bins: every record whole behind the input's header
    out, table, spectrum, names = _run([str(path), world["db_path"], "--bam-output"] + options, tmp_path / "bam")
    assert out == want["summary"] and table == want["table"] and spectrum == want["spectrum"] and names == sorted(stem + ".bam" for stem in STEMS)
    for code, stem in zip("ABU", STEMS):
        header, records, data = bb.read_bam_file(str(tmp_path / "bam" / (stem + ".bam")))
        mine = [r for r, b in zip(kept, want["bins"]) if b == code]
        assert header == bc.header(text=text) and records == [bc.encode(r) for r in mine] and mine, stem
        assert bc.parse(data) == bc.fastq_of(mine)


def test_a_compressed_database_and_a_list_are_refused(world, tmp_path):
    path, _ = _fastq(world, tmp_path)
    _, keys, counts, hist = kf.sound(k=21, n=5, seed=1)
    hpc = tmp_path / "hpc.tbkdb"
    hpc.write_bytes(kf.file_bytes(21, keys, counts, hist, reads=11, bases=1234, magic=b"TBKKMDH1"))
    err = _run([str(path), str(hpc)], tmp_path / "hpc", fails=True)
    assert "read_depth: " in err and "homopolymer-compressed k-mers" in err and "out of scope here" in err
    err = _run([str(path), os.path.join(DATA, "hapA.txt")], tmp_path / "list", fails=True)
    assert "read_depth: " in err and "is not a count database (*.tbkdb)" in err
    assert not [q.name for name in ("hpc", "list") for q in (tmp_path / name).iterdir()]  # no bin was opened


def test_a_failing_run_leaves_no_tmp_file(world, tmp_path, monkeypatch):
    from trio_binning_amd import kmers, read_depth

    def broken(self, *args, **kwargs):
        raise RuntimeError("made to fail")

    path = tmp_path / "reads.fa"
    path.write_text(_text(world["reads"], None))
    table, spectrum = tmp_path / "fails.tsv", tmp_path / "fails_depth.tsv"
    monkeypatch.setattr(kmers.DatabaseQuery, "read_depth", broken)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(RuntimeError, match="made to fail"):
        read_depth.main([str(path), world["db_path"], "--table", str(table), "--spectrum", str(spectrum)])
    for side in (table, spectrum):
        assert not side.exists() and not os.path.exists(str(side) + ".tmp")
