"""BAM input on the device: the transcode kernels by themselves (tbk_bam_fastq_device) against tests/bam_craft.py byte for
byte at the smallest shapes where they can go wrong, then the reader and the command lines on a .bam over many small
windows against the same reads as FASTQ."""
import gzip
import random
from unittest.mock import patch

import pytest

import bam_craft as bc

pytestmark = pytest.mark.gpu

TAGS = b"rqf\x00\x00\x80\x3fnpi\x07\x00\x00\x00"


def _device(gpu, recs, skip=bc.SKIP_DEFAULT, each=False):
    """the device's text of the records must be the rule's, and the host transcoder's; `each`: every record by itself too, which
    pins every measured length"""
    from trio_binning_amd import seq

    data, offsets = bc.records_bytes(recs)
    lengths = bc.lengths_of(recs, skip)
    want = bc.fastq_of(recs, skip)
    counts = (sum(1 for l in lengths if l), sum(1 for l in lengths if not l))
    text, written, skipped = seq.bam_fastq_device(data, offsets, skip)
    assert len(text) == sum(lengths) and (written, skipped) == counts
    if text != want:
        at = next(i for i in range(len(want)) if text[i] != want[i])
        raise AssertionError("first difference at byte {} (tile {}, lane {}): {!r} for {!r}".format(at, at // 4096, at % 4096 // 16, text[at - 8:at + 24], want[at - 8:at + 24]))
    assert seq.bam_fastq_host(data, offsets, skip) == (want, *counts)
    if each:
        for i, r in enumerate(recs):
            one = bc.encode(r)
            assert seq.bam_fastq_device(one, [0], skip) == (bc.text_of(r, skip), int(lengths[i] > 0), int(lengths[i] == 0)), i
    return text


def _seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _qual(rng, n):
    return [rng.randrange(0, 94) for _ in range(n)]


def test_lengths_around_a_lanes_vector(gpu):
    """l_seq around 16 and 32 output bytes, both strands, with and without quality, after names that move every boundary"""
    rng = random.Random(1)
    recs = []
    for length in (1, 2, 3, 15, 16, 17, 31, 32, 33) * 4:   # (four times, under other names: more than one tile of text)
        for flag in (4, 0x14):
            for with_qual in (True, False):
                name = "n" * rng.randrange(1, 19)
                recs.append(bc.record(name, _seq(rng, length, bc.LETTERS), _qual(rng, length) if with_qual else None, flag=flag))
    assert len(bc.fastq_of(recs)) > 4096
    _device(gpu, recs, each=True)


@pytest.mark.parametrize("end", [4095, 4096, 4097])
def test_text_that_ends_beside_a_tile_edge(gpu, end):
    rng = random.Random(end)
    name = "n" * (end - 4094)                    # len = name + 2 * 2044 + 6
    first = bc.record(name, _seq(rng, 2044), _qual(rng, 2044))
    assert len(bc.text_of(first)) == end
    _device(gpu, [first])
    _device(gpu, [dict(first, flag=0x14)])
    _device(gpu, [first, bc.record("b", "ACG", [1, 2, 3])])
    fasta = bc.record("n" * (end - 4092), _seq(rng, 4089), None)   # len = name + 4089 + 3
    assert len(bc.text_of(fasta)) == end
    _device(gpu, [fasta, first, fasta])


def test_a_record_over_three_tiles_and_long_reads(gpu):
    rng = random.Random(3)
    recs = [bc.record("lead", _seq(rng, 1000), _qual(rng, 1000))]
    for length, flag in ((5000, 4), (5001, 0x14), (10000, 0x10), (10001, 0)):
        recs.append(bc.record("long%d" % length, _seq(rng, length, bc.LETTERS), _qual(rng, length), flag=flag, n_cigar=2, tags=TAGS))
        recs.append(bc.record("bare%d" % length, _seq(rng, length), None, flag=flag))
    text = _device(gpu, recs)
    first = len(bc.text_of(recs[0]))
    assert first // 4096 + 2 <= (first + len(bc.text_of(recs[1])) - 1) // 4096   # (recs[1] lies in three tiles)
    assert len(text) > 16 * 4096


def test_names_of_1_and_254_bytes(gpu):
    rng = random.Random(4)
    long_name = "".join(chr(0x21 + i % 94) for i in range(254))
    recs = [bc.record("x", "A", [5]), bc.record(long_name, _seq(rng, 40), _qual(rng, 40)), bc.record("~", _seq(rng, 17), None, flag=0x14),
            bc.record(long_name[::-1], "C", None), bc.record("!", _seq(rng, 33), _qual(rng, 33), flag=0x10)]
    _device(gpu, recs, each=True)


def test_many_one_base_records_in_one_vector(gpu):
    """FASTA records of 5 bytes and FASTQ records of 9: a lane's 16 bytes hold the ends and starts of up to four; skipped ones between"""
    rng = random.Random(5)
    recs = []
    for i in range(1500):
        kind = rng.randrange(6)
        base = rng.choice(bc.LETTERS)
        if kind == 0:
            recs.append(bc.record("s", base, [9], flag=rng.choice([0x104, 0x804, 0x900])))
        elif kind == 1:
            recs.append(bc.record("e", "", []))
        else:
            recs.append(bc.record(rng.choice("abcdefg"), base, None if kind < 4 else [rng.randrange(94)], flag=rng.choice([4, 0x14])))
    text = _device(gpu, recs)
    assert len(text) > 4096 and len(recs) > 4 * 256   # (more than one tile, and more than one block of the measure kernel)


def test_every_code_and_quality(gpu):
    recs = []
    for lead in ("", "A"):   # (the sixteen codes in high and in low nibbles)
        for flag in (4, 0x14):
            seq = lead + bc.LETTERS * 3
            recs.append(bc.record("codes", seq, [(0, 93, 94, 254, 255, 1, 92, 127, 128)[i % 9] for i in range(len(seq))], flag=flag))
            recs.append(bc.record("codes_no_quality", seq, None, flag=flag))
            recs.append(bc.record("absent_by_first", seq, [255] + [7] * (len(seq) - 1), flag=flag))
            recs.append(bc.record("last_is_255", seq, [7] * (len(seq) - 1) + [255], flag=flag))   # (reversed, 0xFF comes first in the text: still qual[0] that decides)
    text = _device(gpu, recs, each=True)
    assert b"~" in text and b"!" in text and text.count(b">") >= 8


def test_reverse_strand_odd_and_even(gpu):
    rng = random.Random(7)
    recs = [bc.record("r%d" % n, _seq(rng, n, bc.LETTERS), _qual(rng, n), flag=0x10 | (4 if n % 3 else 0), n_cigar=n % 3, tags=TAGS if n % 2 else b"")
            for n in (4, 5, 34, 35, 48, 49, 63, 64, 65, 100, 101, 1000, 1001)]
    _device(gpu, recs, each=True)


def test_skipped_records_first_last_and_in_runs(gpu):
    rng = random.Random(8)

    def kept(i):
        return bc.record("k%d" % i, _seq(rng, 50 + i), _qual(rng, 50 + i))

    def skipped(i):
        return [bc.record("sec", _seq(rng, 20), _qual(rng, 20), flag=0x100), bc.record("sup", _seq(rng, 21), None, flag=0x800),
                bc.record("empty", "", []), bc.record("both", _seq(rng, 5), _qual(rng, 5), flag=0x914)][i % 4]

    recs = [skipped(0), skipped(1), kept(0), skipped(2), kept(1), kept(2)] + [skipped(i) for i in range(7)] + [kept(3), skipped(3)]
    _device(gpu, recs)
    _device(gpu, recs, skip=0)        # (nothing skipped but the empty ones)
    _device(gpu, recs, skip=0x100)
    _device(gpu, [skipped(i) for i in range(9)])   # (no text at all)
    _device(gpu, [skipped(0)], each=True)


def test_cigar_and_tags_move_seq_and_qual(gpu):
    rng = random.Random(9)
    recs = [bc.record("c%d" % i, _seq(rng, 30 + i, bc.LETTERS), _qual(rng, 30 + i) if i % 3 else None, flag=(4, 0x14)[i % 2], n_cigar=i, tags=TAGS * (i % 4))
            for i in range(12)]
    _device(gpu, recs, each=True)


def test_zero_records(gpu):
    from trio_binning_amd import seq

    assert seq.bam_fastq_device(b"", []) == (b"", 0, 0)


def test_the_first_bad_record_is_named(gpu):
    from trio_binning_amd import seq

    rng = random.Random(10)
    good = [bc.record("g%d" % i, _seq(rng, 10 + i % 40), _qual(rng, 10 + i % 40)) for i in range(700)]   # (three blocks of the measure kernel)
    bads = [dict(good[0], l_seq=4000), dict(good[0], raw_name=b"a b\0"), dict(good[0], raw_name=b"abc"), dict(good[0], raw_name=b"\0")]
    for which, at in enumerate((0, 699, 350, 256)):
        recs = list(good)
        recs[at] = bads[which]
        data, offsets = bc.records_bytes(recs)
        with pytest.raises(ValueError, match="record {}:".format(at)):
            seq.bam_fastq_device(data, offsets)
        with pytest.raises(ValueError, match="record {}:".format(at)):
            seq.bam_fastq_host(data, offsets)
    recs = list(good)
    recs[600], recs[77], recs[300] = bads[0], bads[1], bads[2]
    data, offsets = bc.records_bytes(recs)
    with pytest.raises(ValueError, match="record 77:"):
        seq.bam_fastq_device(data, offsets)
    with pytest.raises(ValueError, match="offsets"):
        seq.bam_fastq_device(data, [len(data) - 8])


# ---- the reader and the command lines ---------------------------------------------------------------------------------

WINDOW, PAYLOAD = 65536, 777


def _windows(blocks):
    """the reader's windows over bgzf blocks [(file offset, size)]: blocks are taken while the window holds less than WINDOW bytes"""
    out, start, size = [], 0, 0
    for i, (_, n) in enumerate(blocks):
        size += n
        if size >= WINDOW:
            out.append((start, i + 1))
            start, size = i + 1, 0
    if start < len(blocks):
        out.append((start, len(blocks)))
    return out


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """A BAM of a few hundred reads of 1 to 60 000 bases, some without quality, some skipped, in bgzf blocks of 777 bytes, and its
    FASTQ twin.  Checked here: the file is at least four windows long, a block_size field straddles a block edge, and a record
    lies in more than two windows."""
    rng = random.Random(2024)
    tmp = tmp_path_factory.mktemp("bam_library")
    recs, at = [], len(bc.header([]))
    for i in range(300):
        if i == 99:   # a read sized so that the next record's block_size field lies across a block edge: two bytes each side
            length = next(n for n in range(1, 3000) if (at + len(bc.encode(bc.record("m64011_99/%d/ccs" % n, "A" * n, [1] * n, tags=TAGS)))) % PAYLOAD == PAYLOAD - 2)
            letters = "ACGT"
        elif i in (100, 101, 102, 103, 104):
            length, letters = 60000, bc.LETTERS   # (every code, qualities at random: such a record takes more than a window of the file)
        else:
            length, letters = rng.choice([1, 2, 16, 33, 150, 500, 1500, 1500, 3000, 15000 if i % 10 == 0 else 700]), "ACGT"
        seq = "".join(rng.choices(letters, k=length))
        qual = None if i % 9 == 4 else rng.choices(range(94), k=length)
        flag = 0x904 if i % 50 == 49 else (0x14 if i % 4 == 1 else 4)
        if i == 99:
            qual, flag = rng.choices(range(94), k=length), 4
        recs.append(bc.record("m64011_%d/%d/ccs" % (i, length), seq, qual, flag=flag, tags=TAGS))
        at += len(bc.encode(recs[-1]))
    raw = bc.bam_bytes(recs, refs=[])
    data = bc.bgzf(raw, block=PAYLOAD)
    # where the blocks and the records lie
    blocks, p = [], 0
    while p < len(data):
        n = (data[p + 16] | data[p + 17] << 8) + 1
        blocks.append((p, n))
        p += n
    windows = _windows(blocks)
    assert len(data) >= 4 * WINDOW and len(windows) >= 4
    starts, at = [], len(bc.header([]))
    for r in recs:
        starts.append(at)
        at += len(bc.encode(r))
    assert any(s % PAYLOAD > PAYLOAD - 4 for s in starts), "no block_size field straddles a block edge"
    window_of_block = {b: w for w, (lo, hi) in enumerate(windows) for b in range(lo, hi)}
    spans = [window_of_block[(starts[i] + len(bc.encode(recs[i])) - 1) // PAYLOAD] - window_of_block[starts[i] // PAYLOAD] + 1 for i in range(len(recs))]
    assert max(spans) > 2, "no record lies in more than two windows"
    bam, twin = tmp / "reads.hifi_reads.bam", tmp / "reads.fastq"
    bam.write_bytes(data)
    twin.write_bytes(bc.fastq_of(recs))
    return {"recs": recs, "bam": bam, "twin": twin, "data": data, "raw": raw, "dir": tmp, "blocks": blocks, "windows": windows}


def _records(path, **kw):
    from trio_binning_amd import seq

    out = []
    with seq.NativeReader(str(path), **kw) as r:
        on_device = r.inflates_on_device
        b = seq.Batch()
        while r.next_batch(b, 200_000, 0):
            reads = b.reads()
            out.append([(x.name, x.seq, x.qual) for x in reads])
        counts = r.bam_counts()
        from trio_binning_amd._lib import lib

        on_device = on_device and bool(lib.tbk_fastx_inflates_on_device(r._h))   # (still: a loop that handed over to the host says so)
        b.close()
    return out, on_device, counts


def test_reader_gives_the_twins_batches(gpu, library, monkeypatch):
    monkeypatch.setenv("TBK_BGZF_GPU_WINDOW", str(WINDOW))
    want, _, none = _records(library["twin"])
    got, on_device, counts = _records(library["bam"], device=0)
    lengths = bc.lengths_of(library["recs"])
    assert on_device and none is None and counts == (len(lengths), sum(1 for l in lengths if not l))
    flat = lambda batches: [x for b in batches for x in b]
    assert flat(got) == flat(want) and len(flat(got)) == sum(1 for l in lengths if l)
    assert len(got) > 3   # (several batches; where a batch ends depends on the window the parser has at hand, as for any inflated input)
    on_host, was_device, _ = _records(library["bam"])
    assert not was_device and flat(on_host) == flat(want)
    monkeypatch.setenv("TBK_BGZF_GPU_SLOTS", "1")   # (as if the windows' memory were not there: the host does both, as on the bgzf path)
    handed, was_device, _ = _records(library["bam"], device=0)
    assert not was_device and flat(handed) == flat(want)


def _lists(library):
    """k-mers cut from the reads themselves: hapA from every third ACGT read, hapB from the ones behind them"""
    d = library["dir"]
    cut = {0: [], 1: []}
    for i, r in enumerate(library["recs"]):
        if len(r["seq"]) >= 150 and len(r["seq"]) < 20000 and i % 3 < 2:
            cut[i % 3] += [r["seq"][p:p + 21] for p in range(0, len(r["seq"]) - 21, 37)]
    paths = []
    for hap, name in ((0, "hapA.txt"), (1, "hapB.txt")):
        path = d / name
        path.write_text("".join(k + "\n" for k in sorted(set(cut[hap]))))
        paths.append(str(path))
    return paths


@pytest.mark.parametrize("gz", [True, False], ids=["gzip", "no-gzip-output"])
def test_classify_by_kmers_from_bam(gpu, library, capfd, tmp_path, monkeypatch, gz):
    import trio_binning_amd.classify_by_kmers as cbk

    monkeypatch.setenv("TBK_BGZF_GPU_WINDOW", str(WINDOW))
    lists = _lists(library)
    out = {}
    for kind, reads in (("bam", library["bam"]), ("twin", library["twin"])):
        od = tmp_path / kind
        od.mkdir()
        argv = ["classify-by-kmers", str(reads)] + lists + ["--haplotype-a-out-prefix", str(od / "hapA"), "--haplotype-b-out-prefix", str(od / "hapB"),
                                                             "--unclassified-out-prefix", str(od / "unclassified")] + ([] if gz else ["--no-gzip-output"])
        with patch("sys.argv", argv):
            cbk.main()
        tsv, _ = capfd.readouterr()
        names = sorted(p.name for p in od.iterdir())
        assert names == sorted(b + ".fastq" + (".gz" if gz else "") for b in ("hapA", "hapB", "unclassified")), kind
        out[kind] = (tsv, {n: (gzip.open(od / n, "rb") if gz else open(od / n, "rb")).read() for n in names})
    assert out["bam"][0] == out["twin"][0] and out["bam"][0].count("\n") == sum(1 for l in bc.lengths_of(library["recs"]) if l)
    assert out["bam"][1] == out["twin"][1]
    assert all(len(v) > 0 for v in out["bam"][1].values())   # (reads in every bin)


def test_reader_refuses_damaged_files_twice(gpu, library, tmp_path, monkeypatch):
    from trio_binning_amd import seq

    monkeypatch.setenv("TBK_BGZF_GPU_WINDOW", str(WINDOW))
    raw, data = library["raw"], library["data"]
    cut = tmp_path / "cut.bam"
    cut.write_bytes(bc.bgzf(raw[:len(raw) - 5], block=PAYLOAD))   # (ends inside the last record)
    damaged = bytearray(data)
    damaged[library["blocks"][library["windows"][3][0] + 2][0] + 18 + 5] ^= 0x55   # (in the deflate stream of the fourth window's third block)
    bad = tmp_path / "damaged.bam"
    bad.write_bytes(bytes(damaged))
    for path, words in ((cut, "record {}: the file ends inside".format(len(library["recs"]) - 1)), (bad, "")):
        with seq.NativeReader(str(path), device=0) as reader:
            batch = seq.Batch()
            with pytest.raises((ValueError, IOError)) as first:
                while reader.next_batch(batch, 200_000, 0):
                    pass
            with pytest.raises(type(first.value)) as again:
                reader.next_batch(batch, 200_000, 0)
            batch.close()
        assert str(first.value) and str(again.value) == str(first.value) and words in str(first.value), (path.name, str(first.value))


def _parents(seed=21, glen=60_000, n_reads=10_000, read_len=150):
    """two parents of one small genome, a SNP every 200 bases, reads with a few errors (the histogram's first peak): name -> records"""
    rng = random.Random(seed)
    base = rng.choices("ACGT", k=glen)
    out = {}
    for name in ("mother", "father"):
        g = list(base)
        for p in range(glen):
            if rng.random() < 1 / 200:
                g[p] = "ACGT"[("ACGT".index(g[p]) + rng.randrange(1, 4)) % 4]
        recs = []
        for i in range(n_reads):
            p = rng.randrange(0, glen - read_len)
            r = g[p:p + read_len]
            for q in rng.sample(range(read_len), (0, 0, 1, 1, 1, 2, 3, 0)[i % 8]):   # (one error a read, about)
                r[q] = rng.choice("ACGT")
            qual = None if i % 11 == 0 else rng.choices(range(20, 60), k=read_len)
            recs.append(bc.record("%s%d" % (name[0], i), "".join(r), qual, flag=(4, 0x14)[i % 2], tags=TAGS))
        out[name] = recs
    return out


def test_find_unique_kmers_from_bam_parents(gpu, tmp_path, capsys):
    """two small parents as BAM and as FASTQ: the same lists"""
    from trio_binning_amd import find_unique_kmers as fu

    parents = _parents()
    got = {}
    for kind in ("bam", "fastq"):
        d = tmp_path / kind
        (d / "out").mkdir(parents=True)
        paths = []
        for name, recs in parents.items():
            path = d / (name + "." + kind)
            path.write_bytes(bc.bgzf(bc.bam_bytes(recs), block=PAYLOAD) if kind == "bam" else bc.fastq_of(recs))
            paths.append(str(path))
        fu.main(["-k", "21", "-o", str(d / "out"), "-s", str(d), "--capacity", "3000000"] + paths)
        capsys.readouterr()
        got[kind] = {n: open(d / "out" / n).read() for n in ("hapA_only_kmers.txt", "hapB_only_kmers.txt")}
    assert got["bam"] == got["fastq"] and all(len(v) > 22 * 500 for v in got["bam"].values())
