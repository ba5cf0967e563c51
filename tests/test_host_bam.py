"""BAM input without a device: tests/bam_craft.py (the rule) against the host pieces of csrc/tbk_bam.h in a stand-alone
program under AddressSanitizer and UBSan, the native reader on a .bam path against the reader on the FASTQ twin, every
refusal of include/tbk.h "BAM input" with its record number, and what the command lines make of a .bam name."""
import os
import random
import subprocess

import pytest

import bam_craft as bc
from conftest import ROOT


def _mixed_records(seed=5, n=240):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        length = rng.choice([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 100, 777, 1500, 4000])
        seq = "".join(rng.choice(bc.LETTERS if i % 5 == 0 else "ACGT") for _ in range(length))
        qual = None if i % 7 == 3 else [rng.choice([0, 1, 40, 93, 94, 254, 255]) if j else rng.choice([0, 93, 94, 254]) for j in range(length)]
        flag = rng.choice([4, 4, 0x14, 0x104, 0x804, 0x10, 0])
        recs.append(bc.record("read%d/%d" % (i, length), seq, qual, flag=flag, n_cigar=i % 3, tags=b"rqf\x00\x00\x80\x3f" if i % 2 else b""))
    return recs


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/native/bam_check.cpp with its own main, built with AddressSanitizer and UBSan for the CPU"""
    exe = str(tmp_path_factory.mktemp("bam_check") / "bam_check")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                            os.path.join(ROOT, "trio_binning_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "native", "bam_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _check(exe, tmp_path, data, window, skip=bc.SKIP_DEFAULT, cap=1000):
    raw, out = tmp_path / "in.bam.raw", tmp_path / "out.fastq"
    raw.write_bytes(data)
    run = subprocess.run([exe, str(raw), str(out), str(window), hex(skip), str(cap)], capture_output=True, text=True)
    assert run.returncode in (0, 3), run.stdout + run.stderr[-3000:]
    return run.stdout.split(), out.read_bytes() if out.exists() else b""


def test_the_rule_restated_twice():
    """fastq_of (from the records as made) and parse (from the bytes alone) agree, and say what the issue says"""
    recs = _mixed_records()
    assert bc.parse(bc.bam_bytes(recs, refs=[("chr1", 1000), ("c2", 5)])) == bc.fastq_of(recs)
    r = bc.record("n", "=ACMGRSVTWYHKDBN", [0, 93, 94, 254] * 4)
    assert bc.fastq_of([r]) == b"@n\n=ACMGRSVTWYHKDBN\n+\n" + b"!~~~" * 4 + b"\n"
    assert len(bc.fastq_of([r])) == len("n") + 2 * 16 + 6
    r = bc.record("n", "AACM=", [1, 2, 3, 4, 5], flag=0x10)
    assert bc.fastq_of([r]) == b"@n\n=KGTT\n+\n&%$#\"\n"
    assert bc.fastq_of([bc.record("n", "ACG", None)]) == b">n\nACG\n"
    assert bc.fastq_of([bc.record("n", "ACG", [255, 1, 2])]) == b">n\nACG\n"   # (qual[0] == 0xFF: absent)
    assert bc.fastq_of([bc.record("n", "ACG", [1, 2, 3], flag=0x100), bc.record("m", "", []), bc.record("s", "A", [9], flag=0x800)]) == b""
    assert bc.fastq_of([bc.record("n", "A", [9], flag=0x100)], skip_flags=0) == b"@n\nA\n+\n*\n"


@pytest.mark.parametrize("window", [1, 13, 4096, 1 << 22])
def test_host_pieces_under_sanitizers(checker, tmp_path, window):
    recs = _mixed_records()
    data = bc.bam_bytes(recs, refs=[("chr1", 1000)])
    lengths = bc.lengths_of(recs)
    for cap in (1, 1000):
        said, text = _check(checker, tmp_path, data, window, cap=cap)
        assert text == bc.fastq_of(recs)
        assert said == ["ok", str(sum(1 for l in lengths if l)), str(sum(1 for l in lengths if not l))]
    said, text = _check(checker, tmp_path, data, window, skip=0)
    assert text == bc.fastq_of(recs, 0) and said[0] == "ok"
    said, text = _check(checker, tmp_path, bc.bam_bytes([]), window)
    assert said == ["ok", "0", "0"] and text == b""


def _good(i):
    return bc.record("ok%d" % i, "ACGTACGTAC", [30] * 10)


def _broken():
    """(what is wrong, the bad record) for every refusal that a record can carry"""
    long_seq = dict(_good(0), l_seq=400)
    return [
        ("block_size below the fields' sum", long_seq),
        ("block_size one short", dict(_good(0), block_size=32 + 4 + 5 + 10 - 1)),
        ("block_size below the fixed part", dict(_good(0), block_size=31)),
        ("block_size above the bound", dict(_good(0), block_size=bc.MAX_RECORD + 1)),
        ("block_size negative", dict(_good(0), block_size=0xFFFFFFF0)),
        ("l_read_name 1", dict(_good(0), raw_name=b"\0")),
        ("l_read_name 0", dict(_good(0), raw_name=b"")),
        ("a space in the name", dict(_good(0), raw_name=b"a b\0")),
        ("0x7F in the name", dict(_good(0), raw_name=b"ab\x7f\0")),
        ("a NUL inside the name", dict(_good(0), raw_name=b"a\0b\0")),
        ("no NUL at the name's end", dict(_good(0), raw_name=b"abcd")),
    ]


BROKEN = _broken()


def _with_bad(bad, at, n=9):
    recs = [_good(i) for i in range(n)]
    recs[at] = bad
    return recs


@pytest.mark.parametrize("what,bad", BROKEN, ids=[w for w, _ in BROKEN])
def test_the_rule_and_the_host_pieces_refuse(checker, tmp_path, what, bad):
    for at in (0, 4, 8):
        data = bc.bam_bytes(_with_bad(bad, at))
        with pytest.raises(bc.BamError) as exc:
            bc.parse(data)
        assert exc.value.record_no == at, what
        for window in (7, 1 << 20):
            said, _ = _check(checker, tmp_path, data, window)
            assert said[:2] == ["refused", str(at)], (what, at, window, said)
    data = bc.bam_bytes([_good(0), _good(1), bad, _good(3), BROKEN[5][1]])   # two bad records: the lower number
    assert _check(checker, tmp_path, data, 50)[0][:2] == ["refused", "2"]


def _native_reads(path, device=None, max_bases=1 << 20):
    from trio_binning_amd import seq

    out = []
    with seq.NativeReader(str(path), device=device) as reader:
        batch = seq.Batch()
        while reader.next_batch(batch, max_bases, 0):
            out += [(r.name, r.seq, r.qual) for r in batch.reads()]
        counts = reader.bam_counts()
        batch.close()
    return out, counts


@pytest.mark.parametrize("block", [61, 777, 0xFF00])
def test_native_reader_reads_bam_as_its_fastq_twin(built, tmp_path, block):
    recs = _mixed_records(seed=block)
    bam, twin = tmp_path / "x.bam", tmp_path / "x.fastq"
    bam.write_bytes(bc.bgzf(bc.bam_bytes(recs, refs=[("chr1", 1000)]), block=block, eof=block != 61))   # (a missing end-of-file marker is accepted)
    twin.write_bytes(bc.fastq_of(recs))
    want, none = _native_reads(twin)
    got, counts = _native_reads(bam)
    lengths = bc.lengths_of(recs)
    assert none is None and counts == (len(recs), sum(1 for l in lengths if not l))
    assert got == want and len(got) == sum(1 for l in lengths if l)
    assert any(q is None for _, _, q in got) and any(q for _, _, q in got)
    from trio_binning_amd import seq

    assert [(r.name, r.seq, r.qual) for r in seq.open_fastx_read(str(bam))] == want


def test_host_one_shot_equals_the_rule(built):
    from trio_binning_amd import seq

    recs = _mixed_records(seed=11)
    data, offsets = bc.records_bytes(recs)
    lengths = bc.lengths_of(recs)
    text, written, skipped = seq.bam_fastq_host(data, offsets)
    assert text == bc.fastq_of(recs) and (written, skipped) == (sum(1 for l in lengths if l), sum(1 for l in lengths if not l))
    assert seq.bam_fastq_host(data, offsets, 0)[0] == bc.fastq_of(recs, 0)
    assert seq.bam_fastq_host(b"", []) == (b"", 0, 0)
    with pytest.raises(ValueError, match="offsets"):
        seq.bam_fastq_host(data, [len(data) - 8])


def _refusal(path, device=None):
    """the reader's message for a file it must refuse - said again on the next call"""
    from trio_binning_amd import seq

    with seq.NativeReader(str(path), device=device) as reader:
        batch = seq.Batch()
        with pytest.raises((ValueError, IOError)) as first:
            while reader.next_batch(batch, 1 << 20, 0):
                pass
        with pytest.raises(type(first.value)) as again:
            reader.next_batch(batch, 1 << 20, 0)
        batch.close()
    assert str(again.value) == str(first.value) and str(first.value)
    return first.value


@pytest.mark.parametrize("what,bad", BROKEN, ids=[w for w, _ in BROKEN])
def test_native_reader_refuses_naming_the_record(built, tmp_path, what, bad):
    for at in (0, 4, 8):
        path = tmp_path / ("bad%d.bam" % at)
        path.write_bytes(bc.bgzf(bc.bam_bytes(_with_bad(bad, at)), block=97))
        err = _refusal(path)
        assert isinstance(err, ValueError) and "record %d:" % at in str(err), (what, at, str(err))


def test_native_reader_refuses_files(built, tmp_path):
    from trio_binning_amd import seq

    recs = [_good(i) for i in range(12)]
    data = bc.bam_bytes(recs, refs=[("chr1", 1000)])
    cases = {
        "cut.bam": (bc.bgzf(data[:-7], block=50), "record 11: the file ends inside"),
        "cut_in_size.bam": (bc.bgzf(data[:len(bc.header([("chr1", 1000)])) + 2], block=50), "record 0: the file ends inside"),
        "header.bam": (bc.bgzf(data[:20], block=5), "ends inside the header"),
        "magic.bam": (bc.bgzf(b"BAM\2" + data[4:]), "not a BAM file"),
        "fastq.bam": (bc.bgzf(bc.fastq_of(recs)), "not a BAM file"),
        "empty_text.bam": (bc.bgzf(b""), "ends inside the header"),
    }
    for name, (content, words) in cases.items():
        path = tmp_path / name
        path.write_bytes(content)
        err = _refusal(path)
        assert isinstance(err, ValueError) and words in str(err), (name, str(err))
    # a bgzf stream cut inside a block, in front of which every record is whole: the gzip layer's message
    whole = bc.bgzf(data, block=len(data), eof=False)
    (tmp_path / "block.bam").write_bytes(whole + bc.bgzf(b"x" * 100, eof=False)[:-20])
    assert "truncated" in str(_refusal(tmp_path / "block.bam"))
    damaged = bytearray(bc.bgzf(data, block=200))
    damaged[18 + 3] ^= 0x55   # (inside the first block's deflate stream: its CRC-32 no longer holds)
    (tmp_path / "damaged.bam").write_bytes(bytes(damaged))
    assert str(_refusal(tmp_path / "damaged.bam"))
    # a .bam that is not bgzf is refused where it is opened
    for name, content in (("plain.bam", data), ("gzip.bam", __import__("gzip").compress(data)), ("short.bam", b"BAM\1"), ("none.bam", b"")):
        (tmp_path / name).write_bytes(content)
        with pytest.raises(ValueError, match="not a BAM file"):
            seq.NativeReader(str(tmp_path / name))


def test_command_lines_know_bam(built, tmp_path):
    from trio_binning_amd import classify_by_kmers as cli
    from trio_binning_amd import find_unique_kmers as fuk

    assert cli.output_extension("reads.hifi_reads.bam") == ".fastq"
    assert cli.output_extension("a/b.c/x.bam") == ".fastq"
    for name, ext in (("r.fastq", ".fastq"), ("r.fq.gz", ".fq"), ("r.fastq.gz", ".fastq"), ("r.bam.gz", ".bam"), ("r.fa", ".fa"), ("bam", "")):
        assert cli.output_extension(name) == ext, name
    for name in ("a.bam", "a.gz", "a.fastq"):
        (tmp_path / name).write_bytes(b"x" * 1000)
    assert fuk.estimate_bases([str(tmp_path / "a.bam")]) == fuk.estimate_bases([str(tmp_path / "a.gz")]) == 2000
    assert fuk.estimate_bases([str(tmp_path / "a.fastq")]) == 501
    # the arguments as the first reading of the command line takes them (the k-mer arguments as strings: no table is built)
    args = cli._parser(str).parse_args(["--no-gzip-output", str(tmp_path / "reads.hifi_reads.bam"), "hapA.txt", "hapB.txt"])
    assert args.reads.endswith("reads.hifi_reads.bam") and cli.output_extension(args.reads) == ".fastq"
    from trio_binning_amd import seq

    assert seq.output_names("a", "b", "u", cli.output_extension(args.reads), not args.no_gzip_output) == ("a.fastq", "b.fastq", "u.fastq")
    assert seq.output_names("a", "b", "u", cli.output_extension(args.reads), True) == ("a.fastq.gz", "b.fastq.gz", "u.fastq.gz")
