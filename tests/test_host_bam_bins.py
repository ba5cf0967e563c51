"""BAM bins from BAM input without a device (include/tbk.h "BAM output"): the host bgzf coder against a walker that follows
BSIZE and checks every field, the reader's batches that carry their records against ``bam_craft.encode``, the writer's
three BAM files against the input's header and records byte for byte, the same host pieces in a stand-alone program under
AddressSanitizer and UBSan, and what the command line makes of ``--bam-output``."""
import os
import subprocess
import sys

import pytest

import bam_bins_craft as bb
import bam_craft as bc
from conftest import ROOT


# ---- the host encoder ----
@pytest.mark.parametrize("size,members", bb.SIZES, ids=[str(s) for s, _ in bb.SIZES])
def test_host_encoder_payload_sizes(built, size, members):
    from trio_binning_amd import seq

    data = bb.payload(size)
    blob, n = seq.bgzf_members_host(data)
    assert n == members
    assert len(bb.check_members(blob, data, n)) == members
    if size:
        assert len(blob) < size + 26 * members + 64   # (it is coded, not merely stored)


def test_host_encoder_incompressible_members_fit(built):
    from trio_binning_amd import seq

    data, hints = bb.incompressible()
    blob, n = seq.bgzf_members_host(data, hints)
    bb.check_members(blob, data, n)   # (every member <= 65536 bytes: the walker holds each BSIZE to it)
    assert len(blob) > len(data)      # nothing to gain on these bytes: the blocks are stored


def test_hint_handling(built):
    from trio_binning_amd import seq

    data = bb.payload(100000)
    for hints in ([0], [len(data)], [0, 0, 9000, 9000, 9000, len(data), len(data)], [], None):
        blob, n = seq.bgzf_members_host(data, hints)
        bb.check_members(blob, data, n)
    for hints in ([9000, 8999], [0, len(data), 5], [len(data) + 1], [5, 1 << 40]):
        with pytest.raises(ValueError, match="hints"):
            seq.bgzf_members_host(data, hints)


def test_hints_pay(built):
    from trio_binning_amd import seq

    data, hints = bb.alternating()
    assert len(data) == 600 * 1024
    hinted, n1 = seq.bgzf_members_host(data, hints)
    fixed, n2 = seq.bgzf_members_host(data)
    print("hinted %d bytes, fixed cuts %d bytes: %.4f" % (len(hinted), len(fixed), len(hinted) / len(fixed)))
    bb.check_members(hinted, data, n1)
    bb.check_members(fixed, data, n2)
    assert len(hinted) < 0.95 * len(fixed)


@pytest.mark.parametrize("hints,blocks", bb.CUTS, ids=[str(i) for i in range(len(bb.CUTS))])
def test_host_cuts_follow_the_rule(built, hints, blocks):
    from trio_binning_amd import seq

    data = bb.payload(65280)
    blob, n = seq.bgzf_members_host(data, hints)
    assert n == 1 and bb.coded_block_sizes(blob) == blocks


# ---- the reader ----
@pytest.fixture(scope="module")
def crafted():
    recs = bb.big_records()
    text = bb.crafted_header()
    return {"recs": recs, "kept": bb.kept(recs), "text": text, "header": bc.header(text=text), "raw": bc.bam_bytes(recs, text=text)}


@pytest.fixture(scope="module")
def crafted_files(crafted, tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_bins_in")
    out = {}
    for block in (0xFF00, 777):
        out[block] = str(d / ("in%d.bam" % block))
        with open(out[block], "wb") as fh:
            fh.write(bc.bgzf(crafted["raw"], block=block, level=1))
    return out


def test_the_crafted_file_has_every_shape(crafted):
    recs, kept = crafted["recs"], crafted["kept"]
    assert len(crafted["text"]) >= 70000
    assert any(b"MLBC" in r["tags"] for r in kept) and any(not r["tags"] for r in kept)
    assert any(len(r["seq"]) == 100000 for r in kept) and any(len(r["seq"]) == 1 for r in kept)
    assert any(r["qual"] is None for r in kept) and any(r["flag"] & 0x10 for r in kept) and any(r["n_cigar"] for r in kept)
    skipped = [i for i, r in enumerate(recs) if r not in kept]
    assert any(0 < i < len(recs) - 1 and recs[i - 1] in kept and recs[i + 1] in kept for i in skipped)
    assert any(not r["seq"] for r in recs) and any(r["flag"] & 0x100 for r in recs) and any(r["flag"] & 0x800 for r in recs)


@pytest.mark.parametrize("block", [0xFF00, 777])
def test_reader_batches_carry_their_records(built, crafted, crafted_files, block):
    from trio_binning_amd import seq

    names, records = [], []
    with seq.BatchReader(crafted_files[block], keep_records=True) as reader:
        assert reader.bam_header() == crafted["header"]   # (before the first batch: the call reads it)
        batch = seq.Batch()
        while reader.next_batch(batch, 0, 4):
            got = batch.records()
            assert len(got) == batch.n_reads
            records += got
            names += [r.name for r in batch.reads()]
        assert batch.records() == []
        assert reader.bam_header() == crafted["header"]
        assert reader.bam_counts() == (len(crafted["recs"]), len(crafted["recs"]) - len(crafted["kept"]))
        batch.close()
    assert names == [r["name"] for r in crafted["kept"]]
    assert records == [bc.encode(r) for r in crafted["kept"]]


def test_reader_without_the_option_keeps_nothing(built, crafted, crafted_files):
    from trio_binning_amd import seq

    text = bytearray()
    with seq.BatchReader(crafted_files[777]) as reader:
        batch = seq.Batch()
        while reader.next_batch(batch, 1 << 20, 0):
            assert batch.records() == []
            for r in batch.reads():
                text += (">{}\n{}\n".format(r.name, r.seq) if r.qual is None else "@{}\n{}\n+\n{}\n".format(r.name, r.seq, r.qual)).encode()
        batch.close()
    assert bytes(text) == bc.fastq_of(crafted["recs"])


def test_keep_records_is_refused_for_fastq(built, tmp_path):
    from trio_binning_amd import seq

    for name, content in (("r.fastq", b"@a\nACGT\n+\nIIII\n"), ("r.fastq.gz", bc.bgzf(b"@a\nACGT\n+\nIIII\n"))):
        (tmp_path / name).write_bytes(content)
        with pytest.raises(ValueError, match="not BAM"):
            seq.BatchReader(str(tmp_path / name), keep_records=True)
        with seq.BatchReader(str(tmp_path / name)) as reader:
            with pytest.raises(ValueError, match="not BAM"):
                reader.bam_header()


# ---- the writer on the host ----
def write_bins(path, prefix, deal, device=None, limits=((0, 3), (0, 5), (8 << 20, 0))):
    """The file at `path` through the writer in batches of growing size (three reads, five reads, then several MB: `limits` is
    (max_bases, max_reads) of the first batches, its last entry of every later one), bins dealt by `deal(index of the read)`.
    Returns (the three file names, the bins dealt, whether the device coded)."""
    from trio_binning_amd import seq

    dealt = []
    with seq.BatchReader(path, keep_records=True) as reader:
        writer = seq.BinWriter(prefix + "A", prefix + "B", prefix + "U", ".bam", True, device=device, bam_header=reader.bam_header())
        batch = seq.Batch()
        turn = 0
        while True:
            max_bases, max_reads = limits[min(turn, len(limits) - 1)]
            turn += 1
            n = reader.next_batch(batch, max_bases, max_reads)
            if not n:
                break
            bins = bytes(deal(len(dealt) + i) for i in range(n))
            dealt += list(bins)
            writer.write(batch, bins)
        on_device = writer.gpu_encoder
        writer.close()
        batch.close()
    return writer.names, dealt, on_device


def check_bins(names, dealt, kept, header):
    for which, name in zip(b"ABU", names):
        assert name.endswith(".bam")
        got_header, records, data = bb.read_bam_file(name)
        want = [r for r, c in zip(kept, dealt) if c == which]
        assert got_header == header
        assert records == [bc.encode(r) for r in want]
        assert bc.parse(data) == bc.fastq_of(want)
    assert len(dealt) == len(kept)


DEALS = {"pattern": lambda i: b"ABUAABUUB"[i % 9], "all_in_b": lambda i: ord("B")}


@pytest.mark.parametrize("deal", sorted(DEALS))
def test_writer_on_the_host(built, crafted, crafted_files, tmp_path, deal):
    names, dealt, on_device = write_bins(crafted_files[0xFF00], str(tmp_path / "bin"), DEALS[deal])
    assert not on_device
    check_bins(names, dealt, crafted["kept"], crafted["header"])
    if deal == "all_in_b":
        assert os.path.getsize(names[0]) == os.path.getsize(names[2]) < os.path.getsize(names[1])


def test_writer_on_the_host_no_reads_at_all(built, crafted, tmp_path):
    only_skipped = [r for r in crafted["recs"] if r not in crafted["kept"]]
    path = tmp_path / "none.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(only_skipped, text=crafted["text"]), block=5000))
    names, dealt, _ = write_bins(str(path), str(tmp_path / "bin"), DEALS["pattern"])
    assert dealt == []
    check_bins(names, dealt, [], crafted["header"])
    for name in names:   # header plus marker
        with open(name, "rb") as fh:
            payloads = bb.walk(fh.read())
        assert b"".join(payloads) == crafted["header"] and payloads[-1] == b"" and len(payloads) == 3


def test_writer_refuses_batches_without_records(built, crafted, crafted_files, tmp_path):
    from trio_binning_amd import seq

    with seq.BatchReader(crafted_files[0xFF00]) as reader:
        writer = seq.BinWriter(str(tmp_path / "A"), str(tmp_path / "B"), str(tmp_path / "U"), ".bam", True, bam_header=crafted["header"])
        batch = seq.Batch()
        n = reader.next_batch(batch, 0, 2)
        with pytest.raises(RuntimeError, match="no records"):
            writer.write(batch, b"A" * n)
        writer.close()
        batch.close()


def test_zlib_as_the_host_coder(built, crafted, crafted_files, tmp_path):
    """TBK_GZIP_ENCODER=zlib (read when the writer is opened; a fresh process): the same bins"""
    code = ("import sys; sys.path[:0] = [{!r}, {!r}]\nimport test_host_bam_bins as t\n"
            "names, dealt, _ = t.write_bins({!r}, {!r}, t.DEALS['pattern'])\nprint(bytes(dealt).decode())\n").format(
                ROOT, os.path.join(ROOT, "tests"), crafted_files[0xFF00], str(tmp_path / "z"))
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, TBK_GZIP_ENCODER="zlib"))
    assert run.returncode == 0, run.stderr[-3000:]
    dealt = list(run.stdout.split()[-1].encode())
    check_bins([str(tmp_path / "z") + c + ".bam" for c in "ABU"], dealt, crafted["kept"], crafted["header"])


# ---- the same host pieces under sanitizers, as a program ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/native/bam_bins_check.cpp with its own main, built with AddressSanitizer and UBSan for the CPU"""
    exe = str(tmp_path_factory.mktemp("bam_bins_check") / "bam_bins_check")
    csrc = os.path.join(ROOT, "trio_binning_amd", "csrc")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                            os.path.join(ROOT, "tests", "native", "bam_bins_check.cpp"), os.path.join(csrc, "tbk_deflate.cpp"), os.path.join(csrc, "tbk_crc.cpp"),
                            "-lz", "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.mark.parametrize("window,hints", [(1 << 30, 1), (65536, 1), (1000, 0)])
def test_host_pieces_under_sanitizers(checker, crafted, tmp_path, window, hints):
    raw, out = tmp_path / "in.bam.raw", tmp_path / "out.bam"
    raw.write_bytes(crafted["raw"])
    run = subprocess.run([checker, str(raw), str(out), str(window), str(hints), "3"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    said = run.stdout.split()
    assert said[:3] == ["ok", str(len(crafted["kept"])), str(len(crafted["recs"]) - len(crafted["kept"]))]
    header, records, _ = bb.read_bam_file(str(out))
    assert header == crafted["header"] and records == [bc.encode(r) for r in crafted["kept"]]
    assert int(said[4]) == os.path.getsize(str(out))


def test_host_pieces_under_sanitizers_incompressible(checker, tmp_path):
    """records whose bytes do not compress (random qualities and tags over all byte values): stored blocks, members that still fit"""
    import random

    rng = random.Random(31)
    recs = [bc.record("r%d" % i, "".join(rng.choices(bc.LETTERS, k=9000)), [rng.randrange(255) for _ in range(9000)], tags=b"xxBC" + (20000).to_bytes(4, "little") + rng.randbytes(20000))
            for i in range(8)]
    raw, out = tmp_path / "in.bam.raw", tmp_path / "out.bam"
    raw.write_bytes(bc.bam_bytes(recs))
    run = subprocess.run([checker, str(raw), str(out), "40000", "1", "2"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    header, records, _ = bb.read_bam_file(str(out))
    assert records == [bc.encode(r) for r in recs]


# ---- the command line ----
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", *args], capture_output=True, text=True, cwd=ROOT)


def test_command_line(built, tmp_path):
    from trio_binning_amd import _lib

    assert _lib.lib.tbk_abi_version() == 1
    shown = _cli("--help")
    assert shown.returncode == 0 and "--bam-output" in shown.stdout
    data = os.path.join(ROOT, "tests", "data")
    lists = [os.path.join(data, "hapA.txt"), os.path.join(data, "hapB.txt")]
    for argv, words in ((["--bam-output", str(tmp_path / "reads.fastq.gz")] + lists, "must be a .bam file"),
                        (["--bam-output", "--no-gzip-output", str(tmp_path / "reads.bam")] + lists, "exclude each other")):
        run = _cli(*argv)
        assert run.returncode == 2 and "error:" in run.stderr and words in run.stderr, run.stderr[-2000:]
        assert run.stdout == ""
    assert not list(tmp_path.iterdir())
