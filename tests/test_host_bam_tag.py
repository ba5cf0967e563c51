"""Haplotag output without a device (include/tbk.h "Haplotag output"): the host rewriter against the plain-Python rule of
``bam_tag_ref`` on the crafted records, ``out_off`` and every refusal included; the same header in a stand-alone program
under AddressSanitizer and UBSan; the writer with the host coder on one file; and the command line's refusals."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bam_bins_craft as bb
import bam_craft as bc
import bam_tag_ref as tr
from conftest import ROOT

SETS = {"crafted": tr.crafted, "tiny": tr.tiny, "big": tr.big}
_made = {}


def records_of(which):
    """(records, bins, counts, expected bytes, expected out_off) of one crafted set: made once, shared, never changed"""
    if which not in _made:
        recs, bins, counts = SETS[which]()
        _made[which] = (recs, bins, counts) + tr.retag_all(recs, bins, counts)
    return _made[which]


def run_of(recs):
    offsets, at = [], 0
    for r in recs:
        offsets.append(at)
        at += len(r)
    return b"".join(recs), offsets


def test_the_reference_on_a_record_made_by_hand():
    """the rule once by hand, so that the reference is not only compared with code written beside it"""
    rec = bc.encode(bc.record("r", "AC", [5, 6], tags=b"HPi\x09\0\0\0" + b"xyZab\0" + b"kbC\x03"))
    want_body = rec[4:4 + 32 + 2 + 1 + 2] + b"xyZab\0" + b"HPC\x02" + b"kaI\x07\0\0\0" + b"kbI\xff\xff\xff\x7f"
    assert tr.retag(rec, "B", 7, 2 ** 31 - 1) == struct.pack("<i", len(want_body)) + want_body
    assert tr.retag(rec, "U", 0, 1)[4:] == rec[4:41] + b"xyZab\0" + b"kaI\0\0\0\0" + b"kbI\x01\0\0\0"
    assert [name for _, _, name in tr.fields(rec)] == [b"HP", b"xy", b"kb"]


def test_the_crafted_sets_have_every_shape():
    recs, bins, _, out, off = records_of("crafted")
    assert {len(r) % 16 for r in recs} == set(range(16)) and {o % 16 for o in off} == set(range(16))
    assert min(len(r) for r in recs) == 40 and set(bins) == set("ABU")
    kinds = {chr(r[s + 2]) for r in recs for s, _, _ in tr.fields(r)}
    assert kinds == set("AcCsSiIfZHB")
    big, _, _, big_out, big_off = records_of("big")
    assert any(4096 < len(r) < 65536 for r in big) and any(len(r) > 65536 for r in big)
    # a dropped field across a 16-byte vector boundary and a 4096-byte tile boundary, of the input run and of the output
    run_at, across = 0, set()
    for r, o in zip(big, big_off):
        for s, e, name in tr.fields(r):
            if name in tr.DROPPED:
                for step in (16, 4096):
                    if (run_at + s) // step != (run_at + e - 1) // step:
                        across.add(("in", step))
                    dropped_before = sum(e2 - s2 for s2, e2, n2 in tr.fields(r) if n2 in tr.DROPPED and s2 < s)
                    if (o + s - dropped_before - 1) // step != (o + s - dropped_before) // step:
                        across.add(("out", step))
        run_at += len(r)
    assert across == {("in", 16), ("in", 4096), ("out", 16), ("out", 4096)}


@pytest.mark.parametrize("which", sorted(SETS))
def test_host_rewriter_equals_the_reference(built, which):
    from trio_binning_amd import seq

    recs, bins, counts, want, want_off = records_of(which)
    data, offsets = run_of(recs)
    got, off = seq.bam_haplotag_host(data, offsets, bins.encode(), counts)
    assert off == want_off
    assert got == want


def test_host_rewriter_edges(built):
    from trio_binning_amd import _lib, seq

    recs, bins, counts, want, want_off = records_of("crafted")
    assert seq.bam_haplotag_host(b"", [], b"", np.zeros((0, 2), np.int32)) == (b"", [0])          # n = 0
    got, off = seq.bam_haplotag_host(recs[0], [0], b"B", [counts[0]])                              # n = 1
    assert (got, off) == tr.retag_all(recs[:1], "B", counts[:1])
    data, offsets = run_of(recs)
    status, wrote, _, out_len = seq.bam_haplotag_status(data, offsets, bins.encode(), counts, None, cap=len(want) - 1)
    assert status == _lib.TBK_ERR_NOMEM and out_len == len(want) and wrote == b""
    status, wrote, off, out_len = seq.bam_haplotag_status(data, offsets, bins.encode(), counts, None, cap=len(want))
    assert status == 0 and wrote == want and off == want_off
    # any other byte in `bins` counts as U; the records need not lie back to back, nor in order
    got, off = seq.bam_haplotag_host(b"\0" * 3 + recs[1] + b"\0" * 5 + recs[0], [8 + len(recs[1]), 3], b"?A", [(1, 2), (3, 4)])
    assert got == tr.retag(recs[0], "U", 1, 2) + tr.retag(recs[1], "A", 3, 4)
    for bad_counts in ([(-1, 0)], [(0, -1)], [(-2 ** 31, 5)]):
        with pytest.raises(ValueError, match="count below 0"):
            seq.bam_haplotag_host(recs[0], [0], b"A", bad_counts)
    with pytest.raises(ValueError, match="offsets"):
        seq.bam_haplotag_host(recs[0], [1], b"A", [(0, 0)])


@pytest.mark.parametrize("what,tags,reason", tr.refused(), ids=[w.replace(" ", "_") for w, _, _ in tr.refused()])
def test_host_rewriter_refusals(built, what, tags, reason):
    from trio_binning_amd import seq

    good, _, counts, _, _ = records_of("crafted")
    bad = tr.refused_record(tags)
    with pytest.raises(tr.TagError) as said:
        tr.retag_all(good[:5] + [bad] + good[5:8] + [bad], "A" * 10, counts[:10])
    assert said.value.record_no == 5 and said.value.why == reason
    data, offsets = run_of(good[:5] + [bad] + good[5:8] + [bad])
    with pytest.raises(ValueError, match=r"BAM record 5: .*" + reason):
        seq.bam_haplotag_host(data, offsets, b"A" * 10, counts[:10])


def test_host_rewriter_first_of_several_and_too_long(built):
    from trio_binning_amd import seq

    good, _, counts, _, _ = records_of("crafted")
    cases = tr.refused()
    recs = good[:100] + [tr.refused_record(cases[3][1])] + good[100:130] + [tr.refused_record(cases[0][1])] + [tr.refused_record(cases[16][1])]
    data, offsets = run_of(recs)
    with pytest.raises(ValueError, match="BAM record 100: .*" + cases[3][2]):
        seq.bam_haplotag_host(data, offsets, b"U" * len(recs), [(1, 1)] * len(recs))
    huge = tr.too_long_record()
    with pytest.raises(tr.TagError, match=tr.LONG):
        tr.retag(huge, "U", 0, 0)
    data, offsets = run_of([good[0], huge])
    status, _, _, _ = seq.bam_haplotag_status(data, offsets, b"AU", [(0, 0), (0, 0)], None, cap=0)
    assert status == -3   # TBK_ERR_FORMAT
    from trio_binning_amd._lib import last_error

    assert "BAM record 1: " in last_error() and tr.LONG in last_error()


# ---- the same header under sanitizers, as a program ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/native/bam_tag_check.cpp with its own main, built with AddressSanitizer and UBSan for the CPU"""
    exe = str(tmp_path_factory.mktemp("bam_tag_check") / "bam_tag_check")
    csrc = os.path.join(ROOT, "trio_binning_amd", "csrc")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-o", exe,
                            os.path.join(ROOT, "tests", "native", "bam_tag_check.cpp"), "-lpthread"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _check(checker, tmp_path, recs, bins, counts, threads, mode):
    (tmp_path / "in.raw").write_bytes(b"".join(recs))
    (tmp_path / "plan.bin").write_bytes(b"".join(bins[i].encode() + struct.pack("<ii", *counts[i]) for i in range(len(recs))))
    run = subprocess.run([checker, str(tmp_path / "in.raw"), str(tmp_path / "plan.bin"), str(tmp_path / "out.raw"), str(threads), mode], capture_output=True, text=True)
    return run, (tmp_path / "out.raw").read_bytes() if run.returncode == 0 else b""


@pytest.mark.parametrize("which,threads,mode", [("crafted", 3, "run"), ("crafted", 1, "alone"), ("tiny", 5, "run"), ("big", 2, "run"), ("big", 1, "alone")])
def test_host_pieces_under_sanitizers(checker, tmp_path, which, threads, mode):
    recs, bins, counts, want, want_off = records_of(which)
    run, out = _check(checker, tmp_path, recs, bins, counts, threads, mode)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    said = run.stdout.split()
    assert said[:3] == ["ok", str(len(recs)), str(len(want))] and [int(x) for x in said[3:]] == want_off
    assert out == want


def test_host_pieces_under_sanitizers_refusals(checker, tmp_path):
    """every refusal, the bad record the last one of a heap block that ends where it ends"""
    good, _, counts, _, _ = records_of("crafted")
    for what, tags, reason in tr.refused():
        for mode in ("run", "alone"):
            run, _ = _check(checker, tmp_path, good[:3] + [tr.refused_record(tags)], "ABUA", counts[:4], 2, mode)
            assert run.returncode == 3 and run.stdout.startswith("refused 3 ") and reason in run.stdout, (what, mode, run.stdout + run.stderr[-3000:])


# ---- the writer with the host coder ----
def write_tagged(path, out_path, deal, device=None, limits=((0, 1), (8 << 20, 0))):
    """The file at `path` through the haplotag writer, batches by `limits` as test_host_bam_bins.write_bins takes them; bins and
    counts dealt by `deal(index of the read)` -> (bin byte, a, b).  Returns (what was dealt, gpu_encoder, gpu_rewriter)."""
    from trio_binning_amd import seq

    dealt = []
    with seq.BatchReader(path, keep_records=True) as reader:
        writer = seq.BinWriter("", "", "", ".bam", True, device=device, bam_header=reader.bam_header(), haplotag_path=out_path)
        batch = seq.Batch()
        turn = 0
        while True:
            max_bases, max_reads = limits[min(turn, len(limits) - 1)]
            turn += 1
            n = reader.next_batch(batch, max_bases, max_reads)
            if not n:
                break
            mine = [deal(len(dealt) + i) for i in range(n)]
            dealt += mine
            writer.write_counts(batch, bytes(m[0] for m in mine), np.array([m[1:] for m in mine], dtype=np.int32))
        flags = (writer.gpu_encoder, writer.gpu_rewriter)
        writer.close()
        batch.close()
    return dealt, flags[0], flags[1]


def deal_pattern(i):
    return (b"ABUAABUUB"[i % 9],) + tr.COUNTS[i % len(tr.COUNTS)]


def check_tagged(out_path, kept, dealt, header):
    got_header, records, _ = bb.read_bam_file(out_path)
    assert got_header == header
    assert len(dealt) == len(kept) == len(records)
    want, _ = tr.retag_all([bc.encode(r) for r in kept], [chr(d[0]) for d in dealt], [d[1:] for d in dealt])
    assert b"".join(records) == want


@pytest.fixture(scope="module")
def crafted_file(tmp_path_factory):
    recs = bb.crafted_records()
    text = bb.crafted_header()
    path = str(tmp_path_factory.mktemp("bam_tag_in") / "in.bam")
    with open(path, "wb") as fh:
        fh.write(bc.bgzf(bc.bam_bytes(recs, text=text), level=1))
    return {"path": path, "kept": bb.kept(recs), "header": bc.header(text=text), "recs": recs, "text": text}


def test_writer_on_the_host(built, crafted_file, tmp_path):
    out = str(tmp_path / "tagged.bam")
    dealt, on_device, rewrites_on_device = write_tagged(crafted_file["path"], out, deal_pattern)
    assert not on_device and not rewrites_on_device
    check_tagged(out, crafted_file["kept"], dealt, crafted_file["header"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["tagged.bam"]


def test_writer_on_the_host_no_reads_at_all(built, crafted_file, tmp_path):
    only_skipped = [r for r in crafted_file["recs"] if r not in crafted_file["kept"]]
    path = tmp_path / "none.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(only_skipped, text=crafted_file["text"]), block=5000))
    out = str(tmp_path / "tagged.bam")
    dealt, _, _ = write_tagged(str(path), out, deal_pattern)
    assert dealt == []
    with open(out, "rb") as fh:
        payloads = bb.walk(fh.read())
    assert b"".join(payloads) == crafted_file["header"] and payloads[-1] == b""   # header plus marker


def test_writer_call_sequence(built, crafted_file, tmp_path):
    from trio_binning_amd import seq

    header = crafted_file["header"]
    tagged = seq.BinWriter("", "", "", ".bam", True, bam_header=header, haplotag_path=str(tmp_path / "t.bam"))
    bins = seq.BinWriter(str(tmp_path / "A"), str(tmp_path / "B"), str(tmp_path / "U"), ".bam", True, bam_header=header)
    batch = seq.Batch()
    with seq.BatchReader(crafted_file["path"]) as reader:            # batches without records
        n = reader.next_batch(batch, 0, 2)
        with pytest.raises(RuntimeError, match="no records"):
            tagged.write_counts(batch, b"A" * n, np.zeros((n, 2), np.int32))
    with seq.BatchReader(crafted_file["path"], keep_records=True) as reader:
        n = reader.next_batch(batch, 0, 2)
        with pytest.raises(RuntimeError, match="write_counts"):
            tagged.write(batch, b"A" * n)                             # plain write on a haplotag writer
        with pytest.raises(RuntimeError, match="not a haplotag writer"):
            bins.write_counts(batch, b"A" * n, np.zeros((n, 2), np.int32))
        with pytest.raises(ValueError, match="count below 0"):
            tagged.write_counts(batch, b"A" * n, np.array([[0, 0], [0, -1]], np.int32))
    tagged.close()
    bins.close()
    batch.close()
    with pytest.raises(ValueError, match="BAM header"):
        seq.BinWriter("", "", "", ".bam", True, haplotag_path=str(tmp_path / "x.bam"))


# ---- the command line and the native loop ----
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "trio_binning_amd.classify_by_kmers", *args], capture_output=True, text=True, cwd=ROOT)


def test_command_line(built, tmp_path):
    shown = _cli("--help")
    assert shown.returncode == 0 and "--haplotag-output" in shown.stdout
    data = os.path.join(ROOT, "tests", "data")
    lists = [os.path.join(data, "hapA.txt"), os.path.join(data, "hapB.txt")]
    out = str(tmp_path / "tagged.bam")
    for argv, words in ((["--haplotag-output", out, str(tmp_path / "reads.fastq.gz")] + lists, "must be a .bam file"),
                        (["--haplotag-output", out, "--bam-output", str(tmp_path / "reads.bam")] + lists, "--haplotag-output and --bam-output exclude each other"),
                        (["--haplotag-output", out, "--no-gzip-output", str(tmp_path / "reads.bam")] + lists, "--haplotag-output and --no-gzip-output exclude each other")):
        run = _cli(*argv)
        assert run.returncode == 2 and "error:" in run.stderr and words in run.stderr, run.stderr[-2000:]
        assert run.stdout == ""
    assert not list(tmp_path.iterdir())
