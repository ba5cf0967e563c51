"""BAM bins on the device (include/tbk.h "BAM output"): the bgzf mode of csrc/tbk_gdeflate.hip against the same walker and
the same inflated bytes as the host twin - the host tests' shapes, jobs that take the scan and CRC kernels' strided loops
round again, a job whose members carry all three bins - the writer with the device encoder against the host writer's bins,
and classify-by-kmers --bam-output end to end."""
import gzip
import os
import random
from unittest.mock import patch

import pytest

import bam_bins_craft as bb
import bam_craft as bc
from conftest import ROOT
from test_host_bam_bins import DEALS, check_bins, write_bins

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "tests", "data")


def both(data, hints=None):
    """the device's blocks for `data`, checked field by field, beside the host twin's: the same inflated bytes, the same members"""
    from trio_binning_amd import seq

    blob, n = seq.bgzf_members_device(data, hints)
    payloads = bb.check_members(blob, data, n)
    twin, m = seq.bgzf_members_host(data, hints)
    assert m == n and bb.walk(twin) == payloads
    return blob, twin


@pytest.mark.parametrize("size,members", bb.SIZES, ids=[str(s) for s, _ in bb.SIZES])
def test_device_encoder_payload_sizes(gpu, size, members):
    from trio_binning_amd import seq

    data = bb.payload(size)
    blob, _ = both(data)
    assert seq.bgzf_members_device(data)[1] == members
    if size:
        assert len(blob) < size + 26 * members + 64


def test_device_encoder_incompressible_members_fit(gpu):
    data, hints = bb.incompressible()
    blob, _ = both(data, hints)
    assert len(blob) > len(data)


def test_device_hint_handling(gpu):
    from trio_binning_amd import seq

    data = bb.payload(100000)
    for hints in ([0], [len(data)], [0, 0, 9000, 9000, 9000, len(data), len(data)], [], None):
        both(data, hints)
    for hints in ([9000, 8999], [0, len(data), 5], [len(data) + 1], [5, 1 << 40]):
        with pytest.raises(ValueError, match="hints"):
            seq.bgzf_members_device(data, hints)


def test_device_hints_pay(gpu):
    data, hints = bb.alternating()
    hinted, _ = both(data, hints)
    fixed, _ = both(data)
    print("device: hinted %d bytes, fixed cuts %d bytes: %.4f" % (len(hinted), len(fixed), len(hinted) / len(fixed)))
    assert len(hinted) < 0.95 * len(fixed)


@pytest.mark.parametrize("hints,blocks", bb.CUTS, ids=[str(i) for i in range(len(bb.CUTS))])
def test_device_cuts_follow_the_rule(gpu, hints, blocks):
    """(the host twin cuts by the same rule, and where a deflate block ends shows in neither's inflated bytes: count them)"""
    from trio_binning_amd import seq

    data = bb.payload(65280)
    blob, n = seq.bgzf_members_device(data, hints)
    assert n == 1 and bb.coded_block_sizes(blob) == blocks


def test_device_later_trips_of_the_block_scan(gpu):
    """more than 256 deflate blocks in one job: gd_scan_kernel's strided loop goes round again (3 MB, hints every 8200 bytes: ~370 blocks)"""
    data = bb.payload(3_000_000, seed=5)
    both(data, list(range(8200, len(data), 8200)))


def test_device_later_trips_of_the_members(gpu):
    """more than 64 members in one job, the last one short: 70 x 65280 + 999 bytes"""
    data = bb.payload(70 * 65280 + 999, seed=6)
    blob, _ = both(data)
    assert len(bb.walk(blob)) == 71


def test_device_members_of_all_three_tags_interleaved(gpu):
    """One job whose members carry all three tags (the writer's bins) interleaved: every member comes back with its own tag, in the
    order it went in, and inflates to its own piece."""
    import ctypes as C

    from trio_binning_amd._lib import check, lib

    data = bb.payload(11 * 65280 + 4321, seed=9)
    n = 12
    tags = [(0, 1, 2, 2, 0, 1)[i % 6] for i in range(n)]
    hints = list(range(0, len(data), 9001))
    cap = len(data) + 128 * n
    buf = C.create_string_buffer(cap)
    need, members = C.c_uint64(), C.c_uint64()
    out_tags, out_len = (C.c_int32 * n)(*([-1] * n)), (C.c_uint64 * n)()
    check(lib.tbk_bgzf_members_tagged_device_(0, data, len(data), (C.c_uint64 * len(hints))(*hints), len(hints), (C.c_int32 * n)(*tags), buf, cap, C.byref(need),
                                              C.byref(members), out_tags, out_len))
    assert members.value == n and list(out_tags) == tags and sum(out_len) == need.value
    at = 0
    for i in range(n):
        piece = bb.walk(buf.raw[at:at + out_len[i]])
        assert piece == [data[i * 65280:(i + 1) * 65280]]
        at += out_len[i]


def test_writer_job_with_members_of_all_three_bins(gpu, crafted, crafted_files, tmp_path):
    """the same through the writer: its second batch is several MB dealt A, B, U in turn, so one flush submits members of all three
    bins in one job, and each bin's file gets exactly its own, in order"""
    names, dealt, on_device = write_bins(crafted_files[0xFF00], str(tmp_path / "bin"), lambda i: b"ABU"[i % 3], device=0, limits=[(0, 2), (64 << 20, 0)])
    assert on_device
    check_bins(names, dealt, crafted["kept"], crafted["header"])
    assert all(os.path.getsize(n) > 200000 for n in names)   # (each bin holds several members of that job)


# ---- the writer with the device encoder ----
@pytest.fixture(scope="module")
def crafted():
    recs = bb.big_records()
    text = bb.crafted_header()
    return {"recs": recs, "kept": bb.kept(recs), "text": text, "header": bc.header(text=text), "raw": bc.bam_bytes(recs, text=text)}


@pytest.fixture(scope="module")
def crafted_files(crafted, tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_bins_in")
    path = str(d / "in.bam")
    with open(path, "wb") as fh:
        fh.write(bc.bgzf(crafted["raw"], level=1))
    return {0xFF00: path}


@pytest.mark.parametrize("deal", sorted(DEALS))
def test_writer_with_the_device_encoder(gpu, crafted, crafted_files, tmp_path, deal):
    names, dealt, on_device = write_bins(crafted_files[0xFF00], str(tmp_path / "dev"), DEALS[deal], device=0)
    assert on_device   # (tbk_bin_writer_encoder)
    check_bins(names, dealt, crafted["kept"], crafted["header"])
    host_names, host_dealt, host_on_device = write_bins(crafted_files[0xFF00], str(tmp_path / "host"), DEALS[deal])
    assert not host_on_device and host_dealt == dealt
    for a, b in zip(names, host_names):
        assert bb.read_bam_file(a)[2] == bb.read_bam_file(b)[2]


def test_writer_with_the_device_encoder_no_reads_at_all(gpu, crafted, tmp_path):
    only_skipped = [r for r in crafted["recs"] if r not in crafted["kept"]]
    path = tmp_path / "none.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(only_skipped, text=crafted["text"]), block=5000))
    names, dealt, on_device = write_bins(str(path), str(tmp_path / "bin"), DEALS["pattern"], device=0)
    assert on_device and dealt == []
    check_bins(names, dealt, [], crafted["header"])


# ---- end to end ----
def _run_free_kmers(rng, n):
    """21-mers without two equal adjacent bases: what a list made with --compress holds (the command refuses tests/data/hapA.txt in
    that mode - it has runs - so the --compress run gets lists of its own; such a k-mer planted in a read survives compression)"""
    out = []
    while len(out) < n:
        kmer = [rng.choice("ACGT")]
        while len(kmer) < 21:
            kmer.append(rng.choice([c for c in "ACGT" if c != kmer[-1]]))
        out.append("".join(kmer))
    return out


def _library(compressed_lists):
    """About 200 reads cut from the sequences of tests/data: stretches of test.fastq's reads as background, k-mers of hapA.txt (and
    of the run-free list A) planted in a third of them, of hapB.txt (and run-free B) in another third; tags, skipped records and
    reverse-strand records among them."""
    rng = random.Random(77)
    with open(os.path.join(DATA, "test.fastq")) as fh:
        sources = [line.strip() for i, line in enumerate(fh) if i % 4 == 1]
    lists = {hap: [line.strip() for line in open(os.path.join(DATA, "hap%s.txt" % hap)) if line.strip()] for hap in "AB"}
    recs = []
    for i in range(200):
        n = rng.choice([300, 800, 2500, 9000])
        seq = ""
        while len(seq) < n:
            src = rng.choice(sources)
            at = rng.randrange(len(src) - 10)
            seq += src[at:at + rng.randrange(10, 40)]
        seq = list(seq[:n])
        hap = "ABU"[i % 3]
        if hap != "U":
            for j, p in enumerate(range(0, n - 50, 97)):
                seq[p:p + 21] = rng.choice(lists[hap] if j % 2 == 0 else compressed_lists[hap])
        flag = (4, 0x14)[i % 4 == 1]
        qual = None if i % 17 == 5 else [rng.randrange(3, 90) for _ in range(n)]
        recs.append(bc.record("m77/%d/ccs" % i, "".join(seq), qual, flag=flag, tags=bb.tag_block(rng, kinetics=n if i % 5 == 0 else 0) if i % 7 else b""))
        if i % 9 == 4:
            recs.append(bc.record("m77/%d/sup" % i, "".join(seq[:100]), qual[:100] if qual else None, flag=0x800 | 4, tags=bb.tag_block(rng)))
        if i % 31 == 8:
            recs.append(bc.record("m77/%d/none" % i, "", [], tags=bb.tag_block(rng)))
    return recs


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_bins_e2e")
    rng = random.Random(78)
    compressed_lists = {"A": _run_free_kmers(rng, 5), "B": _run_free_kmers(rng, 5)}
    for hap, kmers in compressed_lists.items():
        (d / ("hap%s_compressed.txt" % hap)).write_text("".join(k + "\n" for k in kmers))
    recs = _library(compressed_lists)
    text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:0a1b2c3d\tPL:PACBIO\n@PG\tID:ccs\tPN:ccs\n"
    path = d / "reads.hifi_reads.bam"
    path.write_bytes(bc.bgzf(bc.bam_bytes(recs, text=text), level=1))
    return {"recs": recs, "kept": bb.kept(recs), "header": bc.header(text=text), "bam": str(path),
            "lists": [os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt")],
            "compressed_lists": [str(d / "hapA_compressed.txt"), str(d / "hapB_compressed.txt")]}


def _run(library, capfd, out_dir, extra):
    import trio_binning_amd.classify_by_kmers as cbk

    out_dir.mkdir()
    argv = ["classify-by-kmers", library["bam"]] + library["compressed_lists" if "--compress" in extra else "lists"] + ["--haplotype-a-out-prefix", str(out_dir / "hapA"),
            "--haplotype-b-out-prefix", str(out_dir / "hapB"), "--unclassified-out-prefix", str(out_dir / "unclassified")] + extra
    with patch("sys.argv", argv):
        cbk.main()
    tsv, _ = capfd.readouterr()
    return tsv, sorted(p.name for p in out_dir.iterdir())


def _names_of_fastq(path):
    with gzip.open(path, "rt") as fh:
        lines = fh.read().split("\n")
    names, i = [], 0
    while i < len(lines) and lines[i]:
        names.append(lines[i][1:])
        i += 4 if lines[i][0] == "@" else 2
    return names


def test_classify_by_kmers_bam_output_end_to_end(gpu, library, capfd, tmp_path):
    by_name = {r["name"]: bc.encode(r) for r in library["kept"]}
    tsv_fastq, fastq_names = _run(library, capfd, tmp_path / "fastq", [])
    assert fastq_names == ["hapA.fastq.gz", "hapB.fastq.gz", "unclassified.fastq.gz"]
    assert tsv_fastq.count("\n") == len(library["kept"])
    for mode, extra in (("bam", ["--bam-output"]), ("bam_compress", ["--bam-output", "--compress"])):
        tsv, names = _run(library, capfd, tmp_path / mode, extra)
        assert names == ["hapA.bam", "hapB.bam", "unclassified.bam"]
        if mode == "bam":
            assert tsv == tsv_fastq   # the TSV has the same bytes as without the flag
        else:
            tsv_plain, _ = _run(library, capfd, tmp_path / "fastq_compress", ["--compress"])
            assert tsv == tsv_plain
        bins = {line.split("\t")[0]: line.split("\t")[1] for line in tsv.splitlines()}
        seen = 0
        for which, stem in (("A", "hapA"), ("B", "hapB"), ("U", "unclassified")):
            header, records, _ = bb.read_bam_file(str(tmp_path / mode / (stem + ".bam")))
            assert header == library["header"]
            got_names = [rec[36:36 + rec[12] - 1].decode() for rec in records]
            assert got_names == [r["name"] for r in library["kept"] if bins[r["name"]] == which]
            if mode == "bam":
                assert got_names == _names_of_fastq(str(tmp_path / "fastq" / (stem + ".fastq.gz")))
            assert all(rec == by_name[name] for rec, name in zip(records, got_names))   # every record byte-equal to its input record
            assert records, "bin %s is empty: the library must fill all three" % which
            seen += len(records)
        assert seen == len(library["kept"])
