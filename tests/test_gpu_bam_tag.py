"""Haplotag output on the device (include/tbk.h "Haplotag output"): the kernels of csrc/tbk_bam_tag.hip against the host
rewriter and the plain-Python rule of ``bam_tag_ref`` byte for byte - every aux type, HP wherever it can lie, vector and
tile edges, every refusal - the writer with the device coder (and with the device rewriter) on uneven batches, and
classify-by-kmers --haplotag-output end to end.  Neither kernel strides over records or tiles (a thread per record, a block
per tile), so there is no later trip to take."""
import os
import random
import re
import struct

import numpy as np
import pytest

import bam_bins_craft as bb
import bam_craft as bc
import bam_tag_ref as tr
from conftest import ROOT
from test_gpu_bam_bins import _run, library  # noqa: F401  (the crafted library of the BAM-bin tests, and its runner)
from test_host_bam_tag import check_tagged, deal_pattern, records_of, run_of, write_tagged

pytestmark = pytest.mark.gpu
TBK_ERR_FORMAT, TBK_ERR_NOMEM = -3, -6


@pytest.mark.parametrize("which", ["crafted", "tiny", "big"])
def test_device_rewriter_equals_host_and_reference(gpu, which):
    """crafted: every aux type, HP first / middle / last / alone, the six orders, every stored form of HP, bins and counts mixed,
    every residue mod 16 of sizes and offsets, the smallest record.  tiny: 5000 records, ~70 to a tile.  big: a record larger than
    a tile, one larger than 64 KiB with kinetics arrays and a 70 kB Z string, dropped fields across vector and tile boundaries."""
    from trio_binning_amd import seq

    recs, bins, counts, want, want_off = records_of(which)
    data, offsets = run_of(recs)
    got, off = seq.bam_haplotag_device(data, offsets, bins.encode(), counts)
    host, host_off = seq.bam_haplotag_host(data, offsets, bins.encode(), counts)
    assert off == host_off == want_off
    assert got == host
    assert got == want


def test_device_rewriter_edges(gpu):
    from trio_binning_amd import seq

    recs, bins, counts, want, want_off = records_of("crafted")
    assert seq.bam_haplotag_device(b"", [], b"", np.zeros((0, 2), np.int32)) == (b"", [0])                      # n = 0
    smallest = min(recs, key=len)
    assert len(smallest) == 40
    for which, (a, b) in zip("ABU", [(0, 0), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1)]):                               # n = 1
        assert seq.bam_haplotag_device(smallest, [0], which.encode(), [(a, b)]) == tr.retag_all([smallest], which, [(a, b)])
    data, offsets = run_of(recs)
    status, wrote, _, out_len = seq.bam_haplotag_status(data, offsets, bins.encode(), counts, 0, cap=len(want) - 1)
    assert status == TBK_ERR_NOMEM and out_len == len(want) and wrote == b""                                       # cap one byte short
    status, wrote, off, out_len = seq.bam_haplotag_status(data, offsets, bins.encode(), counts, 0, cap=len(want))
    assert status == 0 and wrote == want and off == want_off
    # records that do not lie back to back, nor in order: the offsets decide
    got, _ = seq.bam_haplotag_device(b"\0" * 3 + recs[1] + b"\0" * 5 + recs[0], [8 + len(recs[1]), 3], b"?A", [(1, 2), (3, 4)])
    assert got == tr.retag(recs[0], "U", 1, 2) + tr.retag(recs[1], "A", 3, 4)
    with pytest.raises(ValueError, match="count below 0"):
        seq.bam_haplotag_device(recs[0], [0], b"A", [(0, -1)])
    with pytest.raises(ValueError, match="offsets"):
        seq.bam_haplotag_device(recs[0], [1], b"A", [(0, 0)])


@pytest.mark.parametrize("what,tags,reason", tr.refused(), ids=[w.replace(" ", "_") for w, _, _ in tr.refused()])
def test_device_rewriter_refusals(gpu, what, tags, reason):
    from trio_binning_amd import _lib, seq

    good, _, counts, _, _ = records_of("crafted")
    bad = tr.refused_record(tags)
    recs = good[:5] + [bad] + good[5:8] + [bad]
    data, offsets = run_of(recs)
    with pytest.raises(ValueError, match=r"BAM record 5: .*" + reason):
        seq.bam_haplotag_device(data, offsets, b"A" * 10, counts[:10])
    said = _lib.last_error()
    with pytest.raises(ValueError) as host:
        seq.bam_haplotag_host(data, offsets, b"A" * 10, counts[:10])
    assert said.split(": ", 1)[1] == str(host.value).split(": ", 1)[1]   # the same record, the same reason


def test_device_rewriter_first_of_several_and_too_long(gpu):
    from trio_binning_amd import _lib, seq

    good, _, counts, _, _ = records_of("crafted")
    tiny, _, _, _, _ = records_of("tiny")
    cases = tr.refused()
    # bad records in three different blocks of the measure kernel: the lowest index wins whichever block runs first
    recs = tiny[:700] + [tr.refused_record(cases[3][1])] + tiny[700:1400] + [tr.refused_record(cases[0][1])] + tiny[1400:2000] + [tr.refused_record(cases[16][1])]
    data, offsets = run_of(recs)
    with pytest.raises(ValueError, match="BAM record 700: .*" + cases[3][2]):
        seq.bam_haplotag_device(data, offsets, b"U" * len(recs), [(1, 1)] * len(recs))
    huge = tr.too_long_record()
    data, offsets = run_of([good[0], huge])
    status, _, _, _ = seq.bam_haplotag_status(data, offsets, b"AU", [(0, 0), (0, 0)], 0, cap=0)
    assert status == TBK_ERR_FORMAT
    assert "BAM record 1: " in _lib.last_error() and tr.LONG in _lib.last_error()


# ---- the writer with the device coder ----
@pytest.fixture(scope="module")
def uneven(tmp_path_factory):
    """1 record, then 5000 tiny ones, then one record of 200 kB: the batches `write_tagged` is told to take"""
    rng = random.Random(21)
    crafted = records_of("crafted")[0]
    last = tr._rec("big/200kb", 100000, tr.b_array("fi", "C", 50000, rng) + tr.HP_FORMS[4] + tr.field("MM", "Z", b"C+m," + b"3," * 2000 + b";\0"), rng)
    assert len(last) > 200000
    recs = [crafted[0]] + records_of("tiny")[0] + [last]
    text = bb.crafted_header()
    d = tmp_path_factory.mktemp("bam_tag_uneven")
    path, none = str(d / "in.bam"), str(d / "none.bam")
    with open(path, "wb") as fh:
        fh.write(bc.bgzf(bc.header(text=text) + b"".join(recs), level=1))
    with open(none, "wb") as fh:
        fh.write(bc.bgzf(bc.bam_bytes([bc.record("skipped", "ACGT", [9] * 4, flag=0x900), bc.record("empty", "", [])], text=text), level=1))
    return {"path": path, "none": none, "recs": recs, "header": bc.header(text=text)}


def _check_file(out, recs, dealt, header):
    got_header, records, _ = bb.read_bam_file(out)   # (the walker holds every block to 65536 bytes and the marker to the end)
    assert got_header == header
    want, _ = tr.retag_all(recs, [chr(d[0]) for d in dealt], [d[1:] for d in dealt])
    assert len(records) == len(recs) == len(dealt) and b"".join(records) == want


@pytest.mark.parametrize("rewrite", ["cpu", "gpu", None])
def test_writer_with_the_device_coder_uneven_batches(gpu, uneven, tmp_path, monkeypatch, rewrite):
    if rewrite is None:
        monkeypatch.delenv("TBK_HAPLOTAG_REWRITE", raising=False)
    else:
        monkeypatch.setenv("TBK_HAPLOTAG_REWRITE", rewrite)
    out = str(tmp_path / "tagged.bam")
    dealt, coder_on_device, rewriter_on_device = write_tagged(uneven["path"], out, deal_pattern, device=0, limits=((0, 1), (0, 5000), (0, 0)))
    assert coder_on_device
    if rewrite is not None:
        assert rewriter_on_device == (rewrite == "gpu")
    _check_file(out, uneven["recs"], dealt, uneven["header"])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["tagged.bam"]


@pytest.mark.parametrize("rewrite", ["cpu", "gpu"])
def test_writer_with_the_device_coder_no_reads_at_all(gpu, uneven, tmp_path, monkeypatch, rewrite):
    monkeypatch.setenv("TBK_HAPLOTAG_REWRITE", rewrite)
    out = str(tmp_path / "tagged.bam")
    dealt, coder_on_device, _ = write_tagged(uneven["none"], out, deal_pattern, device=0)
    assert coder_on_device and dealt == []
    with open(out, "rb") as fh:
        payloads = bb.walk(fh.read())
    assert b"".join(payloads) == uneven["header"] and payloads[-1] == b""   # header plus marker


def test_writer_refusal_names_the_record_in_the_output(gpu, uneven, tmp_path, monkeypatch):
    """a record the rule refuses in the third batch: its number counts the records written before it"""
    from trio_binning_amd import seq

    monkeypatch.setenv("TBK_HAPLOTAG_REWRITE", "gpu")
    good = records_of("crafted")[0]
    bad = tr.refused_record(tr.refused()[16][1], name="twice")
    path = tmp_path / "bad.bam"
    path.write_bytes(bc.bgzf(bc.header() + b"".join(good[:7] + [bad] + good[7:9]), level=1))
    with pytest.raises(ValueError, match="BAM record 7: .*second tag field named HP"):
        write_tagged(str(path), str(tmp_path / "out.bam"), deal_pattern, device=0, limits=((0, 3),))


# ---- end to end ----
def _expected_counts(library, compressed):  # noqa: F811
    from trio_binning_amd import kmers

    lists = library["compressed_lists" if compressed else "lists"]
    reads = [bc.text_of(r).split(b"\n")[1].decode() for r in library["kept"]]
    if compressed:
        reads = [re.sub(r"(.)\1+", r"\1", s) for s in reads]
    ha, hb = kmers.HashSet.from_file(lists[0], 0), kmers.HashSet.from_file(lists[1], 0)
    with kmers.Classifier(ha, hb) as cls:
        bases, offsets = kmers.pack_reads(reads)
        return cls.classify_batch(bases, offsets)


@pytest.mark.parametrize("mode", ["plain", "compress"])
def test_classify_by_kmers_haplotag_output_end_to_end(gpu, library, capfd, tmp_path, mode):  # noqa: F811
    extra = ["--compress"] if mode == "compress" else []
    tsv_bins, bin_names = _run(library, capfd, tmp_path / "bins", extra)
    assert len(bin_names) == 3
    out = tmp_path / "tagged.bam"
    tsv, names = _run(library, capfd, tmp_path / "tagged", extra + ["--haplotag-output", str(out)])
    assert tsv == tsv_bins                       # the TSV has the same bytes as without the option
    assert names == []                           # no bin file appears
    header, records, _ = bb.read_bam_file(str(out))
    assert header == library["header"]
    lines = [line.split("\t") for line in tsv.splitlines()]
    assert [l[0] for l in lines] == [r["name"] for r in library["kept"]] and len(records) == len(lines)
    counts = _expected_counts(library, mode == "compress")
    assert {l[1] for l in lines} == set("ABU") and counts.sum() > 0
    for rec, r, line, (a, b) in zip(records, library["kept"], lines, counts.tolist()):
        tags = tr.tags_of(rec)
        assert tags.get(b"HP") == {"A": ("C", b"\x01"), "B": ("C", b"\x02"), "U": None}[line[1]]    # HP follows the TSV's bin
        assert tags[b"ka"] == ("I", struct.pack("<I", a)) and tags[b"kb"] == ("I", struct.pack("<I", b))
        assert rec == tr.retag(bc.encode(r), line[1], a, b)                                          # all other bytes are the input's


def test_native_loop_refuses_other_input(gpu, tmp_path):
    from trio_binning_amd import kmers

    data = os.path.join(ROOT, "tests", "data")
    ha, hb = kmers.HashSet.from_file(os.path.join(data, "hapA.txt"), 0), kmers.HashSet.from_file(os.path.join(data, "hapB.txt"), 0)
    with kmers.MultiClassifier(ha, hb, [0]) as cls:
        with pytest.raises(ValueError, match="needs BAM input"):
            cls.classify_file(os.path.join(data, "test.fastq"), 1, 1, (str(tmp_path / "t.bam"), "", ""), 3, -1, -1)
    assert not list(tmp_path.iterdir())
