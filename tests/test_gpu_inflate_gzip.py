"""The GPU inflater for ordinary gzip input (csrc/tbk_gdeflate.hip, last part: marker-mode inflate, window propagation, resolve,
CRC-32; csrc/tbk_gzplan.cpp: the plan and the chain check) against gzip.decompress: one member or several, any header fields, any
block types - byte for byte, at the default chunk size and at small ones; damage refused, never returned; the parallel path is what
ran; and the reader and classify-by-kmers on such a file give the plain file's records and the reference's recorded output.

The raw-entry tests' inputs and expectations hold with the host's decoder in the device's place (seq.gzip_inflate_host; the same plan,
chain check and loop - tests/test_host_gzip_plan.py runs that without a device)."""
import gzip
import hashlib
import zlib

import numpy as np
import pytest

import deflate_craft as dc
from test_gpu_inflate import fastq
from test_host_gzip_plan import big_text, member

pytestmark = pytest.mark.gpu

CHUNKS = (None, 4096, 70_000)   # compressed bytes per chunk: the default, and two that cut the small inputs too


@pytest.fixture(scope="module")
def text():
    return big_text()


def _refused(call):
    from trio_binning_amd._lib import TbkError

    try:
        call()
    except (TbkError, ValueError, OSError):
        return True
    return False


def test_text_equals_zlibs(gpu, text):
    from trio_binning_amd import seq

    rng = np.random.default_rng(3)
    texts = {
        "hifi": fastq(rng, 60, 15000),
        "const": fastq(rng, 60, 15000, "const"),
        "short reads": fastq(rng, 5000, 150),
        "noise": rng.integers(0, 256, 300_000, dtype=np.uint8).tobytes(),
        "skewed": rng.choice(np.arange(200, dtype=np.uint8), size=400_000, p=(lambda w: w / w.sum())(1.5 ** -np.arange(200))).tobytes(),
        "periodic": (b"ACGTTGCA" * 7 + b"\n") * 8000,
        "one byte": b"x",
        "empty": b"",
        "27 MB": text,
    }
    for name, t in texts.items():
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (4, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            data = member(t, level, strategy)
            assert gzip.decompress(data) == t
            for chunk in CHUNKS:
                assert seq.gzip_inflate_device(data, chunk=chunk) == t, (name, level, strategy, chunk)
                if chunk is None:
                    assert seq.gzip_inflate_stats()["handed_back"] == 0, (name, level, strategy)


def test_framing(gpu, text):
    """Members of uneven size, a stored member in front, fixed blocks, zero padding between members, an empty member, every optional
    header field, a member whose final block is stored."""
    from trio_binning_amd import seq

    third = len(text) // 3
    small = text[:300_000]
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = raw.compress(small) + raw.flush(zlib.Z_FULL_FLUSH)   # ends on a byte boundary, not final
    stored_last = body + b"\x01\x05\x00\xfa\xff" + b"tail\n"
    files = {
        "members": member(text[:third], 6) + member(text[third:third + 100], 9) + member(text[third + 100:], 1),
        "stored_first": member(text[:third], 0) + b"\0" * 5 + member(text[third:], 6),
        "fixed_blocks": member(text[:third], 6, zlib.Z_FIXED) + member(text[third:], 6),
        "empty member": member(small, 6) + member(b"", 6) + b"\0" * 3 + member(small[::-1], 1) + member(b"", 0),
        "header fields": dc.member(body + b"\x03\x00", small, bgzf=False, fname=b"reads.fq", fcomment=b"a comment", fhcrc=True)
                         + dc.member(body + b"\x03\x00", small, bgzf=False, fname=b"x") + dc.member(body + b"\x03\x00", small, bgzf=False, fhcrc=True),
        "fextra": b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x05\x00XY\x01\x00z" + member(small, 6)[10:],
        "stored final block": dc.member(stored_last, small + b"tail\n", bgzf=False),
    }
    for name, data in files.items():
        want = gzip.decompress(data)
        for chunk in CHUNKS:
            assert seq.gzip_inflate_device(data, chunk=chunk) == want, (name, chunk)
            if chunk is None:
                assert seq.gzip_inflate_stats()["handed_back"] == 0, name


def test_crafted_streams(gpu):
    """Every hand-built valid stream as an ordinary member, alone and all concatenated; every invalid one refused where gzip refuses."""
    from trio_binning_amd import seq

    valid = dc.valid_streams()
    blobs = [dc.member(r, t, bgzf=False) for _, t, r in valid]
    for (name, t, _), blob in zip(valid, blobs):
        assert gzip.decompress(blob) == t
        assert seq.gzip_inflate_device(blob) == t, name
        assert seq.gzip_inflate_stats()["handed_back"] == 0, name
    whole = b"".join(blobs)
    for chunk in CHUNKS:
        assert seq.gzip_inflate_device(whole, chunk=chunk) == gzip.decompress(whole), chunk
    for name, t, raw, kw in dc.invalid_streams():
        blob = blobs[0] + dc.member(raw, t, bgzf=False, **kw) + blobs[1]
        with pytest.raises(Exception):
            gzip.decompress(blob)
        assert _refused(lambda: seq.gzip_inflate_device(blob)), name
    t, cut = dc.truncated_dynamic()
    blob = blobs[0] + dc.member(cut, t, bgzf=False)
    with pytest.raises(Exception):
        gzip.decompress(blob)
    assert _refused(lambda: seq.gzip_inflate_device(blob)), "cut in a dynamic header"


def _damaged(good):
    for kind in ("flip", "cut", "crc", "size"):
        blob = bytearray(good)
        if kind == "flip":
            blob[len(blob) * 3 // 4] ^= 0x10
        elif kind == "cut":
            blob = blob[: len(blob) * 2 // 3]
        elif kind == "crc":
            blob[-8] ^= 1
        else:
            blob[-1] ^= 1
        yield kind, bytes(blob)


def _records(path, **kw):
    from trio_binning_amd import seq

    out = []
    with seq.BatchReader(str(path), **kw) as r:
        on_device, b = r.inflates_on_device, seq.Batch()
        while r.next_batch(b, 3 << 20, 0):
            out += [(x.name, x.seq, x.qual) for x in b.reads()]
        stats = r.gzip_stats()
    return out, on_device, stats


def test_damage_is_refused_never_returned(gpu, text, tmp_path, monkeypatch):
    """A flipped bit at 3/4 of the file, the file cut at 2/3, a CRC byte, an ISIZE byte: each raises, through the raw entry and through
    the reader.  (Refusals under the decoder's fuel bound: nothing here is meant to fault, and nothing is tried twice.)"""
    from trio_binning_amd import seq

    monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
    monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")
    for kind, blob in _damaged(member(text, 6)):
        assert _refused(lambda: seq.gzip_inflate_device(blob)), kind
        assert _refused(lambda: seq.gzip_inflate_device(blob, chunk=200_000, window=2_000_000)), kind
        f = tmp_path / f"{kind}.fastq.gz"
        f.write_bytes(blob)
        assert _refused(lambda: _records(f, device=0)), kind


def test_the_parallel_path_is_what_ran(gpu, text):
    """200 000-byte chunks, windows of ten of them: at least three windows, some window with four chunks kept or more, and at least
    0.8 of all chunks decoded kept (the host test's share for this stream and span: the guesser and the chain rule are the host's)."""
    from trio_binning_amd import seq

    data = member(text, 6)
    assert seq.gzip_inflate_device(data, chunk=200_000, window=2_000_000) == text
    st = seq.gzip_inflate_stats()
    print("27 MB level 6, 200000-byte chunks, 2 MB windows:", st)
    assert st["guessed"] + st["windows"] <= 32 * st["windows"], st   # (no window of more than 32 chunks)
    assert st["windows"] >= 3 and st["most_accepted"] >= 4, st
    assert st["accepted"] >= 0.8 * (st["guessed"] + st["windows"]), st
    assert st["handed_back"] == 0, st


def test_reader_on_the_device(gpu, text, tmp_path, monkeypatch):
    """BatchReader(path, device=0) on an ordinary .fastq.gz: the plain file's records with inflates_on_device true - at levels 1, 6, 9,
    over many small windows, with packing and borrowing (batches kept beyond the reader); TBK_GZIP_INFLATE=cpu keeps the host path."""
    from trio_binning_amd import seq

    monkeypatch.setenv("TBK_PINFLATE_MIN", "0")   # (these files are under the 16 MB default)
    monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")
    plain = tmp_path / "r.fastq"
    plain.write_bytes(text)
    want, _, _ = _records(plain)
    assert len(want) == 1500
    for level in (1, 6, 9):
        f = tmp_path / f"l{level}.fastq.gz"
        f.write_bytes(member(text, level))
        got, on_device, st = _records(f, device=0)
        assert on_device and got == want, level
        assert st["windows"] >= 1 and st["handed_back"] == 0 and st["accepted"] > 1, st
        monkeypatch.setenv("TBK_GZIP_CHUNK", "100000")
        monkeypatch.setenv("TBK_GZIP_WINDOW", "1000000")
        got, on_device, st = _records(f, device=0)
        assert on_device and got == want and st["windows"] >= 10, (level, st)
        with seq.BatchReader(str(f), packing=True, borrowing=True, device=0) as r:
            kept = []
            while True:
                b = seq.Batch()
                if not r.next_batch(b, 3 << 20, 0):
                    break
                kept.append(b)
        assert [(x.name, x.seq, x.qual) for b in kept for x in b.reads()] == want, level   # (the reader is closed)
        del kept
        monkeypatch.delenv("TBK_GZIP_CHUNK")
        monkeypatch.delenv("TBK_GZIP_WINDOW")
        monkeypatch.setenv("TBK_GZIP_INFLATE", "cpu")
        got, on_device, st = _records(f, device=0)
        assert not on_device and got == want and st["windows"] == 0, level
        monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")


def test_cli_from_ordinary_gzip_on_the_device(gpu, capfd, tmp_path, monkeypatch):
    """classify-by-kmers on a gzip.compress'ed copy of the golden k = 21 reads writes the reference's recorded TSV and bins, on one ring
    and on two; and it reads the reference's own tests/data/test.ccs.fastq.gz on the device as on the host."""
    from unittest.mock import patch

    import trio_binning_amd.classify_by_kmers as cbk
    from conftest import DATA, load_golden

    monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
    monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")
    v = next(x for x in load_golden("diff_vectors.json") if x["k"] == 21)
    fa, fb = tmp_path / "la.txt", tmp_path / "lb.txt"
    fa.write_text("".join(x + "\n" for x in v["list_a"]))
    fb.write_text("".join(x + "\n" for x in v["list_b"]))
    fq = tmp_path / "reads21.fa.gz"
    fq.write_bytes(gzip.compress("".join(f">r{i} some comment\n{s}\n" for i, s in enumerate(v["reads"])).encode()))
    monkeypatch.setenv("TBK_GZIP_CHUNK", "2048")
    monkeypatch.setattr(cbk, "_BATCH_BASES", 3000)
    monkeypatch.setattr(cbk, "_BATCH_READS", 20)

    def run(reads, od):
        od.mkdir()
        with patch("sys.argv", ["classify-by-kmers", str(reads), str(fa), str(fb), "--haplotype-a-out-prefix", str(od / "hapA"),
                                "--haplotype-b-out-prefix", str(od / "hapB"), "--unclassified-out-prefix", str(od / "unclassified")]):
            cbk.main()
        out, _ = capfd.readouterr()
        return out, {p.name: hashlib.sha256(gzip.open(p, "rb").read()).hexdigest() for p in sorted(od.iterdir())}

    for devices in ("0", "0,0"):
        monkeypatch.setenv("TBK_DEVICES", devices)
        out, bins = run(fq, tmp_path / ("out" + devices.replace(",", "_")))
        assert out == v["cli_stdout"], devices
        for fn, digest in v["cli_bins"].items():
            assert bins[fn] == digest, (fn, devices)
        # the reference's own fixture: what the host path makes of it
        ccs = DATA + "/test.ccs.fastq.gz"
        got = run(ccs, tmp_path / ("ccs_gpu" + devices.replace(",", "_")))
        monkeypatch.setenv("TBK_GZIP_INFLATE", "cpu")
        want = run(ccs, tmp_path / ("ccs_cpu" + devices.replace(",", "_")))
        monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")
        assert got == want and got[0], devices
