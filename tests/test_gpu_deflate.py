"""The GPU gzip encoder of the bin writer (csrc/tbk_gdeflate.hip) against zlib: every member it writes must inflate to the
piece of text it was given - the reference's bins are read back through gzip (seq.py:86-92) and their DECOMPRESSED bytes are
the contract (seq.py:27-42,132-134; tests/test_classify_by_kmers.py:19-36), whichever encoder wrote them."""
import gzip
import hashlib
import os
import zlib
from unittest.mock import patch

import numpy as np
import pytest

from conftest import DATA, load_golden

pytestmark = pytest.mark.gpu


def fastq(rng, n_reads, length, qual):
    recs = []
    for i in range(n_reads):
        L = int(length if np.isscalar(length) else rng.integers(length[0], length[1]))
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
        if qual == "const":
            q = b"I" * L
        elif qual == "hifi":
            qv = np.clip(rng.normal(60, 15, L), 2, 93).astype(np.uint8)
            qv[rng.random(L) < 0.6] = 93
            q = (qv + 33).tobytes()
        else:
            q = (rng.integers(0, 4, L).astype(np.uint8) * 10 + 35).tobytes()   # binned
        recs.append(b"@read%d some comment\n" % i + seq + b"\n+\n" + q + b"\n")
    return b"".join(recs)


def check_members(pieces, members):
    assert len(members) == len(pieces)
    for i, (p, m) in enumerate(zip(pieces, members)):
        assert m[:4] == b"\x1f\x8b\x08\x00", i
        assert gzip.decompress(m) == p, (i, len(p), len(m))
        # one member, its trailer the piece's CRC-32 and length
        assert int.from_bytes(m[-8:-4], "little") == zlib.crc32(p) and int.from_bytes(m[-4:], "little") == len(p) & 0xFFFFFFFF
    # members back to back are one gzip file (what a bin is)
    assert gzip.decompress(b"".join(members)) == b"".join(pieces)


def test_members_inflate_to_their_text(gpu):
    from trio_binning_amd import seq

    rng = np.random.default_rng(11)
    pieces = [
        fastq(rng, 40, 15000, "hifi"),            # long lines: a block per line, bases and qualities coded apart
        fastq(rng, 40, 15000, "const"),           # runs: matches at distance 1
        fastq(rng, 3000, (50, 300), "binned"),    # short lines: 32 KiB blocks
        fastq(rng, 3, 200_000, "hifi"),           # lines longer than a block
        b"", b"A", b"\n", b"AB", b"A" * 100_000, bytes(range(256)) * 300,
        rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes(),        # noise: stored blocks
        bytes(rng.integers(0, 2, 70_000, dtype=np.uint8) * 255),         # two symbols
        (b">r\n" + b"ACGT" * 20 + b"\n") * 2000,                          # FASTA, very regular
        b"".join(bytes([65 + (i % 7)]) * (i % 300 + 1) for i in range(2000)),   # runs of every length up to 300
    ]
    # runs of one byte each, Fibonacci-like in length: the blocks are coded with runs, so what is counted is a literal and a few matches
    # per run and the trees are 7 and 4 levels deep - no length limit is reached (tests/test_gpu_deflate_limits.py reaches both)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    pieces.append(b"".join(bytes([33 + i]) * c for i, c in enumerate(fib))[:30000])
    # lengths around the 32-byte text word and the 8 KiB block (and its multiples), each starting at an odd offset in the job's text
    blob = fastq(rng, 40, 3000, "hifi")
    for L in (31, 32, 33, 8191, 8192, 8193, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537):
        at = sum(map(len, pieces))
        pieces.append(blob[7:7 + (3 if at % 2 == 0 else 2) + L % 5 * 2])   # (odd, whatever the lengths so far)
        assert (at + len(pieces[-1])) % 2 == 1
        o = int(rng.integers(0, len(blob) - L))
        pieces.append(blob[o:o + L])
    # FASTQ whose lines are 8190-8194 bytes with their newline: the block cutter decides right at a line end
    for L in (8189, 8190, 8191, 8192, 8193):
        pieces.append(fastq(rng, 6, L, "hifi"))
        pieces.append(fastq(rng, 6, L, "const"))
    members = seq.gzip_members_device(pieces)
    check_members(pieces, members)
    # the encoder shrinks what can be shrunk: 2 bits a base + the qualities' entropy, a few bits per 128-byte stretch of a run
    assert len(members[0]) < 0.50 * len(pieces[0]) and len(members[1]) < 0.16 * len(pieces[1])
    assert len(members[10]) < len(pieces[10]) + 5 * (len(pieces[10]) // 8192 + 2) + 64   # noise does not grow beyond the stored blocks' headers


@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_DEFLATE_FUZZ_SEEDS", "6"))))   # (a soak run: TBK_DEFLATE_FUZZ_SEEDS=400)
def test_fuzz_against_zlib(gpu, seed):
    from trio_binning_amd import seq

    rng = np.random.default_rng(1000 + seed)
    pieces = []
    for _ in range(60):
        kind = int(rng.integers(0, 6))
        n = int(rng.integers(1, 300_000)) if rng.random() < 0.8 else int(rng.integers(1, 40))
        if kind == 0:
            p = fastq(rng, max(1, n // 3000), (10, 6000), ["hifi", "const", "binned"][int(rng.integers(0, 3))])
        elif kind == 1:
            alphabet = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)
            p = alphabet[rng.integers(0, alphabet.size, n)].tobytes()
        elif kind == 2:
            runs = rng.integers(1, 600, max(1, n // 100))
            vals = rng.integers(0, 256, runs.size, dtype=np.uint8)
            p = np.repeat(vals, runs).tobytes()
        elif kind == 3:
            w = 2.0 ** -np.arange(int(rng.integers(2, 60)))
            p = rng.choice(np.arange(w.size, dtype=np.uint8) + 40, size=n, p=w / w.sum()).tobytes()
        elif kind == 4:
            line = int(rng.integers(1, 5000))
            body = rng.integers(65, 91, n, dtype=np.uint8)
            body[line::line + 1] = 10
            p = body.tobytes()
        else:
            p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        pieces.append(p)
    check_members(pieces, seq.gzip_members_device(pieces))


def test_a_gigabyte_of_fastq(gpu):
    """1 GB through the encoder in jobs of 128 members of 1 MiB, as the bin writer cuts them: sha256 of the inflated stream."""
    from trio_binning_amd import seq

    rng = np.random.default_rng(5)
    base = fastq(rng, 4600, 15000, "hifi")   # ~138 MB
    want, got = hashlib.sha256(), hashlib.sha256()
    total = 0
    for rep in range(8):
        text = base[rep * 1000:] + base[:rep * 1000]
        pieces = [text[i:i + (1 << 20)] for i in range(0, len(text), 1 << 20)]
        members = seq.gzip_members_device(pieces)
        d = zlib.decompressobj(31)
        for m in members:
            out = zlib.decompressobj(31).decompress(m)
            got.update(out)
        want.update(text)
        total += len(text)
    assert total > 1e9 and got.hexdigest() == want.hexdigest()


@pytest.mark.parametrize("encoder", ["gpu", "cpu"])
def test_cli_bins_through_either_encoder(gpu, capsys, tmp_path, monkeypatch, encoder):
    """classify-by-kmers with gzip'ed bins (the reference's default): the decompressed bins and the TSV equal the reference's
    recorded output whether the device or the host coded the members; TBK_STATS says which it was."""
    import trio_binning_amd.classify_by_kmers as cbk

    v = next(x for x in load_golden("diff_vectors.json") if x["k"] == 21)
    fa, fb = tmp_path / "la.txt", tmp_path / "lb.txt"
    fa.write_text("".join(x + "\n" for x in v["list_a"]))
    fb.write_text("".join(x + "\n" for x in v["list_b"]))
    fq = tmp_path / "reads21.fa"
    with open(fq, "w") as fh:
        for i, s in enumerate(v["reads"]):
            fh.write(f">r{i} some comment\n{s}\n")
    monkeypatch.setenv("TBK_GZIP_ENCODER", encoder)
    monkeypatch.setenv("TBK_STATS", "1")
    monkeypatch.setattr(cbk, "_BATCH_BASES", 300)
    monkeypatch.setattr(cbk, "_BATCH_READS", 5)     # (dozens of flushes: the three-deep job ring turns over many times)
    od = tmp_path / "out"
    od.mkdir()
    with patch("sys.argv", ["classify-by-kmers", str(fq), str(fa), str(fb), "--haplotype-a-out-prefix", str(od / "hapA"),
                            "--haplotype-b-out-prefix", str(od / "hapB"), "--unclassified-out-prefix", str(od / "unclassified")]):
        cbk.main()
    out, err = capsys.readouterr()
    assert out == v["cli_stdout"]
    for fn, digest in v["cli_bins"].items():
        assert hashlib.sha256(gzip.open(od / fn, "rb").read()).hexdigest() == digest, fn
    assert ('"gzip_encoder": "%s"' % ("device" if encoder == "gpu" else "host")) in err, err[-600:]


def test_bin_writer_on_the_device_equals_the_python_writer(gpu, tmp_path):
    """seq.BinWriter(..., device=0): the three bins' gzip members coded on the GPU, many small batches (the job ring turns over, the
    bins' text changes buffers at every flush, members of 1 MiB are cut across batches), FASTQ and FASTA records mixed - the
    decompressed bins equal what the Python mirror of seq.py:27-42,98-136 writes; an empty bin is a valid empty gzip file."""
    import random

    from trio_binning_amd import seq

    rng = random.Random(19)
    recs = []
    for i in range(6000):
        n = rng.randrange(0, 2500)
        s = "".join(rng.choice("ACGT") for _ in range(n))
        kind = rng.random()
        q = None if kind < 0.3 else ("" if kind < 0.35 else "".join(rng.choice("!#5I~") for _ in range(n)))
        recs.append(seq.Read(f"read{i}/x", s, q))
    src = tmp_path / "in.fq"
    with open(src, "w") as fh:
        for r in recs:
            r.print(file=fh)
    for trial, letters in enumerate(("ABU", "AB")):   # (second trial: the unclassified bin stays empty)
        bins_all = "".join(rng.choice(letters) for _ in recs)
        outs = seq.open_outfiles(str(tmp_path / f"pa{trial}"), str(tmp_path / f"pb{trial}"), str(tmp_path / f"pu{trial}"), ".fq", True)
        parsed = list(seq.open_fastx_read(str(src)))
        for r, b in zip(parsed, bins_all):
            r.print(file=outs["ABU".index(b)])
        for fh in outs:
            fh.close()
        w = seq.BinWriter(str(tmp_path / f"na{trial}"), str(tmp_path / f"nb{trial}"), str(tmp_path / f"nu{trial}"), ".fq", True, device=0)
        assert w.gpu_encoder
        got_n = 0
        with seq.BatchReader(str(src)) as r:
            b = seq.Batch()
            while r.next_batch(b, 200_000, 0):
                w.write(b, bins_all[got_n:got_n + b.n_reads].encode())
                got_n += b.n_reads
        w.close()
        assert got_n == len(parsed)
        for py_name, nat_name in zip(seq.output_names(str(tmp_path / f"pa{trial}"), str(tmp_path / f"pb{trial}"), str(tmp_path / f"pu{trial}"), ".fq", True), w.names):
            assert gzip.open(nat_name, "rb").read() == gzip.open(py_name, "rb").read(), nat_name


# ---- the ring around the encoder: uneven flushes, sinks that fall behind or go away ------------------------------------------------
# The bin writer's device path (tbk_fastx.cpp, flush_bins_gpu) keeps three jobs in flight; a collected job's members are written by
# one thread per bin (the lanes) straight from the job's pinned buffer, and that buffer is the one the job three submits later uses
# (and grows, when it needs more room).  Bins that are FIFOs drained slowly keep the lanes behind the writer.

def _uneven_records(rng, seq):
    """~32 Mbases of FASTQ (and some FASTA) records: log-normal lengths, a few of 2-4 MB (longer than a 1 MiB member: members are
    cut inside them and what is left over moves across the text buffers' swap), and a run of ordinary ones first."""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = np.clip(rng.lognormal(np.log(6000), 0.7, 3400), 0, 80_000).astype(np.int64)
    lens[rng.random(lens.size) < 0.01] = 0
    long_at = {900: 2_100_000, 1400: 3_900_000, 2300: 2_700_000, 3000: 3_300_000}
    recs = []
    for i, L in enumerate(lens):
        L = long_at.get(i, int(L))
        s = lut[rng.integers(0, 4, L)].tobytes().decode()
        if i % 23 == 5:
            q = None
        else:
            qv = np.clip(rng.normal(60, 15, L), 2, 93).astype(np.uint8)
            qv[rng.random(L) < 0.6] = 93
            q = (qv + 33).tobytes().decode()
        recs.append(seq.Read(f"r{i}/ccs", s, q))
    return recs


# (max_bases per batch, which bins its records go to): four whole batches of ~3 MB of text to one bin each (every one a job of two
# members: the slots' first buffers), then ~12 MB (slot 1 must grow while the lanes still write job 1), two small ones that code
# nothing for A, ~30 MB all to A (growing again), then the rest in 2 Mbase batches; U stays empty throughout
_UNEVEN = [(1_500_000, "A"), (1_500_000, "B"), (1_500_000, "A"), (1_500_000, "B"), (6_000_000, "ab"), (150_000, "B"), (150_000, "B"),
           (15_000_000, "A")]


def _uneven_letters(bi, n):
    how = _UNEVEN[bi][1] if bi < len(_UNEVEN) else "ab"
    if how in ("A", "B"):
        return how * n
    r = np.random.default_rng(500 + bi)
    return "".join(np.where(r.random(n) < 0.7, "A", "B"))


def _write_uneven(seq, src, prefixes):
    """The records of `src` through seq.BinWriter(device=0) in the batches of _UNEVEN; returns the bins' letters, record by record."""
    w = seq.BinWriter(*prefixes, ".fq", True, device=0)
    letters = []
    try:
        assert w.gpu_encoder
        with seq.BatchReader(str(src)) as r:
            b = seq.Batch()
            bi = 0
            while r.next_batch(b, _UNEVEN[bi][0] if bi < len(_UNEVEN) else 2_000_000, 0):
                x = _uneven_letters(bi, b.n_reads)
                w.write(b, x.encode())
                letters.append(x)
                bi += 1
        assert bi > len(_UNEVEN)
    finally:
        w.close()
    return "".join(letters)


class _SlowDrains:
    """A reader thread per FIFO that takes `chunk` bytes every `pause` seconds (`stop_after`: closes its end after that many bytes).
    Whatever happens to the test, `finish()` lets the threads read at full speed, unblocks any still waiting for a writer and joins
    them with a time limit."""

    def __init__(self, paths, chunk=16 << 10, pause=0.005, stop_after=None):
        import threading

        self.paths, self.got, self.errors = list(paths), {}, []
        self.hurry = threading.Event()
        self.opened = [threading.Event() for _ in self.paths]
        self.threads = []
        for i, p in enumerate(self.paths):
            os.mkfifo(p)
            t = threading.Thread(target=self._drain, args=(i, chunk, pause, (stop_after or {}).get(i)), daemon=True)
            t.start()
            self.threads.append(t)

    def _drain(self, i, chunk, pause, stop_after):
        buf = bytearray()
        try:
            with open(self.paths[i], "rb", buffering=0) as fh:
                self.opened[i].set()
                while stop_after is None or len(buf) < stop_after:
                    piece = fh.read(chunk)
                    if not piece:
                        break
                    buf += piece
                    self.hurry.wait(pause)
        except Exception as e:  # noqa: BLE001  (reported by finish())
            self.errors.append(e)
        self.got[i] = bytes(buf)

    def finish(self, limit=60):
        self.hurry.set()
        for i, p in enumerate(self.paths):
            if not self.opened[i].is_set():   # (the writer never opened this one: a writer end of our own lets the reader go)
                try:
                    os.close(os.open(p, os.O_WRONLY | os.O_NONBLOCK))
                except OSError:
                    pass
        for t in self.threads:
            t.join(limit)
        assert not any(t.is_alive() for t in self.threads), "a drain thread did not end"
        assert not self.errors, self.errors


def _python_bins(seq, tmp_path, src, letters, tag):
    """What the Python mirror of the reference's writer (seq.open_outfiles + Read.print) puts in each bin, as text."""
    names = [str(tmp_path / f"{tag}{x}") for x in ("a", "b", "u")]
    outs = seq.open_outfiles(*names, ".fq", False)
    n = 0
    for r, c in zip(seq.open_fastx_read(str(src)), letters):
        r.print(file=outs["ABU".index(c)])
        n += 1
    for fh in outs:
        fh.close()
    assert n == len(letters)
    return [open(nm, "rb").read() for nm in seq.output_names(*names, ".fq", False)]


def test_uneven_flushes_into_slow_fifos(gpu, tmp_path):
    """Bins that are FIFOs read slowly (16 KiB every 5 ms), fed by flushes of very different sizes: a job slot must grow while the lanes
    still write the members collected from it.  Each bin's decompressed stream equals the Python mirror's bytes; then the same
    sequence into regular files, the control."""
    from trio_binning_amd import seq

    recs = _uneven_records(np.random.default_rng(23), seq)
    src = tmp_path / "in.fq"
    with open(src, "w") as fh:
        for r in recs:
            r.print(file=fh)
    del recs
    prefixes = [str(tmp_path / f"f{x}") for x in ("a", "b", "u")]
    drains = _SlowDrains(seq.output_names(*prefixes, ".fq", True))
    try:
        letters = _write_uneven(seq, src, prefixes)
    finally:
        drains.finish()
    assert "U" not in letters and letters.count("A") > 100 and letters.count("B") > 100
    want = _python_bins(seq, tmp_path, src, letters, "p")
    assert want[2] == b"" and len(want[0]) > 30_000_000
    for i in range(3):
        assert gzip.decompress(drains.got[i]) == want[i], "ABU"[i]
    control = [str(tmp_path / f"c{x}") for x in ("a", "b", "u")]
    assert _write_uneven(seq, src, control) == letters
    for i, nm in enumerate(seq.output_names(*control, ".fq", True)):
        assert gzip.open(nm, "rb").read() == want[i], nm


def test_a_sink_that_goes_away_fails_the_writer(gpu, tmp_path):
    """The reader of bin B closes its end after ~200 kB: the lane's write gets EPIPE (Python ignores SIGPIPE), and BinWriter.write or
    close raises the library's I/O error (OSError) naming it - promptly, with nothing hanging; the device is left usable (a later
    job round-trips)."""
    import time

    from trio_binning_amd import seq

    recs = _uneven_records(np.random.default_rng(29), seq)[:2000]
    src = tmp_path / "in.fq"
    with open(src, "w") as fh:
        for r in recs:
            r.print(file=fh)
    prefixes = [str(tmp_path / f"f{x}") for x in ("a", "b", "u")]
    drains = _SlowDrains(seq.output_names(*prefixes, ".fq", True), pause=0.001, stop_after={1: 200_000})
    failed, w = None, None
    t0 = time.monotonic()
    try:
        w = seq.BinWriter(*prefixes, ".fq", True, device=0)
        assert w.gpu_encoder
        try:
            with seq.BatchReader(str(src)) as r:
                b = seq.Batch()
                while r.next_batch(b, 1_000_000, 0):
                    w.write(b, ("AB" * b.n_reads)[:b.n_reads].encode())
        except OSError as e:
            failed = e
        t1 = time.monotonic()
        try:
            w.close()
        except OSError as e:
            failed = failed or e
        assert time.monotonic() - t1 < 30, "close() took too long"
    finally:
        if w is not None:   # (the readers see the end of their FIFOs only once the writer has closed them)
            try:
                w.close()
            except OSError:
                pass
        drains.finish()
    assert failed is not None, "the writer returned as if the bin had been written"
    assert "write" in str(failed) and "Broken pipe" in str(failed), str(failed)
    assert time.monotonic() - t0 < 120
    assert len(drains.got[1]) >= 200_000
    pieces = [b"@x\nACGT\n+\nIIII\n" * 5000, b"", bytes(range(256)) * 100]
    check_members(pieces, seq.gzip_members_device(pieces))
