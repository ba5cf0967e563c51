"""The GPU inflater for ordinary gzip input (csrc/tbk_gdeflate.hip, last part: gz_inflate_kernel, gz_propagate_kernel,
gz_resolve_kernel, gd_crc_kernel) on the files of tests/gzip_shapes.py, which reach what zlib's default streams of FASTQ do not:
windows carried through chains of short chunks, markers at both ends of the window and copies out of markers, stored and fixed blocks
and blocks without symbols in chunks that do not know their window, flushed streams, block headers that are none, 300 members, a
chunk that runs out of room behind chunk 0, and references before a member's first byte that only the resolved markers show.

Three checks.  The text is gzip's, and what gzip refuses is refused, never returned.  The device's pass a agrees with the host's
decoder chunk by chunk: plan and chain check are shared code, so the run's windows, guessed, accepted, redecoded and most_accepted
equal those of seq.gzip_inflate_host on the same bytes, computed here (a kernel that is right but refuses chunks shows here, not in the
text) - on the refused files as on the valid ones: the stats of a refusal are those of the run up to it, so a device that refuses
in another window or behind other chunks than the host's decoder shows.  (A member cut in its trailer is "done" to either pass a,
and the loop finds the trailer cut.)  One difference is legitimate: a chunk behind a broken one is SKIPPED on the device while the host decodes it and may find it
without room, which moves the loop's ratio - on the decoy and the high-ratio cases the stats are printed and only `accepted` per
window is held.  And the reader gives the plain file's records from such files at 1024-byte chunks and windows.

Nothing here is meant to fault and nothing is tried twice: the refusals are ordinary ones under the decoder's fuel and bounds checks,
and every file has been through the host stand-in (tests/test_host_gzip_shapes.py) first.

Held against scratch mutants of the kernels on an MI355X, one at a time, each once: propagate's before[take + k] as before[k];
propagate resolving through src; src[i % dist] as src[i]; the marker fill from 0x8000 + i + 1 (these four fail short:zblock_l1, the
first case); resolve's v >= 0x8000 as v > 0x8000 and dist > TBK_GZ_HIST as >= (both fail extremes:far_end_first and nothing before
it); the stored block's b.p -= b.cnt >> 3 dropped (fails short:sync).  `if (seen > 0xFF) bad[ci] = 1` dropped SURVIVED the first
form of the far-back files: their trailers said the CRC-32 of 0xFF for all three copied bytes, but only the first of the three lies
before the member, so the mutant's text missed the CRC and was refused all the same.  The trailers now say 0xFF for that one byte
and the text for the other two: the text the mutant returns, which only `bad` refuses (refused:far_back_*;
tests/gzip_shapes.py checks it: zlib, given that one byte as a dictionary, inflates the member to its trailer's CRC-32 and size).
That form has not been run against the mutant on a device.

Not covered: members above 4 GiB (ISIZE wraps), the clamp of a window at max_symbols (3 * 2^29 elements), and DEFLATE blocks longer
than the 1 MiB of input kept behind a window (zlib writes none, and a hand-built one is minutes of pure Python)."""
import time

import pytest

import gzip_shapes as gs
from test_host_gzip_shapes import STAT_KEYS, host_stats

pytestmark = pytest.mark.gpu

LOOSE = ("decoy", "ratio")   # groups whose stats may differ from the host's by skipped chunks (see above)


def _device_run(case):
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    _, blob, chunk, window, _ = case
    t0 = time.perf_counter()
    try:
        got = seq.gzip_inflate_device(blob, chunk=chunk, window=window)
    except (TbkError, ValueError, OSError):
        got = gs.REFUSED
    return got, seq.gzip_inflate_stats(), time.perf_counter() - t0


@pytest.mark.parametrize("name", gs.NAMES)
def test_text_and_stats(gpu, name):
    case = gs.case(name)
    expect = case[4]
    want = host_stats(case)
    got, st, seconds = _device_run(case)
    print("%s: %d bytes, device %.3f s %s, host %s" % (name, len(case[1]), seconds, st, want))
    if expect is gs.REFUSED:
        assert got is gs.REFUSED, name
    else:
        assert got is not gs.REFUSED, name
        assert got == expect, name
    assert st["handed_back"] == 0, st
    if gs.group(name) in LOOSE:
        assert st["accepted"] >= st["windows"] >= 1, st
    else:
        assert {k: st[k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}, name
    planned = gs.min_accepted()
    if name in planned:
        assert st["accepted"] >= planned[name], (st, planned[name])


def _batch_records(b):
    """(name, sequence, quality) of a batch's records as bytes: one of the files holds records that are no text."""
    bases, boff, names, noff, quals, qoff, hq = b.arrays()
    cut = lambda a, off, i: bytes(a[int(off[i]):int(off[i + 1])])
    return [(cut(names, noff, i), cut(bases, boff, i), cut(quals, qoff, i) if hq[i] else None) for i in range(b.n_reads)]


def _records(path, **kw):
    from trio_binning_amd import seq

    out = []
    with seq.BatchReader(str(path), **kw) as r:
        on_device, b = r.inflates_on_device, seq.Batch()
        while r.next_batch(b, 3 << 20, 0):
            out += _batch_records(b)
        stats = r.gzip_stats()
    return out, on_device, stats


def _reader_env(monkeypatch):
    monkeypatch.setenv("TBK_GZIP_INFLATE", "gpu")
    monkeypatch.setenv("TBK_PINFLATE_MIN", "0")
    monkeypatch.setenv("TBK_GZIP_CHUNK", "1024")
    monkeypatch.setenv("TBK_GZIP_WINDOW", "1024")


@pytest.mark.parametrize("name", ["short:zblock_l6", "storedfixed:fastq_and_noise"])
def test_reader_at_small_chunks_and_windows(gpu, name, tmp_path, monkeypatch):
    """BatchReader(path, device=0) at 1024-byte chunks and windows: the plain file's records, inflated on the device, over as many
    windows as the host stand-in makes of the file at that size - each of one chunk, which carries its window on."""
    _reader_env(monkeypatch)
    _, blob, _, _, text = gs.case(name)
    want_stats = host_stats((name, blob, 1024, 1024, text))
    plain, packed = tmp_path / "r.fastq", tmp_path / "r.fastq.gz"
    plain.write_bytes(text)
    packed.write_bytes(blob)
    want, _, _ = _records(plain)
    assert len(want) >= 50
    got, on_device, st = _records(packed, device=0)
    print(name, st)
    assert on_device and got == want
    assert st["handed_back"] == 0 and {k: st[k] for k in STAT_KEYS} == {k: want_stats[k] for k in STAT_KEYS}, (st, want_stats)
    assert st["windows"] >= 50 and st["most_accepted"] == 1, st   # (a window of 1024 bytes is one chunk; 50: tests/test_host_gzip_shapes.py)


def test_reader_refuses_what_the_inflater_refuses(gpu, tmp_path, monkeypatch):
    """A reference before the second member's first byte, nine chunks into it: the reader raises; what it gave before is a prefix of
    the records in front of the damage, and nothing comes after the error."""
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    _reader_env(monkeypatch)
    _, blob, _, _, _ = gs.case("refused:far_back_9_chunks_in")
    text = gs.far_back_text(9)
    plain, packed = tmp_path / "r.fastq", tmp_path / "r.fastq.gz"
    plain.write_bytes(text[:text.index(b"@late\n")])
    packed.write_bytes(blob)
    want, _, _ = _records(plain)
    got = []
    with seq.BatchReader(str(packed), device=0) as r:
        assert r.inflates_on_device
        b = seq.Batch()
        with pytest.raises((TbkError, ValueError, OSError)):
            while r.next_batch(b, 1 << 20, 0):
                got += _batch_records(b)
        try:
            more = r.next_batch(b, 1 << 20, 0)
        except (TbkError, ValueError, OSError):
            more = False
        assert not more
    assert len(got) <= len(want) and got == want[:len(got)]
