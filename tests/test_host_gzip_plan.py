"""The GPU gzip inflater's host side, without a device (csrc/tbk_gzplan.cpp): the window plan (block-start guesses), the chain check
and the loop around them - members, trailers, retries - with the host's own decoder (TbkInflate::run16) standing in for the
device's marker-mode pass, as tests/test_multi_cpu.py stands stubs in for the rings.  What comes out must be gzip's text, and the
host path's refusals; TbkInflate's "position at bit" entry must go on exactly where a sequential decode stood."""
import ctypes as C
import gzip
import os
import re
import zlib

import numpy as np
import pytest

import deflate_craft as dc
from conftest import ROOT


def member(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    return co.compress(data) + co.flush()


def big_text():
    """The 27 MB stream of test_host_native_io.py::test_guessing_inflate_equals_the_sequential_decoder."""
    rng = np.random.default_rng(8)
    n, length = 1500, 9000
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, length))
    quals = (33 + np.clip(rng.normal(30, 8, (n, length)), 0, 60)).astype(np.uint8)
    parts = []
    for i in range(n):
        if i % 3 == 1:
            bases[i, : length // 2] = bases[i - 1, length // 4: length // 4 + length // 2]
        parts.append(b"@read%d/ccs np=%d\n" % (i, i % 17) + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n")
    return b"".join(parts)


@pytest.fixture(scope="module")
def text():
    return big_text()


def test_new_symbols_are_declared_as_built(built):
    """Every new entry of include/tbk.h exists in the library, with the declared parameters."""
    from trio_binning_amd._lib import lib

    header = open(os.path.join(ROOT, "include", "tbk.h")).read()
    want = {
        "tbk_gzip_inflate_device": r"int tbk_gzip_inflate_device\(int device, const uint8_t \*data, uint64_t size, uint8_t \*dst,\s*uint64_t cap, uint64_t \*text_len\);",
        "tbk_gzip_inflate_device_opts": r"int tbk_gzip_inflate_device_opts\(int device, const uint8_t \*data, uint64_t size, uint8_t \*dst, uint64_t cap, uint64_t \*text_len, uint64_t chunk,\s*uint64_t window\);",
        "tbk_gzip_inflate_host": r"int tbk_gzip_inflate_host\(const uint8_t \*data, uint64_t size, uint8_t \*dst, uint64_t cap, uint64_t \*text_len, uint64_t chunk, uint64_t window\);",
        "tbk_gzip_inflate_stats": r"void tbk_gzip_inflate_stats\(uint64_t out\[6\]\);",
        "tbk_gzip_inflate_bench_device": r"int tbk_gzip_inflate_bench_device\(int device, const uint8_t \*data, uint64_t size, int reps, double \*ring_s, double \*kernels_s, uint64_t \*text_bytes,\s*double pass_s\[3\]\);",
        "tbk_fastx_gzip_stats": r"void tbk_fastx_gzip_stats\(const tbk_fastx_reader \*r, uint64_t out\[6\]\);",
        "tbk_inflate_resume_at_bit": r"int tbk_inflate_resume_at_bit\(const uint8_t \*data, uint64_t size, uint64_t stop_bit, uint8_t \*dst, uint64_t cap, uint64_t \*text_len,\s*uint64_t \*boundary_bit\);",
    }
    for name, decl in want.items():
        assert hasattr(lib, name), name
        assert re.search(decl, header), name


def test_without_a_device_the_raw_entry_says_so(built):
    """An error code and a message, no crash: a device index that does not exist (whatever this machine has)."""
    from trio_binning_amd import _lib

    data = gzip.compress(b"ACGT" * 1000)
    n = C.c_uint64(7)
    buf = C.create_string_buffer(1 << 16)
    rc = _lib.lib.tbk_gzip_inflate_device(_lib.device_count() + 3, data, len(data), buf, len(buf), C.byref(n))
    assert rc == _lib.TBK_ERR_NO_DEVICE and n.value == 0
    assert b"no such device" in _lib.lib.tbk_last_error()
    assert _lib.lib.tbk_gzip_inflate_device(0, None, 5, buf, len(buf), C.byref(n)) == _lib.TBK_ERR_INVALID


def test_planner_and_chain_check_reproduce_the_text(built, text):
    """The `members` and `stored_first` files of the host test (and a one-member file) through plan, stand-in pass a, chain check,
    windows, resolve and CRC: gzip's text at several chunk sizes, over several windows; most guesses hold on the one-member stream."""
    from trio_binning_amd import seq

    third = len(text) // 3
    files = {
        "l6": member(text, 6),
        "members": member(text[:third], 6) + member(text[third:third + 100], 9) + member(text[third + 100:], 1),
        "stored_first": member(text[:third], 0) + b"\0" * 5 + member(text[third:], 6),
    }
    for name, blob in files.items():
        assert gzip.decompress(blob) == text
        for chunk, window in ((None, None), (70_000, None), (200_000, 2_000_000), (4096, 300_000)):
            assert seq.gzip_inflate_host(blob, chunk, window) == text, (name, chunk, window)
            st = seq.gzip_inflate_stats()
            assert st["handed_back"] == 0 and st["accepted"] >= 1, (name, st)
    # the condition the GPU test sets for this stream and span: the guesser and the chain rule are the host's own
    assert seq.gzip_inflate_host(files["l6"], 200_000, 2_000_000) == text
    st = seq.gzip_inflate_stats()
    print("l6, 200000-byte chunks, 2 MB windows:", st)
    assert st["windows"] >= 3 and st["most_accepted"] >= 4 and st["accepted"] >= 0.8 * (st["guessed"] + st["windows"]), st
    assert st["guessed"] + st["windows"] <= 32 * st["windows"]
    # small things: nothing to guess at.  (One byte, but not b"x": the reference's binding, run by an earlier test of this process,
    # writes through CPython's shared b"x" - see tests/test_gpu_integration.py.)
    for small in (b"", b"\n", b"A" * 3_000_000, text[:50_000]):
        for level in (0, 1, 9):
            assert seq.gzip_inflate_host(member(small, level)) == small
    assert seq.gzip_inflate_host(b"") == b""


def test_crafted_streams_and_framing_through_the_loop(built):
    """Hand-built streams as ordinary members, alone and concatenated, header fields and padding: gzip's text, gzip's refusals."""
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    valid = dc.valid_streams()
    blobs = [dc.member(r, t, bgzf=False) for _, t, r in valid]
    for (name, t, _), blob in zip(valid, blobs):
        assert seq.gzip_inflate_host(blob) == t, name
    whole = b"".join(blobs)
    assert seq.gzip_inflate_host(whole, 4096) == gzip.decompress(whole)
    framed = b"".join(dc.member(r, t, bgzf=False, fname=b"r.fq", fcomment=b"c", fhcrc=True) + b"\0" * (i % 4) for i, (_, t, r) in enumerate(valid[:8]))
    assert seq.gzip_inflate_host(framed) == gzip.decompress(framed)
    for name, t, raw, kw in dc.invalid_streams():
        kw = {k: v for k, v in kw.items() if k != "bgzf"}
        blob = blobs[0] + dc.member(raw, t, bgzf=False, **kw) + blobs[1]
        with pytest.raises(Exception):
            gzip.decompress(blob)
        with pytest.raises((TbkError, ValueError, OSError)):
            seq.gzip_inflate_host(blob)


def test_damage_is_refused(built, text):
    from trio_binning_amd import seq
    from trio_binning_amd._lib import TbkError

    good = member(text, 6)
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
        with pytest.raises((TbkError, ValueError, OSError)):
            seq.gzip_inflate_host(bytes(blob), 200_000, 2_000_000)


def test_position_at_bit_continues_a_sequential_decode(built, text):
    """A decoder told nothing but a bit - a block boundary a sequential decode reached - and the text so far goes on to the member's end
    with the same text: at boundaries all over the stream, through dynamic, fixed and stored blocks."""
    from trio_binning_amd import _lib

    part = text[:3_000_000]
    for level, strategy in ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
        blob = member(part, level, strategy)
        buf = C.create_string_buffer(len(part) + 16)
        seen = set()
        for frac in (0.0, 0.001, 0.13, 0.5, 0.77, 0.999):
            n, at = C.c_uint64(), C.c_uint64()
            stop = int(len(blob) * 8 * frac)
            _lib.check(_lib.lib.tbk_inflate_resume_at_bit(blob, len(blob), stop, buf, len(part) + 16, C.byref(n), C.byref(at)))
            assert C.string_at(C.addressof(buf), n.value) == part, (level, strategy, frac)
            assert at.value == 0 or at.value >= stop
            seen.add(at.value)
        if strategy == zlib.Z_DEFAULT_STRATEGY and level:
            assert len(seen) >= 5, seen   # (the decoder did take over in mid-stream)
