"""Ordinary gzip files built for the paths of the GPU gzip inflater (csrc/tbk_gzplan.cpp; csrc/tbk_gdeflate.hip, last part) that zlib's
default streams of FASTQ barely reach: chains of chunks shorter than the 32 KiB window, markers at the window's ends, stored and fixed
blocks inside marker-mode chunks, flushed streams, block headers that are none, hundreds of members, and streams that must be refused.
A helper like deflate_craft.py: pytest does not collect it.

``cases()`` returns a list of ``(name, gzip_bytes, chunk, window, expect)``: chunk / window are the compressed bytes per chunk / per
window to run the case at (None: the default), expect is the text (``gzip.decompress`` is the oracle and agrees: checked here) or
``REFUSED`` (``gzip.decompress`` raises: checked here).  The name's part before the colon is the case's group, which says what the
case must reach (tests/test_host_gzip_shapes.py asserts it from the host stand-in's stats); ``min_accepted()`` holds, for the hand-built
streams, the number of chunks their block positions plan - every one of which must be kept; ``refusal(name)`` says why a refused
file is refused and how many chunks a window keeps in front of the damage at the least.

Everything comes from zlib, numpy and deflate_craft with fixed seeds.  The hand-built parts are small (deflate_craft's writer and
greedy_tokens are pure Python).  Building all cases takes about 2 s on one core (half of it the hand-built streams, the rest zlib and the check against gzip.decompress).
"""
import functools
import gzip
import zlib

import numpy as np

import deflate_craft as dc
from deflate_craft import Block


class _Refused:
    def __repr__(self):
        return "REFUSED"


REFUSED = _Refused()
# what cases() learns on its way, behind min_accepted(), far_back_text() and refusal()
_MIN_ACCEPTED = {}
_FAR_BACK_TEXT = {}
_REFUSALS = {}

# every case's name, so that pytest can name the tests without building the files (cases() checks the list)
NAMES = tuple(["short:" + n for n in ("zblock_l1", "zblock_l6", "zblock_l9", "sync", "partial", "full", "mixed")]
              + ["short_w1024:" + n for n in ("zblock_l1", "zblock_l6", "zblock_l9", "mixed")]
              + ["extremes:" + n for n in ("far_end_first", "near_end_first", "chain", "chain_empty_1", "chain_empty_50")]
              + ["storedfixed:cycle", "storedfixed:fastq_and_noise", "decoy:whole_streams", "decoy:headers_and_noise", "members:300",
                 "ratio:periodic_after_fastq"]
              + ["refused:" + n for n in ("far_back_1_chunks_in", "far_back_3_chunks_in", "far_back_9_chunks_in", "bit_flip_in_a_late_chunk",
                                          "bit_flip_in_nlen", "cut_in_a_stored_block", "cut_in_a_dynamic_header", "cut_in_the_trailer_2_of_3",
                                          "trailer_2_of_3_short")])
HEADER = 10   # bytes of a gzip member's header without optional fields


def group(name):
    return name.split(":")[0]


def reads_text(seed, n, length):
    """FASTQ like test_host_gzip_plan.big_text(): halves of reads copied forward from the read two before, which puts the repeats
    2 records - length/4 and 2 records + length/2 back: 22.5 and 27 KB at the length of 6000 used here."""
    rng = np.random.default_rng(seed)
    bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), (n, length))
    quals = (33 + np.clip(rng.normal(30, 8, (n, length)), 0, 60)).astype(np.uint8)
    parts = []
    for i in range(n):
        if i >= 2 and i % 2 == 1:
            bases[i, : length // 2] = bases[i - 2, length // 4: length // 4 + length // 2]
        elif i >= 2:
            bases[i, length // 2:] = bases[i - 2, : length - length // 2]
        parts.append(b"@read%d/ccs np=%d\n" % (i, i % 17) + bases[i].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n")
    return b"".join(parts)


def flushed(text, level, flushes, seed, wbits=31, finish=True):
    """text deflated with a flush of the given kinds (in turn) after every 1024 .. 2048 bytes of it."""
    rng = np.random.default_rng(seed)
    co = zlib.compressobj(level, zlib.DEFLATED, wbits)
    out, at, k = [], 0, 0
    while at < len(text):
        n = int(rng.integers(1024, 2049))
        out.append(co.compress(text[at:at + n]))
        at += n
        if at < len(text):
            out.append(co.flush(flushes[k % len(flushes)]))
            k += 1
    out.append(co.flush() if finish else co.flush(zlib.Z_FULL_FLUSH))
    return b"".join(out)


def raw_of(blocks):
    """(raw DEFLATE stream, the bit every block starts at).  deflate_craft.deflate() resolves the text as it writes and so cannot write
    a distance that reaches too far back; this writes what it is told."""
    w = dc.BitWriter()
    bits = []
    for b in blocks:
        bits.append(w.nbits)
        dc.write_block(w, b)
    return w.getvalue(), bits


def planned_chunks(blocks, bits, chunk, header=HEADER):
    """The start bits (from the member's first byte) of the chunks tbk_gz_plan_window makes of a one-member file in one window, if every
    guess is a true one: the member's first block, then the first non-final dynamic block that starts in each later span of `chunk`
    bytes."""
    found = {}
    for b, at in zip(blocks, bits):
        k = (at // 8) // chunk
        if b.kind == "dynamic" and not b.final and k >= 1:
            found.setdefault(k, header * 8 + at)
    return [header * 8] + [found[k] for k in sorted(found)]


def _stored(data, final=False):
    """A stored block at a byte boundary, as bytes."""
    assert len(data) <= 0xFFFF
    return bytes([1 if final else 0]) + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data


def _hand_built(name, blocks, chunk, zero_symbol_chunk=False):
    raw, bits = raw_of(blocks)
    text = zlib.decompress(raw, -15)
    plan = planned_chunks(blocks, bits, chunk)
    _MIN_ACCEPTED[name] = len(plan)
    if zero_symbol_chunk:   # some chunk holds nothing but blocks without symbols
        starts = [HEADER * 8 + at for at in bits]
        assert any(all(not b.tokens and not b.data for b, at in zip(blocks, starts) if lo <= at < hi) for lo, hi in zip(plan[1:], plan[2:])), name
    return name, dc.member(raw, text, bgzf=False), chunk, None, text


def _marker_extremes(rng):
    """Block A: 33 000 literals, some ten spans of 1024 bytes: chunk 0, whose window is known.  What follows starts in a later span, in
    a chunk that knows nothing of its window."""
    a = Block("dynamic", tokens=list(dc.fasta_history(rng, 33000, b">a")))
    tail = list(b"\n>b\nACGTTGCAAGGCTTAACCGGTTAC\n")
    end = Block("fixed", tokens=list(b">end\nACGT\n"), final=True)
    out = []
    # distance 32768 (marker 0x8000 + 0) and length 258 at the chunk's first symbol; copies that overlap themselves, out of markers
    b1 = Block("dynamic", tokens=[(258, 32768), (3, 32768), (258, 1), (65, 1), (258, 2), (4, 3)] + tail)
    out.append(_hand_built("extremes:far_end_first", [a, b1, end], 1024))
    # a match whose source is the window's last element (marker 0xFFFF), spread over 258 elements
    b2 = Block("dynamic", tokens=[(258, 1), (3, 32768), (258, 32767), (65, 2)] + tail)
    out.append(_hand_built("extremes:near_end_first", [a, b2, end], 1024))
    # a chain: B (950 bytes that do not compress: over 1024 bytes of stream, so C starts in a later span) and C (under 1 KB) reach
    # through each other into A
    b3 = Block("dynamic", tokens=[int(v) for v in rng.integers(0, 256, 950)])
    c3 = Block("dynamic", tokens=[(258, 32768), (100, 32000), (3, 32768), (258, 32000), (17, 951)] + tail)
    out.append(_hand_built("extremes:chain", [a, b3, c3, end], 1024))
    # the same with blocks of no symbols between A and B: one, and fifty whose headers fill several spans by themselves
    w = [1 + (s * 7 % 13) ** 3 for s in range(286)]
    empty = dict(tokens=[], lit_lens=dc.limited_lengths(w, 15), dist_lens=dc.chain_lengths(list(range(30)), 30, 15), hlit=286, hdist=30, runs="none")
    out.append(_hand_built("extremes:chain_empty_1", [a, Block("dynamic", **empty), b3, c3, end], 1024))
    out.append(_hand_built("extremes:chain_empty_50", [a] + [Block("dynamic", **empty) for _ in range(50)] + [b3, c3, end], 1024, zero_symbol_chunk=True))
    return out


def _dynamic_stored_fixed(rng):
    """dynamic, stored, fixed, dynamic, stored (empty), dynamic, over and over, cut from one token list: the matches of the later blocks
    reach back into the stored and the fixed ones."""
    text = dc.fastq_text(rng, 260, 200, dup=0.3)
    toks = dc.greedy_tokens(text)
    plan = (("dynamic", 3000), ("stored", 1200), ("fixed", 1200), ("dynamic", 3000), ("stored", 0), ("dynamic", 3000))
    blocks, at, i, k = [], 0, 0, 0
    while i < len(toks):
        kind, want = plan[k % len(plan)]
        k += 1
        j, n = i, 0
        while j < len(toks) and n < want:
            n += 1 if isinstance(toks[j], int) else toks[j][0]
            j += 1
        blocks.append(Block("stored", data=text[at:at + n]) if kind == "stored" else Block(kind, tokens=toks[i:j]))
        at, i = at + n, j
    blocks.append(Block("fixed", tokens=list(b"@end\nA\n+\nI\n"), final=True))
    case = _hand_built("storedfixed:cycle", blocks, 1024)
    assert case[4] == text + b"@end\nA\n+\nI\n"
    return case, blocks


def _segments(parts):
    """A member of raw streams that each end on a byte boundary (Z_FULL_FLUSH: no match reaches across) and stored blocks between."""
    raw = b"".join(parts) + _stored(b"", final=True)
    text = zlib.decompress(raw, -15)
    return dc.member(raw, text, bgzf=False), text


def _decoys(rng, pool):
    header, _ = raw_of([Block("dynamic", tokens=dc.greedy_tokens(pool[:3000]))])
    whole, garbage = [], []
    for k in range(12):
        real = flushed(pool[k * 50_000:(k + 1) * 50_000], 6, (zlib.Z_BLOCK,), 40 + k, wbits=-15, finish=False)
        whole += [real, _stored(flushed(pool[700_000 + k * 60_000: 760_000 + k * 60_000], 6, (zlib.Z_BLOCK,), 60 + k, wbits=-15))]
        garbage += [real, _stored(header[:160] + rng.integers(0, 256, 30_000, dtype=np.uint8).tobytes())]
    out = []
    for name, parts in (("decoy:whole_streams", whole), ("decoy:headers_and_noise", garbage)):
        blob, text = _segments(parts)
        assert len(blob) < 2_000_000
        out.append((name, blob, 4096, None, text))
    return out


def _many_members(rng, pool):
    parts = []
    for i in range(300):
        at, n = int(rng.integers(0, len(pool) - 6200)), 0 if i % 10 == 3 else int(rng.integers(2048, 6145))
        text, level = pool[at:at + n], (0, 1, 6, 9)[int(rng.integers(0, 4))]
        if i % 7 == 2:
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            parts.append(dc.member(co.compress(text) + co.flush(), text, bgzf=False, fname=b"part%d.fq" % i, fhcrc=True))
        else:
            co = zlib.compressobj(level, zlib.DEFLATED, 31)
            parts.append(co.compress(text) + co.flush())
        if i % 5 == 0:
            parts.append(b"\0" * int(rng.integers(1, 4)))
    blob = b"".join(parts)
    return "members:300", blob, None, None, gzip.decompress(blob)


def _far_back(first, pool, chunks_in):
    """A second member whose late block copies three bytes from one byte before the member's first on.  Its trailer holds the CRC-32 of
    the text with 0xFF for that byte - the low byte of "nothing there" - so that the stream's only fault is the distance."""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    rng = np.random.default_rng(70 + chunks_in)
    out, size, at = [], 0, 0
    while size < chunks_in * 1024 + 300:
        n = int(rng.integers(1024, 2049))
        out.append(co.compress(pool[at:at + n]) + co.flush(zlib.Z_BLOCK))
        size, at = size + len(out[-1]), at + n
    out.append(co.flush(zlib.Z_SYNC_FLUSH))
    lits = b"@late\nACGT"
    assert at + len(lits) + 1 <= 32768
    raw, _ = raw_of([Block("dynamic", tokens=list(lits) + [(3, at + len(lits) + 1)] + list(b"\n+\nIIIIIII\n")),
                     Block("fixed", tokens=list(b"@end\nA\n+\nI\n"), final=True)])
    said = pool[:at] + lits + b"\xff" + pool[:2] + b"\n+\nIIIIIII\n" + b"@end\nA\n+\nI\n"
    d = zlib.decompressobj(-15, zdict=b"\xff")   # the byte in front of the member, were it there and 0xFF
    assert d.decompress(b"".join(out) + raw) == said and d.eof
    _FAR_BACK_TEXT[chunks_in] = gzip.decompress(first) + said
    # the hand-built block lies behind chunks_in * 1024 bytes of a stream with a block start every 1100 bytes or sooner: in chunk
    # chunks_in or later of the member's window
    _REFUSALS["refused:far_back_%d_chunks_in" % chunks_in] = (("distance too far back",), chunks_in + 1)
    return "refused:far_back_%d_chunks_in" % chunks_in, first + dc.member(b"".join(out) + raw, said, bgzf=False), 1024, None, REFUSED


@functools.lru_cache(maxsize=1)
def cases():
    out = []
    short = reads_text(21, 50, 6000)   # 600 KB
    pool = reads_text(22, 125, 6000)   # 1.5 MB to cut from
    # ---- chains of short chunks: a block boundary every 1 - 2 KB of text, chunks of 1024 bytes ----
    streams = {"zblock_l%d" % level: flushed(short, level, (zlib.Z_BLOCK,), 30 + level) for level in (1, 6, 9)}
    streams["sync"] = flushed(short, 6, (zlib.Z_SYNC_FLUSH,), 31)
    streams["partial"] = flushed(short, 6, (zlib.Z_PARTIAL_FLUSH,), 32)
    streams["full"] = flushed(short, 6, (zlib.Z_FULL_FLUSH,), 33)
    streams["mixed"] = flushed(short, 6, (zlib.Z_BLOCK, zlib.Z_SYNC_FLUSH, zlib.Z_BLOCK, zlib.Z_PARTIAL_FLUSH, zlib.Z_BLOCK, zlib.Z_FULL_FLUSH), 34)
    for name, blob in streams.items():
        out.append(("short:" + name, blob, 1024, None, short))
        if name.startswith("zblock") or name == "mixed":
            out.append(("short_w1024:" + name, blob, 1024, 1024, short))
    # ---- hand-built ----
    rng = np.random.default_rng(23)
    out += _marker_extremes(rng)
    cycle, cycle_blocks = _dynamic_stored_fixed(rng)
    out.append(cycle)
    # ---- stored blocks from zlib: 200 KB of FASTQ, then a record of 100 KB that does not compress, four times ----
    parts = []
    for k in range(4):
        noise = rng.integers(0, 255, 100_000, dtype=np.uint8)
        noise[noise >= 10] += 1   # (no line feed)
        parts += [pool[k * 204_340:(k + 1) * 204_340], b"@noise%d\n" % k + noise[:50_000].tobytes() + b"\n+\n" + noise[50_000:].tobytes() + b"\n"]
    alternating = b"".join(parts)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    alt_blob = co.compress(alternating) + co.flush()
    out.append(("storedfixed:fastq_and_noise", alt_blob, 4096, None, alternating))
    out += _decoys(rng, pool)
    out.append(_many_members(rng, pool))
    big = reads_text(24, 170, 6000) + (b"ACGTTGCA" * 7 + b"\n") * (20_000_000 // 57)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    out.append(("ratio:periodic_after_fastq", co.compress(big) + co.flush(), 70_000, None, big))
    # ---- refused ----
    first = gzip.compress(pool[:80_000], 6)
    for chunks_in in (1, 3, 9):
        out.append(_far_back(first, pool[100_000:], chunks_in))
    z6 = streams["zblock_l6"]
    # a flushed stream has a block start every 2048 bytes of text, 1100 bytes of stream, or sooner: at least every other span of 1024
    # bytes starts a chunk, so half the spans in front of the damage are chunks kept
    _REFUSALS["refused:bit_flip_in_a_late_chunk"] = (("CRC or size mismatch",), len(z6) // 2 // 1024 // 2)
    out.append(("refused:bit_flip_in_a_late_chunk", z6[:len(z6) // 2] + bytes([z6[len(z6) // 2] ^ 0x10]) + z6[len(z6) // 2 + 1:], 1024, None, REFUSED))
    sync = streams["sync"]
    at = sync.index(b"\x00\x00\xff\xff", len(sync) // 2)
    _REFUSALS["refused:bit_flip_in_nlen"] = (("corrupt stored block",), at // 1024 // 2)
    out.append(("refused:bit_flip_in_nlen", sync[:at + 2] + b"\xfb" + sync[at + 3:], 1024, None, REFUSED))
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    fastq_bytes = len(co.compress(parts[0]) + co.flush(zlib.Z_BLOCK))
    # (zlib's own blocks of FASTQ are some 30 KB of stream: few chunks of 4096 bytes, but guessed ones, in front of the noise)
    _REFUSALS["refused:cut_in_a_stored_block"] = (("truncated gzip file",), 2)
    out.append(("refused:cut_in_a_stored_block", alt_blob[:fastq_bytes + 50_000], 4096, None, REFUSED))
    full = streams["full"]
    at = full.index(b"\x00\x00\xff\xff", len(full) // 2)
    # (the header's code lengths run into the zeros kept behind the input, which give no code to 256: the decoder says the first
    # fault it meets)
    _REFUSALS["refused:cut_in_a_dynamic_header"] = (("truncated gzip file", "no end-of-block code"), at // 1024 // 2)
    out.append(("refused:cut_in_a_dynamic_header", full[:at + 4 + 20], 1024, None, REFUSED))
    m = [gzip.compress(pool[k * 30_000:(k + 1) * 30_000], 6) for k in range(3)]
    _REFUSALS["refused:cut_in_the_trailer_2_of_3"] = (("truncated gzip file",), 1)
    _REFUSALS["refused:trailer_2_of_3_short"] = (("CRC or size mismatch",), 1)
    out.append(("refused:cut_in_the_trailer_2_of_3", m[0] + m[1][:-3], None, None, REFUSED))
    out.append(("refused:trailer_2_of_3_short", m[0] + m[1][:-4] + m[2], None, None, REFUSED))
    # ---- the oracle ----
    for name, blob, _, _, expect in out:
        if expect is REFUSED:
            try:
                gzip.decompress(blob)
            except Exception:
                continue
            raise AssertionError("gzip.decompress takes " + name)
        assert gzip.decompress(blob) == expect, name
    assert len(out) == len(NAMES) and {c[0] for c in out} == set(NAMES), [c[0] for c in out]
    out.sort(key=lambda c: NAMES.index(c[0]))
    assert set(_REFUSALS) == {c[0] for c in out if c[4] is REFUSED}
    return out


def min_accepted():
    """{name: chunks planned} of the hand-built files."""
    cases()
    return dict(_MIN_ACCEPTED)


def refusal(name):
    """(the messages a refusal of the file may give, the least chunks some window keeps in front of and with the damage)."""
    cases()
    return _REFUSALS[name]


def far_back_text(chunks_in):
    """What the file of refused:far_back_<chunks_in>_chunks_in would say if the bytes in front of its second member were 0xFF: FASTQ up
    to the record "@late", which holds the reference."""
    cases()
    return _FAR_BACK_TEXT[chunks_in]


def case(name):
    return next(c for c in cases() if c[0] == name)
