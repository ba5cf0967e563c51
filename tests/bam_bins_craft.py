"""Helpers of the BAM-bin tests (include/tbk.h "BAM output"): a bgzf walker that follows BSIZE and checks every field of
every block, a splitter of an uncompressed BAM into header and records, and the crafted input the reader, the writer and
the device tests share.  The inflater is Python's ``zlib``; the records come from ``bam_craft``."""
import random
import struct
import zlib

import bam_craft as bc

PAYLOAD = 65280
EOF_MARKER = bc.EOF_BLOCK
assert len(EOF_MARKER) == 28


def walk(blob):
    """The payloads of the bgzf blocks that make up ``blob``, every field of every block checked: the fixed 16 bytes,
    BSIZE (the walk follows it and must end exactly at the end), a raw deflate stream that ends where the trailer begins,
    CRC-32, ISIZE, payload <= 65280 and block <= 65536."""
    out, p = [], 0
    while p < len(blob):
        assert len(blob) - p >= 26, "a block is cut off at {}".format(p)
        assert blob[p:p + 16] == bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0]), (p, blob[p:p + 16].hex())
        size = struct.unpack_from("<H", blob, p + 16)[0] + 1
        assert 26 <= size <= 65536 and p + size <= len(blob), (p, size)
        d = zlib.decompressobj(-15)
        text = d.decompress(blob[p + 18:p + size - 8])
        assert d.eof and not d.unused_data, "the deflate stream of the block at {} does not end at its trailer".format(p)
        crc, isize = struct.unpack_from("<II", blob, p + size - 8)
        assert crc == zlib.crc32(text), "CRC-32 of the block at {}".format(p)
        assert isize == len(text) <= PAYLOAD, (p, isize, len(text))
        out.append(text)
        p += size
    assert p == len(blob)
    return out


def split_bam(data):
    """An uncompressed BAM -> (header bytes, [record bytes, block_size included])."""
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, p)
        p += 8 + l_name
    header, records = data[:p], []
    while p < len(data):
        (bs,) = struct.unpack_from("<I", data, p)
        assert p + 4 + bs <= len(data), "a record is cut off"
        records.append(data[p:p + 4 + bs])
        p += 4 + bs
    return header, records


def read_bam_file(path):
    """A BAM bin on disk -> (header, records, inflated bytes): the bgzf fields hold and the last 28 bytes are the marker."""
    with open(path, "rb") as fh:
        blob = fh.read()
    assert blob[-28:] == EOF_MARKER, "no end-of-file marker at the end of {}".format(path)
    payloads = walk(blob)
    assert payloads[-1] == b""
    data = b"".join(payloads)
    return split_bam(data) + (data,)


def tag_block(rng, kinetics=0):
    """A tag block as HiFi records carry: scalar tags, a Z string and B arrays (``kinetics`` entries each for fi / ri)."""
    out = b"zmi" + struct.pack("<i", rng.randrange(1 << 20)) + b"rqf" + struct.pack("<f", 0.999) + b"npC" + bytes([rng.randrange(3, 30)])
    out += b"RGZ" + b"0a1b2c3d" + b"\0"
    n = rng.randrange(1, 40)
    out += b"MLBC" + struct.pack("<i", n) + bytes(rng.randrange(256) for _ in range(n))
    out += b"MMZ" + b"C+m," + b",".join(str(rng.randrange(9)).encode() for _ in range(n)) + b";\0"
    if kinetics:
        for tag in (b"fi", b"ri"):
            out += tag + b"BC" + struct.pack("<i", kinetics) + bytes(rng.choices(range(5, 60), k=kinetics))
    return out


def crafted_records(seed=11):
    """The shapes the issue lists: tag blocks with B arrays, a 100 kb read, 1-base reads, records without quality,
    reverse-strand records, records with cigar operations, skipped records between kept ones."""
    rng = random.Random(seed)
    recs = []

    def seq_of(n):
        return "".join(rng.choices("ACGT", k=n))

    def qual_of(n):
        return [rng.randrange(2, 94) for _ in range(n)]

    for i in range(60):
        n = rng.choice([1, 1, 2, 17, 150, 999, 3000, 7001])
        kind = i % 10
        flag = 4
        qual = qual_of(n)
        tags = tag_block(rng, kinetics=n if i % 3 == 0 else 0)
        n_cigar = 0
        if kind == 1:
            flag = 4 | 0x10
        elif kind == 2:
            qual = None
        elif kind == 3:
            flag = 0x100          # secondary: skipped
        elif kind == 4:
            n_cigar = 3
        elif kind == 5:
            flag = 0x800 | 0x10   # supplementary: skipped
        elif kind == 6:
            n, qual = 0, []       # no bases: skipped
        elif kind == 7:
            tags = b""
        recs.append(bc.record("m{}/{}/ccs".format(seed, i), seq_of(n) if n else "", qual, flag=flag, n_cigar=n_cigar, tags=tags))
        if i == 20:
            recs.append(bc.record("long/100kb", seq_of(100000), qual_of(100000), tags=tag_block(rng, kinetics=100000)))
    return recs


def crafted_header():
    """a header whose text is 70 KB of @RG lines: it spans two bgzf blocks"""
    text = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join("@RG\tID:{:08x}\tPL:PACBIO\tDS:READTYPE=CCS\n".format(i).encode() for i in range(1700))
    text += b"@PG\tID:ccs\tPN:ccs\tVN:6.4.0\n"
    assert len(text) > 70000
    return text


def kept(records):
    return [r for r in records if r["seq"] and not r["flag"] & bc.SKIP_DEFAULT]


def big_records(seed=12):
    """crafted_records and, behind them, eight reads of 40-100 kb with kinetics arrays: several MB, so that a writer fed
    batches of growing size gets a few KB first and several MB at the end"""
    rng = random.Random(seed)
    recs = crafted_records(seed)
    for i in range(8):
        n = rng.randrange(40000, 100000)
        recs.append(bc.record("big{}/{}".format(seed, i), "".join(rng.choices("ACGT", k=n)), [rng.randrange(2, 94) for _ in range(n)],
                              flag=4 | (0x10 if i % 2 else 0), tags=tag_block(rng, kinetics=n)))
        if i % 3 == 0:
            recs.append(bc.record("skip{}/{}".format(seed, i), "ACGT", [30] * 4, flag=0x904))
    return recs


# ---- the encoder's shapes (host twin and device alike) ----
SIZES = [(0, 0), (1, 1), (65279, 1), (65280, 1), (65281, 2), (130560, 2)]   # payload bytes -> members


def payload(n, seed=3):
    """n bytes shaped like packed seq, qual and tags taking turns (skewed, so that they compress)"""
    rng = random.Random(seed * 1000003 + n)
    out = bytearray()
    while len(out) < n:
        kind = len(out) // 5000 % 3
        alphabet = (bytes([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88]), bytes(range(2, 50)), bytes(range(256)))[kind]
        out += bytes(rng.choices(alphabet, k=5000))
    return bytes(out[:n])


def incompressible(n=200000, seed=17):
    """bytes from a seeded generator over all 256 values, and hints every 8193 bytes: every deflate block is as short as
    the rule allows and falls back to stored - the member must still fit 65536 bytes"""
    rng = random.Random(seed)
    return rng.randbytes(n), list(range(8193, n, 8193))


def alternating(total=600 * 1024, stretch=12 * 1024, seed=23):
    """12 KiB stretches alternating between 16 equiprobable byte values and 64 others; hints at the stretch boundaries"""
    rng = random.Random(seed)
    a, b = bytes(range(16)), bytes(range(100, 164))
    out = bytearray()
    for i in range(total // stretch):
        out += bytes(rng.choices(a if i % 2 == 0 else b, k=stretch))
    return bytes(out), list(range(0, len(out) + 1, stretch))


def check_members(blob, data, n_members=None):
    """the field checks of `walk`, the count and the inflated bytes of an encoder's output for `data`"""
    payloads = walk(blob)
    assert b"".join(payloads) == data
    assert len(payloads) == (len(data) + PAYLOAD - 1) // PAYLOAD
    assert all(len(p) == PAYLOAD for p in payloads[:-1])
    if n_members is not None:
        assert n_members == len(payloads)
    return payloads


def coded_block_sizes(member):
    """Bytes of text of every deflate block of one bgzf member whose blocks are all coded (none stored): both coders end a
    coded block with an empty stored block - 00 00 ff ff behind a byte boundary - so the text decodable up to each such
    marker says where the blocks end.  (The four bytes could occur inside coded data, once in 2^32 positions: the inputs
    of the tests that use this are fixed.)"""
    d = zlib.decompressobj(-15)
    body, sizes, at = member[18:-8], [], 0
    while True:
        nxt = body.find(b"\x00\x00\xff\xff", at)
        if nxt < 0:
            break
        text = d.decompress(body[at:nxt + 4])
        at = nxt + 4
        if text:
            sizes.append(len(text))
    assert d.eof and at == len(body)
    return sizes


# hints for one member of 65280 bytes -> the blocks the cut rule gives: a block ends at the first hint in (8192, 16384] from its
# start, else at 16384, and at the member's end
CUTS = [
    ([], [16384, 16384, 16384, 16128]),
    ([8192], [16384, 16384, 16384, 16128]),                    # 8192 from the start is not past the least
    ([8193], [8193, 16384, 16384, 16384, 7935]),
    ([100, 16384, 16385], [16384, 16384, 16384, 16128]),       # a hint at 16384 ends the block where it ends anyway; 16385 is 1 into the next
    ([9000, 9001, 30000, 65280], [9000, 16384, 16384, 16384, 7128]),   # 9001 is 1 into the second block; 30000 is 4616 into the third
    ([16384 + 8193, 16384 + 8194], [16384, 8193, 16384, 16384, 7935]),
]
