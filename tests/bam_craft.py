"""Unaligned BAM files made by hand (``struct`` and ``zlib`` only: no htslib here) and the rule the reader's BAM input is
held to, restated independently of the C++ and the kernels: ``fastq_of`` is what ``samtools fastq`` prints for the records,
without a ``/1`` suffix or tags.

A record is a dict, so that a test can break one field at a time: ``record`` fills it from the read and ``encode`` writes
it, taking every length from the data unless the dict names another (``l_read_name``, ``l_seq``, ``block_size``,
``raw_name``)."""
import struct
import zlib

LETTERS = "=ACMGRSVTWYHKDBN"
COMPLEMENT = "=TGKCYSBAWRDMHVN"  # the complement of the letter with the same code
SKIP_DEFAULT = 0x900            # secondary | supplementary
MAX_RECORD = 1 << 28
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def record(name, seq, qual=None, flag=4, n_cigar=0, tags=b""):
    """name: str; seq: a string over LETTERS; qual: a sequence of ints 0..255 as long as seq, or None for the absent form
    (0xFF throughout); n_cigar: that many cigar operations (their content is of no interest to a reader of unaligned reads)."""
    assert qual is None or len(qual) == len(seq)
    return {"name": name, "seq": seq, "qual": None if qual is None else bytes(qual), "flag": flag, "n_cigar": n_cigar, "tags": bytes(tags)}


def encode(rec):
    name = rec.get("raw_name", rec["name"].encode() + b"\0")
    seq = rec["seq"]
    codes = [LETTERS.index(c) for c in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    qual = rec["qual"] if rec["qual"] is not None else b"\xff" * len(seq)
    cigar = b"".join(struct.pack("<I", (7 + i) << 4) for i in range(rec["n_cigar"]))
    body = name + cigar + packed + qual + rec["tags"]
    fixed = struct.pack("<iiBBHHHIiii", -1, -1, rec.get("l_read_name", len(name)) & 0xFF, 0, 4680, rec["n_cigar"], rec["flag"],
                        rec.get("l_seq", len(seq)), -1, -1, 0)
    assert len(fixed) == 32
    return struct.pack("<I", rec.get("block_size", len(fixed) + len(body)) & 0xFFFFFFFF) + fixed + body


def header(refs=(), text=b"@HD\tVN:1.6\tSO:unknown\n"):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out


def records_bytes(records):
    """the records back to back, and where each begins"""
    offsets, out = [], bytearray()
    for r in records:
        offsets.append(len(out))
        out += encode(r)
    return bytes(out), offsets


def bam_bytes(records, refs=(), text=b"@HD\tVN:1.6\tSO:unknown\n"):
    """the uncompressed BAM: header and records"""
    return header(refs, text) + records_bytes(records)[0]


def bgzf(data, block=0xFF00, level=6, eof=True):
    """bgzf members of at most `block` bytes of payload each (small payloads make records straddle blocks), then the
    end-of-file marker"""
    out = bytearray()
    for at in range(0, len(data), block):
        piece = data[at:at + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out += struct.pack("<BBBBIBBHBBHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25)
        out += body + struct.pack("<II", zlib.crc32(piece), len(piece))
    return bytes(out) + (EOF_BLOCK if eof else b"")


class BamError(ValueError):
    def __init__(self, record_no, why):
        super().__init__("record {}: {}".format(record_no, why))
        self.record_no = record_no


def text_of(rec, skip_flags=SKIP_DEFAULT):
    """the FASTQ (FASTA without quality) text of one record as `record` made it; b"" when it is skipped"""
    seq, qual = rec["seq"], rec["qual"]
    if not seq or rec["flag"] & skip_flags:
        return b""
    absent = qual is None or qual[0] == 0xFF
    if rec["flag"] & 0x10:
        seq = "".join(COMPLEMENT[LETTERS.index(c)] for c in reversed(seq))
        qual = None if qual is None else qual[::-1]
    if absent:
        return ">{}\n{}\n".format(rec["name"], seq).encode()
    return "@{}\n{}\n+\n".format(rec["name"], seq).encode() + bytes(min(q, 93) + 33 for q in qual) + b"\n"


def fastq_of(records, skip_flags=SKIP_DEFAULT):
    return b"".join(text_of(r, skip_flags) for r in records)


def lengths_of(records, skip_flags=SKIP_DEFAULT):
    return [len(text_of(r, skip_flags)) for r in records]


def parse(data, skip_flags=SKIP_DEFAULT):
    """An uncompressed BAM (bytes) -> its FASTQ text, by the rule of include/tbk.h read from the bytes alone (what a broken
    record does is decided here, not in `record`).  Raises BamError with the 0-based number of the first bad record."""
    if data[:4] != b"BAM\1":
        raise BamError(0, "not a BAM file")
    try:
        (l_text,) = struct.unpack_from("<i", data, 4)
        p = 8 + l_text
        (n_ref,) = struct.unpack_from("<i", data, p)
        p += 4
        for _ in range(n_ref):
            (l_name,) = struct.unpack_from("<i", data, p)
            p += 8 + l_name
        if p > len(data):
            raise struct.error
    except struct.error:
        raise BamError(0, "the file ends inside the header")
    out, no = bytearray(), 0
    while p < len(data):
        if len(data) - p < 4:
            raise BamError(no, "the file ends inside the record")
        (bs,) = struct.unpack_from("<I", data, p)
        if bs > MAX_RECORD:
            raise BamError(no, "block_size too large")
        if bs < 32:
            raise BamError(no, "block_size too small")
        if len(data) - p - 4 < bs:
            raise BamError(no, "the file ends inside the record")
        l_name, n_cigar, flag, l_seq = data[p + 12], *struct.unpack_from("<HHI", data, p + 16)
        if bs < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            raise BamError(no, "block_size too small")
        if l_name < 2:
            raise BamError(no, "l_read_name < 2")
        name = data[p + 36:p + 36 + l_name]
        if name[-1] != 0:
            raise BamError(no, "no NUL")
        if any(c < 0x21 or c > 0x7E for c in name[:-1]):
            raise BamError(no, "name byte")
        s = p + 36 + l_name + 4 * n_cigar
        seq = "".join(LETTERS[(data[s + (i >> 1)] >> (4 * (1 - (i & 1)))) & 15] for i in range(l_seq))
        qual = data[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq]
        out += text_of({"name": name[:-1].decode(), "seq": seq, "qual": qual, "flag": flag}, skip_flags)
        p += 4 + bs
        no += 1
    return bytes(out)
