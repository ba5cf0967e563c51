"""A plain-Python DEFLATE reader (RFC 1951) that reports the STRUCTURE of what it reads, and the gzip / bgzf framing around it (RFC
1952, SAM spec 4.1).  ``deflate_craft`` is the writer; this is its counterpart and shares its tables.  No zlib in here: the point is a
second opinion on a stream - which blocks it has, which code lengths each one sent and how, which tokens - so that a test can tell
which paths an ENCODER took from the bytes it wrote, and hold the code it chose against a rule.  It is a helper: pytest does not
collect it (no ``test_`` prefix).

``read_raw(buf, at)`` reads one raw DEFLATE stream that starts at byte ``at``; ``read_member(buf, at)`` one gzip member.  Both refuse
(``BadStream``) what RFC 1951 forbids; a code that is over-subscribed, or incomplete - but for a distance code of one symbol of
length 1, or of none - is refused with ``BadCode``.
"""
import struct
from dataclasses import dataclass, field
from typing import List, Tuple, Union

from deflate_craft import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA, len_code

Token = Union[int, Tuple[int, int]]


class BadStream(ValueError):
    """The bytes are not a DEFLATE stream / a gzip member."""


class BadCode(BadStream):
    """A Huffman code that no decoder may accept, or a header that describes none."""


@dataclass
class Block:
    kind: str                       # "stored", "fixed" or "dynamic"
    final: bool
    bits: Tuple[int, int]           # [first bit, bit behind the block) of the stream, counted from the stream's first byte
    text: Tuple[int, int]           # [start, end) of the block's bytes in the inflated text
    tokens: List[Token] = field(default_factory=list)   # a literal is an int, a match (length, distance); a stored block has none
    # ---- dynamic blocks ----
    hlit: int = 0                   # as counts: 257 .. 286, 1 .. 30, 4 .. 19
    hdist: int = 0
    hclen: int = 0
    cl_lens: List[int] = field(default_factory=list)             # the 19 code-length-code lengths, by symbol
    cl_tokens: List[Tuple[int, int]] = field(default_factory=list)   # as written: (symbol, how many lengths it stands for)
    lit_lens: List[int] = field(default_factory=list)            # hlit lengths (fixed: the 288 of the fixed code)
    dist_lens: List[int] = field(default_factory=list)           # hdist lengths
    symbols_at: int = 0             # the bit where the block's tokens begin (behind the header)


@dataclass
class Member:
    header: dict                    # flg, mtime, xfl, os, extra (list of (si1 si2, bytes)), bsize, fname, fcomment, hcrc, raw_at
    blocks: List[Block]
    text: bytes
    crc: int                        # the trailer's
    isize: int
    end: int                        # the byte behind the member


class _Bits:
    def __init__(self, buf: bytes, at: int):
        self.buf, self.base, self.byte, self.acc, self.n = buf, at, at, 0, 0

    @property
    def pos(self) -> int:
        return (self.byte - self.base) * 8 - self.n

    def need(self, n: int) -> None:
        while self.n < n:
            if self.byte >= len(self.buf):
                raise BadStream("the stream ends inside a block")
            self.acc |= self.buf[self.byte] << self.n
            self.byte += 1
            self.n += 8

    def get(self, n: int) -> int:
        if not n:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    def align(self) -> None:
        """To the next byte boundary; whole bytes looked at ahead go back."""
        self.byte -= self.n >> 3
        self.acc = self.n = 0


def check_code(lens, what: str, lone_ok: bool = False) -> None:
    """RFC 1951 3.2.2: the lengths must fill the code space exactly.  lone_ok: one code of length 1, or none at all, passes too."""
    used = [l for l in lens if l]
    total = sum(1 << (15 - l) for l in used)
    if total > 1 << 15:
        raise BadCode("%s code over-subscribed" % what)
    if total < 1 << 15 and not (lone_ok and (not used or used == [1])):
        raise BadCode("%s code incomplete" % what)


class _Decoder:
    """Canonical code -> symbols (RFC 1951 3.2.2; a code goes into the stream from its most significant bit, 3.1.1): a table over the
    next `longest` bits of the stream."""

    def __init__(self, lens):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        self.longest = max((l for l in range(1, 16) if count[l]), default=0)
        size = 1 << self.longest
        self.table = [None] * size
        nxt, code = [0] * 16, 0
        for l in range(1, 16):
            code = (code + count[l - 1]) << 1
            nxt[l] = code
        for s, l in enumerate(lens):
            if not l:
                continue
            c = nxt[l]
            nxt[l] += 1
            if c >> l:
                continue   # (over-subscribed: check_code has refused it)
            r = int(format(c, "0%db" % l)[::-1], 2)
            for k in range(r, size, 1 << l):
                self.table[k] = (s, l)

    def read(self, b: _Bits) -> int:
        want = self.longest
        while b.n < want and b.byte < len(b.buf):
            b.acc |= b.buf[b.byte] << b.n
            b.byte += 1
            b.n += 8
        e = self.table[b.acc & ((1 << want) - 1)] if want else None
        if e is None:
            raise BadCode("bits that are no code")
        if e[1] > b.n:
            raise BadStream("the stream ends inside a block")
        b.acc >>= e[1]
        b.n -= e[1]
        return e[0]


def _read_dynamic_header(b: _Bits, blk: Block) -> None:
    blk.hlit, blk.hdist, blk.hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    if blk.hlit > 286 or blk.hdist > 30:
        raise BadCode("too many length or distance symbols")
    blk.cl_lens = [0] * 19
    for i in range(blk.hclen):
        blk.cl_lens[CL_ORDER[i]] = b.get(3)
    check_code(blk.cl_lens, "code-length")
    cl = _Decoder(blk.cl_lens)
    lens: List[int] = []
    total = blk.hlit + blk.hdist
    while len(lens) < total:
        s = cl.read(b)
        if s < 16:
            rep, v = 1, s
        elif s == 16:
            if not lens:
                raise BadCode("a repeat with no length before it")
            rep, v = 3 + b.get(2), lens[-1]
        elif s == 17:
            rep, v = 3 + b.get(3), 0
        else:
            rep, v = 11 + b.get(7), 0
        if len(lens) + rep > total:
            raise BadCode("a repeat past the last length")
        blk.cl_tokens.append((s, rep))
        lens += [v] * rep
    blk.lit_lens, blk.dist_lens = lens[:blk.hlit], lens[blk.hlit:]
    if not blk.lit_lens[256]:
        raise BadCode("no end-of-block code")
    check_code(blk.lit_lens, "literal/length")
    check_code(blk.dist_lens, "distance", lone_ok=True)


def read_raw(buf: bytes, at: int = 0, history: bytes = b"") -> Tuple[List[Block], bytes, int]:
    """(blocks, text, the byte behind the stream) of the raw DEFLATE stream at buf[at:]."""
    b = _Bits(buf, at)
    out = bytearray(history)
    blocks: List[Block] = []
    while True:
        start = b.pos
        final, btype = bool(b.get(1)), b.get(2)
        t0 = len(out)
        if btype == 3:
            raise BadStream("block type 3")
        if btype == 0:
            b.align()
            n, nn = b.get(16), b.get(16)
            if n ^ nn != 0xFFFF:
                raise BadStream("a stored block whose NLEN is not the complement of LEN")
            assert b.n == 0
            if b.byte + n > len(buf):
                raise BadStream("the stream ends inside a stored block")
            out += buf[b.byte:b.byte + n]
            b.byte += n
            blk = Block("stored", final, (start, b.pos), (t0 - len(history), len(out) - len(history)))
            blk.symbols_at = b.pos - 8 * n
        else:
            blk = Block("fixed" if btype == 1 else "dynamic", final, (start, start), (0, 0))
            if btype == 1:
                blk.lit_lens, blk.dist_lens = list(FIXED_LIT), list(FIXED_DIST)
            else:
                _read_dynamic_header(b, blk)
            blk.symbols_at = b.pos
            lit, dist = _Decoder(blk.lit_lens), _Decoder(blk.dist_lens)
            while True:
                s = lit.read(b)
                if s < 256:
                    out.append(s)
                    blk.tokens.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise BadStream("length symbol %d" % s)
                length = LEN_BASE[s - 257] + b.get(LEN_EXTRA[s - 257])
                if not dist.longest:
                    raise BadStream("a match in a block without distance codes")
                d = dist.read(b)
                if d > 29:
                    raise BadStream("distance symbol %d" % d)
                d = DIST_BASE[d] + b.get(DIST_EXTRA[d])
                if d > len(out):
                    raise BadStream("a distance past the start of the text")
                blk.tokens.append((length, d))
                if d == 1:
                    out += out[-1:] * length
                else:
                    for _ in range(length):
                        out.append(out[-d])
            blk.bits, blk.text = (start, b.pos), (t0 - len(history), len(out) - len(history))
        blocks.append(blk)
        if final:
            break
    b.align()
    return blocks, bytes(out[len(history):]), b.byte


_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data: bytes) -> int:
    c = 0xFFFFFFFF
    t = _CRC_TABLE
    for v in data:
        c = t[(c ^ v) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def read_member(buf: bytes, at: int = 0) -> Member:
    """The gzip member at buf[at:]: header fields, blocks, text, trailer.  The trailer's CRC-32 and ISIZE must be the text's."""
    if len(buf) < at + 10 or buf[at:at + 3] != b"\x1f\x8b\x08":
        raise BadStream("no gzip header")
    flg = buf[at + 3]
    if flg & 0xE0:
        raise BadStream("reserved flag bits")
    mtime, xfl, os_ = struct.unpack_from("<IBB", buf, at + 4)
    h = {"flg": flg, "mtime": mtime, "xfl": xfl, "os": os_, "extra": [], "bsize": None, "fname": None, "fcomment": None, "hcrc": None}
    p = at + 10
    if flg & 4:
        xlen, = struct.unpack_from("<H", buf, p)
        p += 2
        q, end = p, p + xlen
        while q + 4 <= end:
            n, = struct.unpack_from("<H", buf, q + 2)
            h["extra"].append((bytes(buf[q:q + 2]), bytes(buf[q + 4:q + 4 + n])))
            if buf[q:q + 2] == b"BC" and n == 2:
                h["bsize"], = struct.unpack_from("<H", buf, q + 4)
            q += 4 + n
        if q != end:
            raise BadStream("FEXTRA subfields do not fill XLEN")
        p = end
    for key, bit in (("fname", 8), ("fcomment", 16)):
        if flg & bit:
            z = buf.index(b"\0", p)
            h[key] = bytes(buf[p:z])
            p = z + 1
    if flg & 2:
        h["hcrc"], = struct.unpack_from("<H", buf, p)
        if h["hcrc"] != crc32(bytes(buf[at:p])) & 0xFFFF:
            raise BadStream("header CRC")
        p += 2
    h["raw_at"] = p
    blocks, text, end = read_raw(buf, p)
    if end + 8 > len(buf):
        raise BadStream("the member ends before its trailer")
    crc, isize = struct.unpack_from("<II", buf, end)
    if crc != crc32(text) or isize != len(text) & 0xFFFFFFFF:
        raise BadStream("the trailer is not the text's CRC-32 and size")
    if h["bsize"] is not None and h["bsize"] != end + 8 - at - 1:
        raise BadStream("BSIZE is not the member's size - 1")
    return Member(h, blocks, text, crc, isize, end + 8)


def read_members(buf: bytes) -> List[Member]:
    """Every member of a gzip / bgzf file, back to back."""
    out, at = [], 0
    while at < len(buf):
        out.append(read_member(buf, at))
        at = out[-1].end
    return out


def histogram(blk: Block) -> List[int]:
    """The literal/length frequencies of a block's tokens, the end-of-block code included (286 counts)."""
    f = [0] * 286
    f[256] = 1
    for t in blk.tokens:
        f[t if isinstance(t, int) else 257 + len_code(t[0])] += 1
    return f
