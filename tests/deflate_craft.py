"""A bit-exact raw DEFLATE writer (RFC 1951) driven by an explicit plan, and gzip / bgzf framing (RFC 1952, SAM spec 4.1).

zlib writes only a small part of what DEFLATE allows: it never runs a code-length repeat across the literal/length to distance
boundary, never writes a distance tree of one code or of none, trims HLIT, HDIST and HCLEN and seldom gives a distance code more than
nine bits.  Other writers (libdeflate, igzip, pigz) do.  This module writes such streams on purpose - and, one knob at a time, streams
that break one rule - so that the suite can hold the project's inflaters against ``gzip.decompress``.  It is a helper: pytest does not
collect it (no ``test_`` prefix).

A plan is a list of ``Block``.  A block holds its tokens: a literal is an int 0..255, a match a ``(length, distance)`` tuple.  Stored
blocks hold ``data`` instead.  ``deflate(blocks)`` returns ``(raw, text)``: the stream and the text it stands for; a stream meant to be
valid is checked against ``zlib.decompress(raw, -15)`` (``check=True``, the default).
"""
import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

Token = Union[int, Tuple[int, int]]


def len_code(length: int) -> int:
    """Length symbol index 0..28 of a match length 3..258 (258 is code 28, not 27 with its largest extra)."""
    assert 3 <= length <= 258, length
    if length == 258:
        return 28
    c = 27
    while LEN_BASE[c] > length:
        c -= 1
    return c


def dist_code(dist: int) -> int:
    assert 1 <= dist <= 32768, dist
    c = 29
    while DIST_BASE[c] > dist:
        c -= 1
    return c


def length_bounds() -> List[int]:
    """Every length code's smallest and largest length."""
    out = []
    for c in range(29):
        lo = LEN_BASE[c]
        hi = 258 if c == 28 else lo + (1 << LEN_EXTRA[c]) - 1
        out += [lo, hi] if hi != lo else [lo]
    return out


def dist_bounds() -> List[int]:
    """Every distance code's smallest and largest distance."""
    out = []
    for c in range(30):
        lo = DIST_BASE[c]
        hi = lo + (1 << DIST_EXTRA[c]) - 1
        out += [lo, hi] if hi != lo else [lo]
    return out


class BitWriter:
    """LSB-first bits into bytes (DEFLATE's order); Huffman codes go in from their most significant bit."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def nbits(self) -> int:
        return len(self.out) * 8 + self.n

    def put(self, value: int, n: int) -> None:
        assert 0 <= value < (1 << n) or n == 0 and value == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int) -> None:
        self.put(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self) -> None:
        if self.n:
            self.put(0, 8 - self.n)

    def data(self, b: bytes) -> None:
        assert self.n == 0
        self.out += b

    def getvalue(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lens: Sequence[int]) -> List[int]:
    """RFC 1951 3.2.2 codes of the lengths (an over-subscribed set gets codes that run past their length: fine for a stream that is
    meant to be refused, as long as those symbols are not written)."""
    bl_count = [0] * 16
    for l in lens:
        bl_count[l] += 1
    bl_count[0] = 0
    next_code, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for l in lens:
        out.append(next_code[l] if l else 0)
        if l:
            next_code[l] += 1
    return out


def kraft(lens: Sequence[int]) -> float:
    return sum(2.0 ** -l for l in lens if l)


def limited_lengths(weights: Sequence[int], max_bits: int) -> List[int]:
    """Optimal code lengths no longer than max_bits for the symbols of nonzero weight (package-merge).  One symbol alone gets
    length 1."""
    syms = sorted((w, s) for s, w in enumerate(weights) if w > 0)
    lens = [0] * len(weights)
    if not syms:
        return lens
    if len(syms) == 1:
        lens[syms[0][1]] = 1
        return lens
    assert len(syms) <= 1 << max_bits
    leaves = [(w, (s,)) for w, s in syms]
    cur = list(leaves)
    for _ in range(max_bits - 1):
        packages = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packages, key=lambda x: x[0])
    for _, ss in cur[:2 * len(syms) - 2]:
        for s in ss:
            lens[s] += 1
    return lens


def chain_lengths(symbols: Sequence[int], nsym: int, max_bits: int) -> List[int]:
    """A complete code over `symbols` as deep as max_bits allows: weights 2^-rank make the Huffman tree a chain, cut at max_bits, so
    that several of the symbols get codes of exactly max_bits."""
    w = [0] * nsym
    for r, s in enumerate(symbols):
        w[s] = 1 << max(0, 40 - r)
    lens = limited_lengths(w, max_bits)
    assert max(lens) == max_bits or len(symbols) <= max_bits, (max(lens), max_bits)
    return lens


@dataclass
class Block:
    kind: str                                  # "stored", "fixed" or "dynamic"
    tokens: List[Token] = field(default_factory=list)
    data: bytes = b""                          # stored blocks
    final: bool = False
    # ---- dynamic blocks: by default the lengths come from the tokens' frequencies, limited to lit_max / dist_max bits ----
    lit_lens: Optional[List[int]] = None       # explicit code lengths of the literal/length alphabet (len >= hlit)
    dist_lens: Optional[List[int]] = None
    lit_max: int = 15
    dist_max: int = 15
    hlit: Optional[int] = None                 # number of literal/length lengths sent (257..288); default trimmed
    hdist: Optional[int] = None                # 1..32; default trimmed
    hclen: Optional[int] = None                # 4..19; default trimmed
    runs: str = "split"                        # code-length runs: "split" (zlib), "cross" (runs span the two trees), "none"
    cl_lens: Optional[List[int]] = None        # explicit code-length code (19 lengths)
    cl_tokens: Optional[List[Tuple[int, int]]] = None   # explicit (symbol, extra value) list instead of the run encoder
    # ---- rule breakers ----
    nlen: Optional[int] = None                 # stored: NLEN that is not ~LEN
    no_eob: bool = False                       # dynamic / fixed: do not write the end-of-block code


def _cl_runs(lens: Sequence[int]) -> List[Tuple[int, int]]:
    """zlib's run encoding of one run of lengths: 16 (3-6 copies of the previous), 17 (3-10 zeros), 18 (11-138 zeros)."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
                r -= k
            if r >= 3:
                out.append((17, r - 3))
                r = 0
            out += [(0, 0)] * r
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                r -= k
            out += [(v, 0)] * r
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _resolve(tokens: Sequence[Token], hist: bytearray) -> None:
    for t in tokens:
        if isinstance(t, int):
            hist.append(t)
        else:
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(hist), (t, len(hist))
            start = len(hist) - dist
            for k in range(length):
                hist.append(hist[start + k])


def _write_symbols(w: BitWriter, tokens, lit_lens, lit_codes, dist_lens, dist_codes, no_eob):
    for t in tokens:
        if isinstance(t, int):
            assert lit_lens[t], ("literal without a code", t)
            w.code(lit_codes[t], lit_lens[t])
        else:
            length, dist = t
            c = len_code(length)
            assert lit_lens[257 + c], ("length without a code", length)
            w.code(lit_codes[257 + c], lit_lens[257 + c])
            w.put(length - LEN_BASE[c], LEN_EXTRA[c])
            d = dist_code(dist)
            assert d < len(dist_lens) and dist_lens[d], ("distance without a code", dist)
            w.code(dist_codes[d], dist_lens[d])
            w.put(dist - DIST_BASE[d], DIST_EXTRA[d])
    if not no_eob:
        w.code(lit_codes[256], lit_lens[256])


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def write_block(w: BitWriter, b: Block) -> None:
    w.put(1 if b.final else 0, 1)
    if b.kind == "stored":
        w.put(0, 2)
        w.align()
        n = len(b.data)
        assert n <= 0xFFFF
        w.data(struct.pack("<HH", n, (~n & 0xFFFF) if b.nlen is None else b.nlen) + b.data)
        return
    if b.kind == "fixed":
        w.put(1, 2)
        _write_symbols(w, b.tokens, FIXED_LIT, canonical_codes(FIXED_LIT), FIXED_DIST, canonical_codes(FIXED_DIST), b.no_eob)
        return
    assert b.kind == "dynamic"
    w.put(2, 2)
    if b.lit_lens is not None:
        lit = list(b.lit_lens)
    else:
        f = [0] * 286
        f[256] = 1
        for t in b.tokens:
            f[t if isinstance(t, int) else 257 + len_code(t[0])] += 1
        lit = limited_lengths(f, b.lit_max)
    if b.dist_lens is not None:
        dist = list(b.dist_lens)
    else:
        f = [0] * 30
        for t in b.tokens:
            if not isinstance(t, int):
                f[dist_code(t[1])] += 1
        dist = limited_lengths(f, b.dist_max) if any(f) else [0]
    hlit = b.hlit if b.hlit is not None else max(257, max((i + 1 for i, l in enumerate(lit) if l), default=0))
    hdist = b.hdist if b.hdist is not None else max(1, max((i + 1 for i, l in enumerate(dist) if l), default=0))
    lit = (lit + [0] * 288)[:hlit]
    dist = (dist + [0] * 32)[:hdist]
    if b.cl_tokens is not None:
        cl = list(b.cl_tokens)
    elif b.runs == "cross":
        cl = _cl_runs(lit + dist)
    elif b.runs == "none":
        cl = [(l, 0) for l in lit + dist]
    else:
        cl = _cl_runs(lit) + _cl_runs(dist)
    if b.cl_lens is not None:
        cl_lens = list(b.cl_lens)
    else:
        f = [0] * 19
        for s, _ in cl:
            f[s] += 1
        if sum(1 for x in f if x) < 2:   # a complete code-length code needs two symbols
            f[1 if not f[1] else 2] += 1
        cl_lens = limited_lengths(f, 7)
    hclen = b.hclen if b.hclen is not None else max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]), default=0))
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl_codes = canonical_codes(cl_lens)
    for s, x in cl:
        w.code(cl_codes[s], cl_lens[s])
        if s in CL_EXTRA:
            w.put(x, CL_EXTRA[s])
    _write_symbols(w, b.tokens, lit, canonical_codes(lit), dist, canonical_codes(dist), b.no_eob)


def deflate(blocks: Sequence[Block], check: bool = True, history: bytes = b"") -> Tuple[bytes, bytes]:
    """(raw DEFLATE stream, its text).  check: the stream must give the text under zlib (a plan meant to be valid)."""
    w = BitWriter()
    hist = bytearray(history)
    for b in blocks:
        write_block(w, b)
        if b.kind == "stored":
            hist += b.data
        else:
            _resolve(b.tokens, hist)
    raw, text = w.getvalue(), bytes(hist[len(history):])
    if check:
        assert blocks and blocks[-1].final and not any(b.final for b in blocks[:-1])
        d = zlib.decompressobj(-15)
        got = d.decompress(raw) + d.flush()
        assert got == text and d.eof and not d.unused_data, "the plan does not give its text under zlib"
    return raw, text


def greedy_tokens(text: bytes, start: int = 0, max_len: int = 258, max_dist: int = 32768, min_dist: int = 1) -> List[Token]:
    """Literals and matches for text[start:] (text[:start] is history): the longest match among the last few places its first three
    bytes were seen, within the limits."""
    heads = {}
    out: List[Token] = []
    for i in range(max(0, start - max_dist - 2), start):
        heads.setdefault(text[i:i + 3], []).append(i)
    i, n = start, len(text)
    while i < n:
        best, bd = 0, 0
        key = text[i:i + 3]
        if len(key) == 3:
            for j in reversed(heads.get(key, [])[-8:]):
                d = i - j
                if d > max_dist:
                    break
                if d < min_dist:
                    continue
                L = 0
                while L < max_len and i + L < n and text[j + L] == text[i + L]:
                    L += 1
                if L > best:
                    best, bd = L, d
        step = best if best >= 3 else 1
        if best >= 3:
            out.append((best, bd))
        else:
            out.append(text[i])
        for k in range(i, i + step):
            heads.setdefault(text[k:k + 3], []).append(k)
        i += step
    return out


def split_tokens(tokens: Sequence[Token], parts: int) -> List[List[Token]]:
    k = max(1, (len(tokens) + parts - 1) // parts)
    return [list(tokens[i:i + k]) for i in range(0, len(tokens), k)]


# ---- framing -------------------------------------------------------------------------------------------------------------------------

def member(raw: bytes, text: bytes, bgzf: bool = True, other: Optional[str] = None, fname: Optional[bytes] = None, fcomment: Optional[bytes] = None,
           fhcrc: bool = False, crc: Optional[int] = None, isize: Optional[int] = None, bsize: Optional[int] = None) -> bytes:
    """One gzip member around a raw DEFLATE stream.  bgzf: FEXTRA holds the BC subfield, whose BSIZE is the member's length - 1 (bsize
    overrides it), alone or with another subfield `other` ("before" or "after" it).  CRC-32 and ISIZE are the text's unless
    overridden."""
    flg = (4 if bgzf else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    head = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff")
    if bgzf:
        sub = b"XY" + struct.pack("<H", 3) + b"abc"
        bc = b"BC" + struct.pack("<H", 2) + b"\0\0"
        extra = {None: bc, "after": bc + sub, "before": sub + bc}[other]
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    if fcomment is not None:
        head += fcomment + b"\0"
    if fhcrc:
        head += struct.pack("<H", zlib.crc32(bytes(head)) & 0xFFFF)
    tail = struct.pack("<II", (zlib.crc32(text) & 0xFFFFFFFF) if crc is None else crc, (len(text) & 0xFFFFFFFF) if isize is None else isize)
    out = bytearray(head) + raw + tail
    if bgzf:
        at = 12 + (7 if other == "before" else 0) + 4
        size = len(out) - 1 if bsize is None else bsize
        assert size <= 0xFFFF, "a bgzf member is at most 65536 bytes"
        out[at:at + 2] = struct.pack("<H", size)
    return bytes(out)


def bgzf_file(members: Sequence[bytes], eof: bool = True) -> bytes:
    return b"".join(members) + (EOF_BLOCK if eof else b"")


# ---- texts ---------------------------------------------------------------------------------------------------------------------------

def fastq_text(rng, n_reads: int, read_len: int, quals: bytes = b"#+5?IS]", dup: float = 0.0) -> bytes:
    """FASTQ records; `dup` of the reads repeat an earlier read's bases (matches at long distances)."""
    recs, seqs = [], []
    for i in range(n_reads):
        L = int(rng.integers(max(1, read_len // 2), read_len + 1))
        if seqs and rng.random() < dup:
            s = seqs[int(rng.integers(0, len(seqs)))]
        else:
            s = bytes(b"ACGT"[c] for c in rng.integers(0, 4, L))
        seqs.append(s)
        q = bytes(quals[c] for c in rng.integers(0, len(quals), len(s)))
        recs.append(b"@r%d x\n%s\n+\n%s\n" % (i, s, q))
    return b"".join(recs)


def fasta_history(rng, n: int, name: bytes = b">h") -> bytes:
    """A FASTA record of about n bytes: a name line, then lines of 60 random bases."""
    out = bytearray(name + b"\n")
    while len(out) < n:
        out += bytes(b"ACGT"[c] for c in rng.integers(0, 4, 60)) + b"\n"
    return bytes(out[:n - 1]) + b"\n"


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
# Every case is (name, text, raw): a raw DEFLATE stream and the text it stands for.  Texts are FASTQ or FASTA (what the reader takes),
# at most 65536 bytes (one bgzf member), and every stream of valid_streams() passed deflate()'s zlib check.

MAX_BGZF_TEXT = 65536


def _lits(b: bytes) -> List[Token]:
    return list(b)


def _dyn_from_text(text: bytes, final=True, **kw) -> Block:
    return Block("dynamic", tokens=greedy_tokens(text), final=final, **kw)


def _shaped_lit_lens(text_syms, zero_runs_at, max_bits=15) -> List[int]:
    """A complete literal/length code: the text's symbols and 256 heavy, every symbol below 286 that is not in zero_runs_at light (codes
    nobody writes, which shape the code-length runs)."""
    w = [0] * 286
    for s in range(286):
        if s not in zero_runs_at:
            w[s] = 1
    for s in text_syms:
        w[s] = 1 << 20
    w[256] = 1 << 20
    return limited_lengths(w, max_bits)


def _matrix_members(rng) -> List[Tuple[str, bytes, bytes]]:
    """Every length code's smallest and largest length against every distance code's smallest and largest distance; members of
    FASTA history (stored blocks) followed by a dynamic block of the planned matches, the deeper members with 15-bit codes."""
    pairs = sorted((d, L) for d in dist_bounds() for L in length_bounds())
    out, cur, k = [], [], 0

    def flush(cur, k):
        hist_n = max(64, max(d for d, _ in cur))
        hist = fasta_history(rng, hist_n, b">m%d" % k)
        toks = [(L, d) for d, L in cur]
        used_d = sorted({dist_code(d) for d, _ in cur})
        used_l = sorted({257 + len_code(L) for _, L in cur})
        deep = k % 2 == 0
        blocks = [Block("stored", data=hist[i:i + 20000]) for i in range(0, len(hist), 20000)]
        blocks.append(Block("dynamic", tokens=toks, final=True,
                            lit_lens=chain_lengths(used_l + [256], 286, 15) if deep else None,
                            dist_lens=chain_lengths(used_d, 30, 15) if deep and len(used_d) > 15 else None))
        raw, text = deflate(blocks)
        out.append(("len_x_dist_%d" % k, text, raw))

    size = 0
    for d, L in pairs:
        need = max(64, d) + size + L
        if cur and need > MAX_BGZF_TEXT - 64:
            flush(cur, k)
            k += 1
            cur, size = [], 0
        cur.append((d, L))
        size += L
    flush(cur, k)
    return out


def valid_streams(seed: int = 11) -> List[Tuple[str, bytes, bytes]]:
    import numpy as np

    rng = np.random.default_rng(seed)
    cases = []

    def add(name, blocks):
        raw, text = deflate(blocks)
        assert len(text) <= MAX_BGZF_TEXT, (name, len(text))
        cases.append((name, text, raw))

    fq = fastq_text(rng, 120, 200, quals=bytes(range(35, 75)), dup=0.3)[:60000]
    fq = fq[:fq.rfind(b"\n@") + 1]
    syms = sorted(set(fq))
    toks = greedy_tokens(fq)
    used_l = sorted({257 + len_code(t[0]) for t in toks if not isinstance(t, int)})
    # 15-bit codes in the literal tree (the text's own symbols at the bottom of a chain); codes one bit past each table's index
    for L in (15, 11, 10, 9):
        add("lit_chain_%d" % L, [Block("dynamic", tokens=toks, final=True, lit_lens=chain_lengths(syms + used_l + [256], 286, L))])
    # distances: every distance code used, the tree as deep as 15, 9 and 8 bits (GPU index 9, host index 8)
    fa = fasta_history(rng, 40000, b">d")
    for L in (15, 9, 8, 10):
        add("dist_chain_%d" % L, [Block("stored", data=fa[:30000]), Block("fixed", tokens=_lits(fa[30000:])),
                                   Block("dynamic", tokens=[(L2, d) for d in dist_bounds() for L2 in (3, 10, 258)], final=True,
                                         dist_lens=chain_lengths(list(range(30)), 30, L))])
    # one distance code of length 1 (zlib's one incomplete code); no distance code at all
    q = b"@a\n" + b"ACGT" * 500 + b"\n+\n" + b"I" * 2000 + b"\n"
    qt = greedy_tokens(q, max_dist=1)
    one = [0] * 30
    one[0] = 1
    add("dist_single_len1", [Block("dynamic", tokens=qt, final=True, dist_lens=one, hdist=1)])
    far = [0] * 30
    far[29] = 1
    farh = fasta_history(rng, 32768, b">far")
    add("dist_single_len1_far", [Block("stored", data=farh), Block("dynamic", tokens=[(258, 32768 - 7), (3, 24577)] * 8, final=True,
                                                                   dist_lens=far)])
    add("dist_none", [Block("dynamic", tokens=_lits(fq[:5000]), final=True, dist_lens=[0], hdist=1)])
    add("dist_none_untrimmed", [Block("dynamic", tokens=_lits(fq[:5000]), final=True, dist_lens=[0] * 30, hdist=30)])
    # a literal/length code of two symbols: the end of block and one length code; the text is matches into a stored block
    rec = b">x\nACGTTGCA\n"
    two = [0] * 286
    two[256] = two[257 + len_code(24)] = 1
    dl = [0] * 30
    dl[dist_code(12)] = 1
    add("lit_two_symbols", [Block("stored", data=rec), Block("dynamic", tokens=[(24, 12)] * 400, final=True, lit_lens=two, dist_lens=dl)])
    # HLIT = 286 and HDIST = 30 with unused zero lengths, split and cross-boundary runs
    for runs in ("split", "cross", "none"):
        add("untrimmed_%s" % runs, [Block("dynamic", tokens=greedy_tokens(fq[:20000], max_len=100, min_dist=5), final=True, hlit=286,
                                          hdist=30, runs=runs)])
    # HCLEN 5 .. 19: every literal/length code of 8 bits (the code-length code needs 16, 17 or 18, 0 and 8 only)
    eight = [8] * 256 + [0] * 30
    eight[255] = 0
    eight[256] = 8
    for h in range(5, 20):
        add("hclen_%d" % h, [Block("dynamic", tokens=_lits(fq[:3000]), final=True, lit_lens=eight, dist_lens=[0], hdist=1, hclen=h)])
    # repeats 16, 17, 18 at their least and most: zero runs of 3, 10, 11 and 138, equal lengths in runs of 4 and 7
    fa2 = fasta_history(rng, 8000, b">h")
    zeros = set(range(0, 10)) | set(range(11, 14)) | set(range(15, 26)) | set(range(105, 243))
    sl = _shaped_lit_lens(set(fa2), zeros)
    cl = _cl_runs(sl + [0])
    assert {(17, 0), (17, 7), (18, 0), (18, 127)} <= set(cl), cl
    add("repeat_extremes", [Block("dynamic", tokens=_lits(fa2), final=True, lit_lens=sl, dist_lens=[0], hdist=1)])
    add("repeat16_extremes", [Block("dynamic", tokens=_lits(fa2[:2000]), final=True, lit_lens=sl, dist_lens=[0], hdist=1,
                                    cl_tokens=_runs16(sl) + [(0, 0)])])
    # a run across the tree boundary: the literal tree's zero tail and the distance tree's zero head, one 18
    xt = greedy_tokens(fq[:20000], max_len=100, min_dist=5)
    add("cross_boundary_zeros", [Block("dynamic", tokens=xt, final=True, hlit=286, hdist=30, runs="cross")])
    # every length code at both ends, against every distance code's bounds (distance 32768 among them)
    cases += _matrix_members(rng)
    # overlapping matches at distances 1 .. 65, lengths up to 258
    ov = _lits(b">o\n" + b"ACGTTTGCAAGTCCGATGACGTACGTTAGCATGCATCGATCGTAGCTAGCTAGCATCGATGCATGCTAGC\n")
    ov += [(L, d) for d in range(1, 66) for L in (3, d + 1 if d < 257 else 258, 258) if 3 <= L <= 258]
    add("overlap_1_65", [Block("dynamic", tokens=ov, final=True)])
    # matches that reach back across earlier blocks, a stored one among them
    a, b_, c = fasta_history(rng, 9000, b">a"), fasta_history(rng, 7000, b">b"), fasta_history(rng, 5000, b">c")
    back = [(258, 20000), (100, 16000 + 7), (30, 9100), (77, 12345), (5, 21000 - 3)]
    add("back_across_blocks", [Block("stored", data=a), Block("fixed", tokens=_lits(b_)), Block("dynamic", tokens=_lits(c)),
                               Block("dynamic", tokens=back + _lits(b"\n>e\nACGT\n"), final=True)])
    # stored blocks of length 0 and of the largest size a bgzf member holds, starting at every bit offset
    for k in range(8):
        c13 = [c_ for c_ in range(8) if (2 + 5 * c_) % 8 == k][0]
        pre = Block("fixed", tokens=_lits(b">s\nA") + [(11, 1)] * c13 + _lits(b"\n"))
        head_bytes = (50 + 13 * c13 + 3 + 7) // 8 + 4
        pre_text = 5 + 11 * c13
        big = fasta_history(rng, min(65536 - 18 - 8 - head_bytes, MAX_BGZF_TEXT - pre_text), b">S")
        add("stored_max_at_bit_%d" % k, [pre, Block("stored", data=big, final=True)])
        add("stored_empty_at_bit_%d" % k, [pre, Block("stored", data=b""), Block("fixed", tokens=_lits(b">t\nACGT\n"), final=True)])
    # 2000 empty fixed blocks and 2000 empty stored blocks in one member
    many = [Block("fixed", tokens=_lits(b">f\nAC"))] + [Block("fixed") for _ in range(2000)] + [Block("stored") for _ in range(2000)]
    add("empty_blocks_4000", many + [Block("fixed", tokens=_lits(b"GT\n"), final=True)])
    # a final block of each type
    add("final_fixed", [Block("dynamic", tokens=toks[:2000]), Block("fixed", tokens=_lits(b"@z\nA\n+\nI\n"), final=True)])
    add("final_stored", [Block("dynamic", tokens=toks[:2000]), Block("stored", data=b"@z\nA\n+\nI\n", final=True)])
    add("final_dynamic", [Block("stored", data=b"@y\nC\n+\nI\n"), Block("dynamic", tokens=_lits(b"@z\nA\n+\nI\n"), final=True)])
    return cases


def _runs16(lens: Sequence[int]) -> List[Tuple[int, int]]:
    """The lengths with 16 at its least (3 copies) and most (6), as often as they fit: each run of equal nonzero lengths is sent as the
    length and then copies of 6, 3 and single lengths."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        i += r
        out.append((v, 0))
        r -= 1
        while v and r >= 3:
            k = 6 if r >= 6 else 3
            out.append((16, k - 3))
            r -= k
        out += [(v, 0)] * r
    assert (16, 0) in out and (16, 3) in out
    return out


def invalid_streams(seed: int = 12) -> List[Tuple[str, bytes, bytes, dict]]:
    """Streams that break one rule each: (name, text, raw, member keyword arguments).  The member carries the text's CRC-32 and ISIZE
    unless the case is about them, so only the decoder can tell; where a decoder that skips the rule can, the stream gives the text
    (a distance tree nobody reads, lengths nobody writes).  gzip.decompress refuses every one of them."""
    import numpy as np

    rng = np.random.default_rng(seed)
    fq = fastq_text(rng, 30, 150)
    syms = sorted(set(fq))
    lits = _lits(fq)
    cases = []

    def add(name, blocks, **kw):
        raw, text = deflate(blocks, check=False)
        cases.append((name, text, raw, kw))

    def dyn(**kw):
        kw.setdefault("dist_lens", [0])
        kw.setdefault("hdist", len(kw["dist_lens"]))
        return [Block("dynamic", tokens=lits, final=True, **kw)]

    # over-subscribed codes: the distance tree (nobody reads it), the literal/length tree (one unused symbol too many)
    add("oversub_dist", dyn(dist_lens=[1, 1, 1]))
    ll = limited_lengths([1 << 20 if s in syms or s == 256 else 0 for s in range(286)], 15)
    over = list(ll)
    over[285] = max(ll)
    add("oversub_lit", dyn(lit_lens=over))
    # incomplete codes: not zlib's single code of length 1
    add("incomplete_dist_one_len2", dyn(dist_lens=[2]))
    add("incomplete_dist_two_len2", dyn(dist_lens=[2, 2]))
    w = [1 << 20 if s in syms or s == 256 else 0 for s in range(286)]
    w[285] = 1
    inc = limited_lengths(w, 15)
    inc[285] = 0
    add("incomplete_lit", dyn(lit_lens=inc))
    cl_f = [0] * 19
    for s, _ in _cl_runs(ll) + [(0, 0)]:
        cl_f[s] += 1
    cl_f[18 if not cl_f[18] else 17 if not cl_f[17] else 1] = 1
    cl_inc = limited_lengths(cl_f, 7)
    cl_inc[18 if cl_f[18] == 1 else 17 if cl_f[17] == 1 else 1] = 0
    add("incomplete_codelength_code", dyn(lit_lens=ll, cl_lens=cl_inc))
    # too many symbols: HLIT > 286 (287, 288), HDIST > 30 (31, 32)
    add("hlit_287", dyn(lit_lens=ll, hlit=287))
    add("hlit_288", dyn(lit_lens=ll, hlit=288))
    add("hdist_31", dyn(lit_lens=ll, dist_lens=[0] * 31))
    add("hdist_32", dyn(lit_lens=ll, dist_lens=[0] * 32))
    # a repeat (16) with no previous length: the lengths start with three copies of "nothing"
    assert ll[0] == ll[1] == ll[2] == 0
    add("repeat16_first", dyn(lit_lens=ll, cl_tokens=[(16, 0)] + _cl_runs(ll[3:]) + [(0, 0)]))
    # no end-of-block code (the literals still decode; the block never ends)
    ne = limited_lengths([1 << 20 if s in syms else (1 if s == 255 else 0) for s in range(286)], 15)
    add("no_eob_code", dyn(lit_lens=ne, no_eob=True))
    # HCLEN 4: only 16, 17, 18 and 0 have code-length codes, so every length is 0 - no end-of-block code either
    add("hclen_4", [Block("dynamic", final=True, lit_lens=[0] * 257, dist_lens=[0], hdist=1, hclen=4,
                          cl_lens=[1] + [0] * 15 + [0, 2, 2], no_eob=True)])
    # a stored block whose NLEN is not the complement of LEN
    add("stored_bad_nlen", [Block("stored", data=fq, final=True, nlen=(~len(fq) & 0xFFFF) ^ 0x0100)])
    add("stored_bad_nlen_empty", [Block("stored", data=b"", nlen=0x0000), Block("stored", data=fq, final=True)])
    # a member whose trailer says CRC 0 and ISIZE 0 but whose stream holds text
    add("isize_zero", [Block("dynamic", tokens=greedy_tokens(fq), final=True)], crc=0, isize=0)
    # bytes between the final block and the trailer
    raw, text = deflate([Block("dynamic", tokens=greedy_tokens(fq), final=True)])
    cases.append(("junk_before_trailer", text, raw + b"\x00\x00\x00", {}))
    cases.append(("junk_before_trailer_fixed", text, deflate([Block("fixed", tokens=lits, final=True)])[0] + b"\x5a", {}))
    return cases


def truncated_dynamic(seed: int = 13) -> Tuple[bytes, bytes]:
    """(text, raw): a stream cut off inside its first dynamic block header (after the code-length code, in the lengths)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    fq = fastq_text(rng, 30, 150)
    raw, text = deflate([Block("dynamic", tokens=greedy_tokens(fq), final=True, runs="none")])
    return text, raw[:30]
