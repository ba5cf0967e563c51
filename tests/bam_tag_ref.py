"""The haplotag rule of include/tbk.h ("Haplotag output") in plain Python, written from the rule and not from the C++: the
walker of a record's aux area, the rewrite of one record and of a run, and the crafted records the host, sanitizer and
device tests share.  Records come from ``bam_craft``; a tag block is bytes."""
import random
import struct

import bam_craft as bc

MAX_RECORD = bc.MAX_RECORD
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
ELEMENT = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
DROPPED = (b"HP", b"ka", b"kb")

# the reasons, as words that occur in tbk_last_error()
SHORT_FIELD = "fewer than 3 bytes"
TYPE = "unknown type"
SUBTYPE = "unknown subtype"
NEG_COUNT = "negative count"
PAST_END = "runs past the record's end"
NO_NUL = "without a NUL"
TWICE = {b"HP": "second tag field named HP", b"ka": "second tag field named ka", b"kb": "second tag field named kb"}
LONG = "larger than TBK_BAM_MAX_RECORD"


class TagError(ValueError):
    def __init__(self, why, record_no=None):
        super().__init__(why)
        self.why, self.record_no = why, record_no


def aux_start(rec):
    l_name, n_cigar, _flag, l_seq = rec[12], *struct.unpack_from("<HHI", rec, 16)
    return 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def fields(rec):
    """[(start, end, name)] of the aux fields of one record (bytes, block_size field included); TagError by the rule."""
    end = 4 + struct.unpack_from("<I", rec, 0)[0]
    at, out, seen = aux_start(rec), [], set()
    assert at <= end <= len(rec)
    while at < end:
        if end - at < 3:
            raise TagError(SHORT_FIELD)
        name, kind, v = rec[at:at + 2], chr(rec[at + 2]), at + 3
        if kind in FIXED:
            size = FIXED[kind]
        elif kind in "ZH":
            nul = rec.find(b"\0", v, end)
            if nul < 0:
                raise TagError(NO_NUL)
            size = nul + 1 - v
        elif kind == "B":
            if end - v < 5:
                raise TagError(PAST_END)
            sub = chr(rec[v])
            if sub not in ELEMENT:
                raise TagError(SUBTYPE)
            (count,) = struct.unpack_from("<i", rec, v + 1)
            if count < 0:
                raise TagError(NEG_COUNT)
            size = 5 + count * ELEMENT[sub]
        else:
            raise TagError(TYPE)
        if v + size > end:
            raise TagError(PAST_END)
        if name in DROPPED:
            if name in seen:
                raise TagError(TWICE[name])
            seen.add(name)
        out.append((at, v + size, name))
        at = v + size
    return out


def retag(rec, which, a, b):
    """the tagged record; `which` is one of "ABU" """
    end = 4 + struct.unpack_from("<I", rec, 0)[0]
    body = rec[4:aux_start(rec)] + b"".join(rec[s:e] for s, e, name in fields(rec) if name not in DROPPED)
    if which == "A":
        body += b"HPC\x01"
    elif which == "B":
        body += b"HPC\x02"
    body += b"kaI" + struct.pack("<I", a) + b"kbI" + struct.pack("<I", b)
    if len(body) > MAX_RECORD:
        raise TagError(LONG)
    assert len(body) <= end - 4 + 18
    return struct.pack("<i", len(body)) + body


def retag_all(records, bins, counts):
    """(the tagged records back to back, out_off) of a list of record bytes; TagError names the first bad record"""
    out, off = bytearray(), [0]
    for i, rec in enumerate(records):
        try:
            out += retag(rec, bins[i], counts[i][0], counts[i][1])
        except TagError as exc:
            raise TagError(exc.why, i)
        off.append(len(out))
    return bytes(out), off


def tags_of(rec):
    """{name: (type, raw value bytes)} of a record's aux fields (the end-to-end test reads HP, ka and kb with it)"""
    return {name: (chr(rec[s + 2]), rec[s + 3:e]) for s, e, name in fields(rec)}


# ---- crafted tag fields ----
def field(name, kind, value=b""):
    return name.encode() + kind.encode() + value


def b_array(name, sub, count, rng=None):
    body = bytes((rng.randrange(256) if rng else i & 0xFF) for i in range(count * ELEMENT[sub]))
    return field(name, "B", sub.encode() + struct.pack("<i", count) + body)


def every_type():
    """one field of every type: B with each subtype and with count 0, an empty Z, an H"""
    out = [field("aA", "A", b"x"), field("ac", "c", b"\xff"), field("aC", "C", b"\x07"), field("as", "s", b"\x01\x80"), field("aS", "S", b"\xff\xff"),
           field("ai", "i", struct.pack("<i", -5)), field("aI", "I", struct.pack("<I", 4000000000)), field("af", "f", struct.pack("<f", 0.5)),
           field("aZ", "Z", b"text with spaces\0"), field("eZ", "Z", b"\0"), field("aH", "H", b"1AE301\0"), field("eH", "H", b"\0")]
    for sub in "cCsSiIf":
        out.append(b_array("b" + sub, sub, 3))
        out.append(b_array("z" + sub, sub, 0))
    return out


HP_FORMS = [field("HP", k, v) for k, v in (("c", b"\x01"), ("C", b"\x02"), ("s", b"\x01\x00"), ("S", b"\x02\x00"), ("i", struct.pack("<i", 1)),
                                           ("I", struct.pack("<I", 2)), ("Z", b"one\0"))]
COUNTS = [(0, 0), (1, 2), (2 ** 31 - 1, 0), (0, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1), (12345, 678)]


def _rec(name, seq_len, tags, rng, flag=4, qual=True):
    seq = "".join(rng.choices("ACGT", k=seq_len))
    return bc.encode(bc.record(name, seq, [rng.randrange(2, 94) for _ in range(seq_len)] if qual else None, flag=flag, tags=tags))


def crafted(seed=5):
    """The records of the issue's list that are small: every aux type; HP first, in the middle, last and alone; HP, ka and kb in all
    six orders; HP in every stored form; the smallest record; name lengths 1..40 with l_seq 1..3 (every residue mod 16 of sizes and
    offsets); a record without quality, a reverse-strand one, one with cigar operations.  Returns (records, bins, counts)."""
    import itertools

    rng = random.Random(seed)
    other = every_type()
    recs = [_rec("all", 33, b"".join(other), rng)]
    hp = HP_FORMS[1]
    recs.append(_rec("hp_first", 20, hp + other[0] + other[8], rng))
    recs.append(_rec("hp_middle", 21, other[8] + hp + other[12], rng))
    recs.append(_rec("hp_last", 22, other[3] + other[10] + hp, rng))
    recs.append(_rec("hp_only", 23, hp, rng))
    ka, kb = field("ka", "I", struct.pack("<I", 99)), field("kb", "i", struct.pack("<i", 77))
    for order in itertools.permutations((hp, ka, kb)):
        recs.append(_rec("order", 9, other[8] + order[0] + other[13] + order[1] + order[2] + other[5], rng))
    for order in itertools.permutations((hp, ka, kb)):
        recs.append(_rec("packed", 5, b"".join(order), rng))     # the three side by side, and nothing else
    for form in HP_FORMS:
        recs.append(_rec("form", 12, other[9] + form + other[6], rng))
    recs.append(_rec("k", 1, b"", rng))                          # the smallest record
    for name_len in range(1, 41):
        for l_seq in (1, 2, 3):
            recs.append(_rec("n" * name_len, l_seq, (hp if (name_len + l_seq) % 3 == 0 else b"") + (other[name_len % len(other)] if name_len % 2 else b""), rng))
    recs.append(_rec("noqual", 40, other[8] + hp, rng, qual=False))
    recs.append(_rec("reverse", 41, ka + other[8], rng, flag=0x14))
    recs.append(bc.encode(bc.record("cigar", "ACGTACGTAC", [30] * 10, n_cigar=3, tags=kb + other[1])))
    bins = "".join("ABU"[i % 3] for i in range(len(recs)))
    counts = [COUNTS[i % len(COUNTS)] for i in range(len(recs))]
    return recs, bins, counts


def tiny(n=5000, seed=6):
    """n records of 51-70 bytes: many records per tile"""
    rng = random.Random(seed)
    hp = HP_FORMS[0]
    recs = [_rec("t%d" % (i % 97), 1 + i % 4, hp if i % 5 == 0 else (field("xs", "s", b"\x01\x02") if i % 5 == 1 else b""), rng) for i in range(n)]
    return recs, "".join(rng.choice("ABU") for _ in range(n)), [(rng.randrange(1000), rng.randrange(1000)) for _ in range(n)]


def big(seed=7):
    """One record larger than a 4096-byte tile, one larger than 64 KiB with kinetics B arrays and a 70 kB Z string, and records whose
    dropped field straddles a 16-byte vector boundary and a 4096-byte tile boundary of the input and the output: a 6000-byte Z
    named HP, and HP C fields pushed byte by byte across the boundary by a Z field in front of them."""
    rng = random.Random(seed)
    hp = HP_FORMS[1]
    recs = [_rec("tile", 3000, b_array("fi", "C", 3000, rng) + hp + field("MM", "Z", b"C+m," + b"1," * 900 + b";\0"), rng)]
    mm = b"C+m," + b",".join(str(rng.randrange(20)).encode() for _ in range(30000))
    mm = mm[:70000] + b";\0"
    recs.append(_rec("ont/big", 20000, b_array("fi", "C", 20000, rng) + field("ka", "I", b"\1\0\0\0") + b_array("ri", "S", 20000, rng) + field("MM", "Z", mm) + hp
                     + b_array("ML", "C", 5000, rng), rng))
    recs.append(_rec("longhp", 100, field("xx", "Z", b"q" * 3000 + b"\0") + field("HP", "Z", b"h" * 6000 + b"\0") + field("yy", "Z", b"r" * 3000 + b"\0"), rng))
    for pad in range(20):                        # the record sizes step the HP field across a 16-byte boundary ...
        recs.append(_rec("vec", 2, field("pd", "Z", b"p" * pad + b"\0") + hp + field("zz", "Z", b"s" * 40 + b"\0"), rng))
    for pad in range(4040, 4060, 3):             # ... and across a tile boundary of the input run
        recs.append(_rec("tileedge", 2, field("pd", "Z", b"p" * pad + b"\0") + hp + field("zz", "Z", b"s" * 100 + b"\0"), rng))

    def plan(n):
        return "".join("BAU"[i % 3] for i in range(n)), [COUNTS[(i + 1) % len(COUNTS)] for i in range(n)]

    # ... and records whose HP field's place is the first byte of an output tile, and 5 bytes into one: the tagged bytes in front
    # of them are counted, and the Z field in front of HP is as long as it takes
    for into in (0, 5):
        so_far = len(retag_all(recs, *plan(len(recs)))[0])
        probe = _rec("outedge", 2, field("pd", "Z", b"\0") + hp, rng)
        hole = so_far + len(probe) - len(hp)      # where HP's place would lie in the output with an empty pd
        pad = (into - hole) % 4096
        recs.append(_rec("outedge", 2, field("pd", "Z", b"p" * pad + b"\0") + hp + field("zz", "Z", b"s" * 100 + b"\0"), rng))
    return (recs,) + plan(len(recs))


def refused(seed=8):
    """[(what, tags, reason)]: a tag block that breaks the rule in one way each (the record's name and bases are sound)"""
    hp = HP_FORMS[1]
    ok = field("ok", "Z", b"fine\0")
    return [
        ("two bytes left", ok + b"ab", SHORT_FIELD),
        ("one byte left", ok + b"a", SHORT_FIELD),
        ("type", ok + field("ab", "q", b"\1\2\3\4"), TYPE),
        ("type lower z", field("ab", "z", b"x\0"), TYPE),
        ("subtype", ok + field("ab", "B", b"Z" + struct.pack("<i", 1) + b"\0"), SUBTYPE),
        ("negative count", field("ab", "B", b"C" + struct.pack("<i", -1)), NEG_COUNT),
        ("most negative count", field("ab", "B", b"i" + struct.pack("<i", -2 ** 31)), NEG_COUNT),
        ("i cut", ok + field("ab", "i", b"\1\2\3"), PAST_END),
        ("s cut", field("ab", "s", b"\1"), PAST_END),
        ("A without a value", field("ab", "A"), PAST_END),
        ("B header cut", field("ab", "B", b"C\1\0\0"), PAST_END),
        ("B array cut", field("ab", "B", b"S" + struct.pack("<i", 3) + b"\0" * 5), PAST_END),
        ("B count huge", field("ab", "B", b"i" + struct.pack("<i", 2 ** 31 - 1) + b"\0" * 8), PAST_END),
        ("Z without NUL", ok + field("ab", "Z", b"never ends" * 30), NO_NUL),
        ("H without NUL", field("ab", "H", b"AB"), NO_NUL),
        ("Z empty and cut", field("ab", "Z"), NO_NUL),
        ("HP twice", hp + ok + HP_FORMS[6], TWICE[b"HP"]),
        ("ka twice", field("ka", "I", b"\0" * 4) + field("ka", "C", b"\1"), TWICE[b"ka"]),
        ("kb twice", ok + field("kb", "Z", b"\0") + hp + field("kb", "Z", b"\0"), TWICE[b"kb"]),
    ]


def refused_record(tags, name="bad", seed=9):
    return _rec(name, 7, tags, random.Random(seed))


def too_long_record():
    """A record whose tagged form is 1 byte past TBK_BAM_MAX_RECORD: block_size = TBK_BAM_MAX_RECORD - 13 with one B array as its
    tags (256 MiB of zeros: built once, by multiplication)."""
    head = bc.encode(bc.record("huge", "A", [9]))
    room = MAX_RECORD - 13 - (len(head) - 4)
    tags = field("zz", "B", b"C" + struct.pack("<i", room - 8)) + bytes(room - 8)
    rec = struct.pack("<I", MAX_RECORD - 13) + head[4:] + tags
    assert len(rec) == 4 + MAX_RECORD - 13
    return rec
