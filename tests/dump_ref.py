"""The counted-dump rule of include/tbk.h restated with Python and numpy: what tests/test_gpu_kmerdb_dump.py and
tests/test_gpu_dump_cli.py hold the device to, itself held to the oracle's counter by tests/test_host_dump_ref.py.
A helper, not a test."""
import numpy as np

from oracle.unique_oracle import canonical, kmer_strings

import kmerdb_files as kf

# the reasons a line is refused by, in the words of the library's message ("<file>: line <n>: <reason>")
TOO_LONG = "line too long"
EMPTY = "empty line"
SHORT_KMER = "the k-mer is shorter than k"
NOT_ACGT = "a byte of the k-mer is not one of ACGT (upper case)"
NO_COUNTER = "no separator and no counter behind the k-mer"
LONG_KMER = "the k-mer is longer than k"
NO_SEPARATOR = "no tab or space behind the k-mer"
EMPTY_COUNTER = "the counter is empty"
NOT_DIGITS = "the counter is not a decimal number"
TOO_MANY_DIGITS = "the counter has more than 32 digits"
ZERO = "the counter is 0"
NOT_COMPRESSED = "it is not homopolymer-compressed"


class DumpError(ValueError):
    def __init__(self, line_no, reason):
        super().__init__("line {}: {}".format(line_no, reason))
        self.line_no, self.reason = line_no, reason


def rank(kmer: str) -> int:
    """The lexicographic rank of a k-mer as the database stores it: base 0 in the top bits of the 2k."""
    v = 0
    for ch in kmer:
        v = (v << 2) | "ACGT".index(ch)
    return v


def parse_line(line: bytes, k: int, compressed: bool = False):
    """(rank of the canonical k-mer, counter saturated at 255) of one line without its newline, or the reason it is refused
    by: the first thing wrong, reading from the left."""
    if len(line) > k + 35:
        return TOO_LONG
    if not line:
        return EMPTY
    for c in line[:k]:
        if c in b"\t ":
            return SHORT_KMER
        if c not in b"ACGT":
            return NOT_ACGT
    if len(line) < k:
        return SHORT_KMER
    if len(line) == k:
        return NO_COUNTER
    if line[k] not in b"\t ":
        return LONG_KMER if line[k] in b"ACGT" else NO_SEPARATOR
    digits = line[k + 1:]
    if not digits:
        return EMPTY_COUNTER
    if any(c not in b"0123456789" for c in digits):
        return NOT_DIGITS
    if len(digits) > 32:
        return TOO_MANY_DIGITS
    value = int(digits)
    if value == 0:
        return ZERO
    kmer = line[:k].decode()
    if compressed and any(a == b for a, b in zip(kmer, kmer[1:])):
        return NOT_COMPRESSED
    return rank(canonical(kmer)), min(value, 255)


def lines_of(text: bytes):
    """The lines of a file: the last one may lack its newline, an empty file has none."""
    if not text:
        return []
    lines = text.split(b"\n")
    return lines[:-1] if text.endswith(b"\n") else lines


def parse(text: bytes, k: int, compressed: bool = False):
    """(keys uint64, counts uint8) of one file's text, a pair per line in file order; raises DumpError(line_no, reason) for
    the first line that breaks the rule."""
    keys, counts = [], []
    for no, line in enumerate(lines_of(text), 1):
        got = parse_line(line, k, compressed)
        if isinstance(got, str):
            raise DumpError(no, got)
        keys.append(got[0])
        counts.append(got[1])
    return np.array(keys, dtype=np.uint64), np.array(counts, dtype=np.uint8)


def fold(keys, counts):
    """Ascending distinct keys with min(255, sum) of their counters."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.int64)
    if not keys.size:
        return keys, np.zeros(0, dtype=np.uint8)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    first = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
    return keys[first], np.minimum(np.add.reduceat(counts, first), 255).astype(np.uint8)


def database(keys, counts, floor="auto"):
    """(keys, counters, hist, floor) of the database the pairs make: folded; floor 1 keeps every entry (row 0 = n), floor 2
    leaves the ones out of the entries and in row 1 (row 0 = distinct keys); auto is 1 when a folded 1 exists."""
    keys, counters = fold(keys, counts)
    hist = np.bincount(counters, minlength=256).astype(np.uint64)
    assert hist[0] == 0
    hist[0] = keys.size
    if floor == "auto":
        floor = 1 if hist[1] else 2
    if floor == 2:
        keep = counters >= 2
        keys, counters = keys[keep], counters[keep]
    return keys, counters, hist, floor


def magic(floor: int, compressed: bool = False) -> bytes:
    return {(2, False): b"TBKKMDB1", (2, True): b"TBKKMDH1", (1, False): b"TBKKMFB1", (1, True): b"TBKKMFH1"}[(floor, compressed)]


def database_bytes(texts, k, floor="auto", compressed=False, reads=0, bases=0) -> bytes:
    """The *.tbkdb file of the database that the files' texts make, read as one text."""
    parsed = [parse(t, k, compressed) for t in texts]
    keys = np.concatenate([p[0] for p in parsed]) if parsed else np.zeros(0, dtype=np.uint64)
    counts = np.concatenate([p[1] for p in parsed]) if parsed else np.zeros(0, dtype=np.uint8)
    keys, counters, hist, floor = database(keys, counts, floor)
    return kf.file_bytes(k, keys, counters, hist, reads=reads, bases=bases, magic=magic(floor, compressed))


def format(keys, counters, k, lo=1, hi=255) -> bytes:  # noqa: A001  (the name the issue gives it)
    """`kmc_dump -ciLO -cxHI`: KMER<tab>COUNT<newline> in the keys' order for the entries with a counter in [lo, hi]."""
    keys = np.asarray(keys, dtype=np.uint64)
    counters = np.asarray(counters)
    keep = (counters >= lo) & (counters <= hi)
    return "".join("{}\t{}\n".format(s, int(c)) for s, c in zip(kmer_strings(keys[keep], k), counters[keep])).encode()


def revcomp(kmer: str) -> str:
    return kmer.translate(str.maketrans("ACGT", "TGCA"))[::-1]
