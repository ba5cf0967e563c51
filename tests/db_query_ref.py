"""The reference of the database query's tests: a plain Python loop over the windows of each sequence against a dict
{canonical k-mer: counter}, as oracle.unique_oracle.database leaves it.  Nothing here touches a device.
tests/test_host_assembly_qv.py holds `canonical` to the oracle's and the loop to oracle.count_kmers."""
import numpy as np

import kmerdb_files as kf

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def canonical(kmer):
    """the counter's rule: the lexicographic minimum of an upper-case k-mer and its reverse complement"""
    return min(kmer, revcomp(kmer))


def lex_rank(kmer):
    """a database's key: base 0 in the top bits of the 2k"""
    return sum("ACGT".index(c) << (2 * (len(kmer) - 1 - i)) for i, c in enumerate(kmer))


def window_kmers(sequence, k):
    """per window start 0 .. len - k: the canonical k-mer, or None for a window that is not clean (case folded)"""
    s = sequence.upper()
    return [canonical(s[i:i + k]) if all(c in "ACGT" for c in s[i:i + k]) else None for i in range(len(s) - k + 1)]


class Tally:
    """What a query session holds after some batches: histogram (256 rows, row 0 absent) and copies per k-mer of the database."""

    def __init__(self, db):
        self.db = db
        self.hist = np.zeros(256, dtype=np.uint64)
        self.copies = {}

    def add(self, sequences, k, min_count=2):
        """(per_read (n, 2) uint64, counts uint8 per base of the batch) of one batch, which is added to the tally"""
        per_read = np.zeros((len(sequences), 2), dtype=np.uint64)
        counts = np.zeros(sum(len(s) for s in sequences), dtype=np.uint8)
        at = 0
        for r, s in enumerate(sequences):
            for w, km in enumerate(window_kmers(s, k)):
                if km is None:
                    continue
                c = self.db.get(km, 0)
                per_read[r, 0] += 1
                per_read[r, 1] += c >= max(2, min_count)
                counts[at + w] = c
                self.hist[c] += 1
                if c:
                    self.copies[km] = self.copies.get(km, 0) + 1
            at += len(s)
        return per_read, counts

    def completeness(self, min_count=2, max_count=255):
        lo, hi = max(2, min_count), min(255, max_count)
        solid = [km for km, c in self.db.items() if lo <= c <= hi]
        return sum(1 for km in solid if km in self.copies), len(solid)

    def spectrum(self):
        spec = np.zeros((6, 256), dtype=np.uint64)
        for km, c in self.db.items():
            spec[min(self.copies.get(km, 0), 5), c] += 1
        return spec


def database_bytes(db, k, singletons=3):
    """the *.tbkdb file of a dict {canonical k-mer: counter 2..255}"""
    ranks = np.array(sorted(lex_rank(km) for km in db), dtype=np.uint64)
    by_rank = {lex_rank(km): c for km, c in db.items()}
    counts = np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = singletons
    hist[0] = ranks.size + singletons
    return kf.file_bytes(k, ranks, counts, hist, reads=1, bases=k)


def absent_stretches(counts, clean):
    """[(first, last)] of the maximal stretches of consecutive clean windows with counter 0: a loop"""
    out, start = [], None
    for w, ok in enumerate(clean):
        if ok and counts[w] == 0:
            if start is None:
                start = w
        elif start is not None:
            out.append((start, w - 1))
            start = None
    if start is not None:
        out.append((start, len(clean) - 1))
    return out

