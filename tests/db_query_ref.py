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


# ---- the same with numpy, for databases and batches that the loop above cannot follow -----------------------------------------
# tests/test_host_db_query_ref_np.py holds it to the loop on small inputs before it judges the device on large ones.
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i


def window_ranks(bases, offsets, k):
    """(rank, clean), one per base of the batch: the database key of the canonical k-mer of the window that starts there -
    the smaller of the forward and the reverse-complement rank, which is the lexicographic minimum - and whether the window is
    clean (k bases of ACGT, either case, inside one sequence).  rank is 0 where clean is False."""
    bases = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    total = int(off[-1]) if off.size else 0
    codes = _CODE[bases[:total]]
    bad = np.concatenate([[0], np.cumsum(codes == 255)])
    nw = max(total - k + 1, 0)
    clean = np.zeros(total, dtype=bool)
    rank = np.zeros(total, dtype=np.uint64)
    if not nw:
        return rank, clean
    clean[:nw] = bad[k:k + nw] == bad[:nw]
    left = np.repeat(off[1:], np.diff(off)) - np.arange(total)  # bases from here to the end of the sequence
    clean &= left >= k
    c = (codes & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        fwd |= c[j:j + nw] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[j:j + nw]) << np.uint64(2 * j)
    rank[:nw] = np.minimum(fwd, rc)
    rank[~clean] = 0
    return rank, clean


class TallyNp:
    """Tally for a database given as its sorted ranks and their counters: the same answers, from searchsorted and bincount."""

    def __init__(self, ranks, counters):
        self.ranks = np.asarray(ranks, dtype=np.uint64)
        self.counters = np.asarray(counters, dtype=np.uint8)
        assert self.ranks.size == self.counters.size and (self.ranks.size < 2 or (self.ranks[1:] > self.ranks[:-1]).all())
        self.hist = np.zeros(256, dtype=np.uint64)
        self.copies = np.zeros(self.ranks.size, dtype=np.uint64)

    def add(self, bases, offsets, k, min_count=2):
        """(per_read (n, 2) uint64, counts uint8 per base of the batch) of one batch, which is added to the tally"""
        off = np.asarray(offsets).astype(np.int64)
        rank, clean = window_ranks(bases, offsets, k)
        counts = np.zeros(rank.size, dtype=np.uint8)
        if self.ranks.size:
            at = np.minimum(np.searchsorted(self.ranks, rank), self.ranks.size - 1)
            hit = clean & (self.ranks[at] == rank)
            counts[hit] = self.counters[at[hit]]
            self.copies += np.bincount(at[hit], minlength=self.ranks.size).astype(np.uint64)
        self.hist += np.bincount(counts[clean], minlength=256).astype(np.uint64)
        before = np.zeros((rank.size + 1, 2), dtype=np.uint64)
        np.cumsum(clean, out=before[1:, 0])
        np.cumsum(clean & (counts >= max(2, min_count)), out=before[1:, 1])
        return before[off[1:]] - before[off[:-1]], counts

    def completeness(self, min_count=2, max_count=255):
        solid = (self.counters >= max(2, min_count)) & (self.counters <= min(255, max_count))
        return int((solid & (self.copies > 0)).sum()), int(solid.sum())

    def spectrum(self):
        spec = np.zeros((6, 256), dtype=np.uint64)
        np.add.at(spec, (np.minimum(self.copies, 5).astype(np.int64), self.counters.astype(np.int64)), 1)
        return spec
