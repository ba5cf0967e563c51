"""A count database too large for a dict, for the references that ask theirs only for `db.get(kmer, 0)` (repair_ref,
screen_ref): a read-only mapping over (sorted ranks, counters) that answers through db_query_ref.lex_rank and np.searchsorted.
The keys are canonical k-mers as upper-case strings, as in the dicts it stands in for.  tests/test_host_rank_db.py holds it to
a plain dict.  Nothing here touches a device."""
import numpy as np

import db_query_ref as ref


class RankDb:
    def __init__(self, ranks, counters, k):
        self.ranks = np.asarray(ranks, dtype=np.uint64)
        self.counters = np.asarray(counters, dtype=np.uint8)
        self.k = k
        assert self.ranks.size == self.counters.size and (self.ranks.size < 2 or (self.ranks[1:] > self.ranks[:-1]).all())

    def _at(self, kmer):
        """the entry of a k-mer string, or -1"""
        if len(kmer) != self.k or not self.ranks.size:
            return -1
        rank = np.uint64(ref.lex_rank(kmer))
        at = int(np.searchsorted(self.ranks, rank))
        return at if at < self.ranks.size and self.ranks[at] == rank else -1

    def get(self, kmer, default=None):
        at = self._at(kmer)
        return default if at < 0 else int(self.counters[at])

    def __getitem__(self, kmer):
        at = self._at(kmer)
        if at < 0:
            raise KeyError(kmer)
        return int(self.counters[at])

    def __contains__(self, kmer):
        return self._at(kmer) >= 0

    def __len__(self):
        return int(self.ranks.size)


def kmer_string(rank, k):
    """the k-mer of a rank: base 0 from the top bits"""
    return "".join("ACGT"[(int(rank) >> (2 * (k - 1 - i))) & 3] for i in range(k))
