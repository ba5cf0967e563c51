"""The GC x count matrix of a count database and the selection by GC content (include/tbk.h: tbk_kmerdb_gc_spectrum, the
min_gc / max_gc of tbk_select_options) restated with numpy on (ascending keys, counters).  A key is a lexicographic rank: base
0 in the top bits of the 2k, two bits a base, A, C, G, T = 0, 1, 2, 3.  The GC here is taken base by base - the two-bit
code is 1 or 2 - and not by the xor-and-popcount the library uses; tests/test_host_gc_spectrum.py holds it against counting
letters in the k-mer strings.  All integers, so what the tests compare with is exact."""
import numpy as np

import db_select_ref


def kmer_of(key: int, k: int) -> str:
    """the k-mer a rank stands for"""
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def rank_of(kmer: str) -> int:
    """kmer_of's inverse (any k up to 32; bits above 2k stay 0)"""
    rank = 0
    for base in kmer:
        rank = (rank << 2) | "ACGT".index(base)
    return rank


def gc_of(keys) -> np.ndarray:
    """the G-or-C bases of every key, int64; bits above 2k are zero and count as A"""
    keys = np.asarray(keys, dtype=np.uint64)
    total = np.zeros(keys.shape, dtype=np.int64)
    for i in range(32):
        code = (keys >> np.uint64(2 * i)) & np.uint64(3)
        total += ((code == 1) | (code == 2)).astype(np.int64)
    return total


def gc_spectrum(keys, counts, k: int) -> np.ndarray:
    """(k + 1, 256) uint64: cell [g, c] = the entries with g G-or-C bases and counter c"""
    g, c = gc_of(keys), np.asarray(counts, dtype=np.int64)
    assert g.size == c.size and (g.size == 0 or int(g.max()) <= k)
    return np.bincount(g * 256 + c, minlength=(k + 1) * 256).astype(np.uint64).reshape(k + 1, 256)


def select(base_keys, base_counts, base_range=(1, 255), partners=(), rule=db_select_ref.BASE, gc=(0, 32)):
    """db_select_ref.select of the entries of base whose GC lies in gc = (lo, hi), inclusive; the counter a kept entry gets
    depends on that entry alone, so dropping entries before the selection or after it is the same"""
    base_keys, base_counts = np.asarray(base_keys, dtype=np.uint64), np.asarray(base_counts, dtype=np.uint8)
    assert 0 <= gc[0] <= gc[1] <= 32
    g = gc_of(base_keys)
    inside = (g >= gc[0]) & (g <= gc[1])
    return db_select_ref.select(base_keys[inside], base_counts[inside], base_range, partners, rule)
