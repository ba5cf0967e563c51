"""CPU restatement of the find-unique-kmers step — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Two layers with different standing:

* ``analyze_histogram_rows`` follows the reference's own arithmetic (find_unique_kmers.py:132-168:
  first local minimum of the histogram, then the first count whose row drops below it) and is
  PINNED: tests/golden/unique_cutoffs.json was recorded from the real function.

* ``count_kmers`` / ``histogram_rows`` / ``unique_kmers`` restate what the KMC 3 tools the reference
  shells out to do at its settings (find_unique_kmers.py:82-90,123-129,186-194,218-225): canonical
  counting over both strands, k-mers with a symbol outside ACGT skipped, lower case = upper case,
  default -ci2 (k-mers seen once are not stored), -cs255 (counters saturate), kmers_subtract, dump
  with -ci/-cx in lexicographic order.  KMC is not in the reference checkout and not installed:
  PARITY WITH KMC IS UNPINNED; these functions pin the GPU path to this stated reading of it.

Pure Python: small inputs only.  ``count_kmers_np`` and the ``*_np`` functions beside it restate the
same three functions on numpy arrays for inputs of some Mbases to some hundred Mbases;
tests/test_unique_host.py holds them to the pure-Python ones.
"""
from collections import Counter
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")


def canonical(kmer: str) -> str:
    rc = kmer.translate(_COMP)[::-1]
    return kmer if kmer <= rc else rc


def count_kmers(reads: Iterable[str], k: int) -> Counter:
    """Occurrences of every canonical k-mer (uncapped, singletons included)."""
    c: Counter = Counter()
    for read in reads:
        s = read.upper()
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if all(ch in "ACGT" for ch in w):
                c[canonical(w)] += 1
    return c


def database(counts: Counter) -> Dict[str, int]:
    """What `kmc` leaves in its database: counter >= 2 (-ci2), saturated at 255 (-cs255)."""
    return {km: min(n, 255) for km, n in counts.items() if n >= 2}


def histogram_rows(db: Dict[str, int]) -> List[Tuple[int, int]]:
    """Rows of `kmc_tools transform db histogram`: (counter value, number of k-mers), values 1..255."""
    h = Counter(db.values())
    return [(c, h.get(c, 0)) for c in range(1, 256)]


class HistogramError(Exception):
    pass


def analyze_histogram_rows(rows: Iterable[Tuple[int, int]]) -> Tuple[int, int, bool]:
    """(min_coverage, max_coverage, warned) from histogram rows — find_unique_kmers.py:132-168."""
    min_cov, max_cov = False, False
    min_cov_count = None
    last = -1
    for coverage, count in rows:
        if coverage != 2:  # the row of count 2 is only remembered (:136)
            if not min_cov:
                if count > last:  # counts start rising: the row before is the local minimum (:140-143)
                    min_cov = coverage - 1
                    min_cov_count = last
            elif not max_cov:
                if count < min_cov_count:  # first row below the count at the minimum (:147-150)
                    max_cov = coverage
                    break
        last = count
    if not min_cov or not max_cov:  # 0 counts as "not found", as in the reference (:154)
        raise HistogramError()
    return min_cov, max_cov, (max_cov - min_cov < 5)


def unique_kmers(db_a: Dict[str, int], db_b: Dict[str, int], min_count: int, max_count: int) -> List[str]:
    """kmers_subtract then kmc_dump -ci -cx: k-mers of A not in B with min <= counter <= max, sorted."""
    return sorted(km for km, n in db_a.items() if km not in db_b and min_count <= n <= max_count)


# ---- the same on numpy arrays ---------------------------------------------------------------------
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def pack(reads: Iterable[str]) -> Tuple[np.ndarray, np.ndarray]:
    """(bases uint8 back to back, offsets uint64 n + 1) of ASCII reads: the batch layout of the C-ABI."""
    enc = [r.encode("ascii") for r in reads]
    offsets = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(b) for b in enc), dtype=np.uint64, count=len(enc)), out=offsets[1:])
    return np.frombuffer(b"".join(enc), dtype=np.uint8), offsets


def _merge(keys: np.ndarray, counts: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    if not keys.size:
        return keys, counts
    first = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
    return keys[first], np.add.reduceat(counts, first)


def count_kmers_np(bases: np.ndarray, offsets: np.ndarray, k: int, chunk: int = 1 << 23) -> Tuple[np.ndarray, np.ndarray]:
    """``count_kmers`` for a packed batch: (keys, counts), keys = the canonical k-mers as uint64 with base 0 in
    the top bits of the 2k (A < C < G < T: numeric order is lexicographic order), ascending; counts int64, uncapped."""
    assert 1 <= k <= 32
    bases = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    n = off.size - 1
    total = int(off[-1]) if n >= 0 else 0
    # every read followed by one invalid byte: no window spans two reads
    code = np.full(total + n, 4, dtype=np.uint8)
    lens = off[1:] - off[:-1]
    code[np.arange(total, dtype=np.int64) + np.repeat(np.arange(n, dtype=np.int64), lens)] = _CODE[bases[:total]]
    n_win = code.size - k + 1
    if n_win <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    bad = np.zeros(code.size + 1, dtype=np.int64)  # bad[i] = non-ACGT bytes before position i
    np.cumsum(code == 4, out=bad[1:])
    parts_k, parts_c = [], []
    for lo in range(0, n_win, chunk):
        hi = min(n_win, lo + chunk)
        c = (code[lo:hi + k - 1] & 3).astype(np.uint64)
        w = hi - lo
        fwd = np.zeros(w, dtype=np.uint64)
        rc = np.zeros(w, dtype=np.uint64)
        for j in range(k):
            b = c[j:j + w]
            fwd = (fwd << np.uint64(2)) | b
            rc |= (np.uint64(3) - b) << np.uint64(2 * j)
        ok = bad[lo + k:hi + k] == bad[lo:hi]
        u, cnt = np.unique(np.minimum(fwd, rc)[ok], return_counts=True)
        parts_k.append(u)
        parts_c.append(cnt.astype(np.int64))
    if len(parts_k) == 1:
        return parts_k[0], parts_c[0]
    return _merge(np.concatenate(parts_k), np.concatenate(parts_c))


def add_counts_np(a: Tuple[np.ndarray, np.ndarray], b: Tuple[np.ndarray, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """Counts of two batches together."""
    return _merge(np.concatenate((a[0], b[0])), np.concatenate((a[1], b[1])))


def histogram_np(counts: np.ndarray) -> np.ndarray:
    """hist[c], c = 1..255: distinct k-mers whose count capped at 255 is c (singletons included); hist[0]: all."""
    h = np.bincount(np.minimum(counts, 255), minlength=256).astype(np.int64)
    h[0] = counts.size
    return h


def unique_np(a: Tuple[np.ndarray, np.ndarray], b: Tuple[np.ndarray, np.ndarray], min_count: int, max_count: int) -> np.ndarray:
    """``unique_kmers(database(a), database(b), ...)`` as ascending keys."""
    ka, ca = a
    capped = np.minimum(ca, 255)
    keep = (ca >= 2) & (capped >= min_count) & (capped <= max_count)
    in_b = np.isin(ka, b[0][b[1] >= 2], assume_unique=True)
    return ka[keep & ~in_b]


def kmer_strings(keys: np.ndarray, k: int) -> List[str]:
    """The k-mers of such keys as text."""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.empty((keys.size, k), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        out[:, j] = lut[((keys >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.intp)]
    return [row.tobytes().decode() for row in out]


def read_list_np(path: str, k: int) -> np.ndarray:
    """A k-mer list file (one k-mer of k letters per line) as keys, in file order; raises if a line is malformed."""
    raw = np.fromfile(path, dtype=np.uint8)
    assert raw.size % (k + 1) == 0, "list file: wrong size for lines of k letters"
    rows = raw.reshape(-1, k + 1)
    assert (rows[:, k] == 10).all(), "list file: line not k letters long"
    c = _CODE[rows[:, :k]]
    assert (c < 4).all() and (rows[:, :k] < 96).all(), "list file: letter outside upper-case ACGT"
    keys = np.zeros(rows.shape[0], dtype=np.uint64)
    for j in range(k):
        keys = (keys << np.uint64(2)) | c[:, j].astype(np.uint64)
    return keys
