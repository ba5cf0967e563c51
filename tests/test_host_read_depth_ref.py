"""tests/read_depth_ref.py, the judge of the read depth's device tests, held to a second formulation - a 256-row count array walked
by its cumulative sum, and numpy.quantile(method="lower") where the windows are few enough for its floats to be exact - to
hand-worked records for 1, 2, 3, 4, 5, 8 and 9 clean windows, and its splitmix64 to the known answers.  No device."""
import numpy as np
import pytest

import db_query_ref as ref
import read_depth_ref as rd


def _by_counts(counters, m):
    """the same record from a count array: the value at a rank is the first row at which the cumulative sum passes it"""
    rows = np.zeros(256, dtype=np.int64)
    for c in counters:
        if c is not None:
            rows[c if c >= m else 0] += 1
    clean = int(rows.sum())
    if not clean:
        return (0,) * 10
    running = np.cumsum(rows)
    at = lambda rank: int(np.searchsorted(running, rank, side="right"))  # noqa: E731  (the first row with running > rank)
    present = clean - int(rows[0])
    there = np.cumsum(rows[1:])
    middle = 1 + int(np.searchsorted(there, (present - 1) // 2, side="right")) if present else 0
    return (clean, present, int(rows[255]), int((rows * np.arange(256)).sum()), *[at(j * (clean - 1) // 4) for j in range(5)], middle)


def _by_quantile(counters, m):
    d = np.array(rd.depths(counters, m), dtype=np.int64)
    assert 0 < d.size < 1 << 20  # (a rank q (n - 1) in doubles: exact far beyond this)
    there = d[d >= 1]
    return (int(d.size), int(there.size), int((d == 255).sum()), int(d.sum()),
            *[int(np.quantile(d, j / 4, method="lower")) for j in range(5)], int(np.quantile(there, 0.5, method="lower")) if there.size else 0)


# clean windows -> the ranks floor(j (clean - 1) / 4), j = 0..4, worked by hand
RANKS = {1: (0, 0, 0, 0, 0), 2: (0, 0, 0, 0, 1), 3: (0, 0, 1, 1, 2), 4: (0, 0, 1, 2, 3), 5: (0, 1, 2, 3, 4), 8: (0, 1, 3, 5, 7), 9: (0, 2, 4, 6, 8)}

#   counters (None: not clean), m, the record:            clean present saturated sum  lowest q1 median q3 highest present_median
HAND = [
    ([7], 1,                                               (1, 1, 0, 7,      7, 7, 7, 7, 7,         7)),
    ([None, 0, None, 9], 1,                                (2, 1, 0, 9,      0, 0, 0, 0, 9,         9)),
    ([255, 3, 0], 1,                                       (3, 2, 1, 258,    0, 0, 3, 3, 255,       3)),
    ([5, 1, 9, 7], 2,                                      (4, 3, 0, 21,     0, 0, 5, 7, 9,         7)),   # the 1 is below m: depth 0
    ([10, 50, 30, 20, 40], 1,                              (5, 5, 0, 150,    10, 20, 30, 40, 50,    30)),
    ([8, 7, 6, 5, 4, 3, 2, 1], 1,                          (8, 8, 0, 36,     1, 2, 4, 6, 8,         4)),
    ([0, 255, 0, None, 4, 0, 255, 0, 6, 0], 1,             (9, 4, 2, 520,    0, 0, 0, 6, 255,       6)),   # median 0, present_median not
    ([2, 2, 2, 2], 3,                                      (4, 0, 0, 0,      0, 0, 0, 0, 0,         0)),   # every counter below m
    ([None, None], 1,                                      (0,) * 10),
    ([], 1,                                                (0,) * 10),
    ([255] * 5, 255,                                       (5, 5, 5, 1275,   255, 255, 255, 255, 255, 255)),
    ([254, 255], 255,                                      (2, 1, 1, 255,    0, 0, 0, 0, 255,       255)),
]


def test_the_ranks_by_hand():
    for clean, ranks in RANKS.items():
        assert tuple(j * (clean - 1) // 4 for j in range(5)) == ranks
        v = list(range(100, 100 + clean))  # distinct depths: the record names its ranks
        assert rd.record(v[::-1], 1)[4:9] == tuple(v[r] for r in ranks), clean


@pytest.mark.parametrize("counters, m, want", HAND)
def test_hand_worked_records(counters, m, want):
    assert rd.record(counters, m) == want
    assert _by_counts(counters, m) == want
    if want[0]:
        assert _by_quantile(counters, m) == want


def test_the_reference_against_the_second_formulation():
    rng = np.random.default_rng(28)
    for trial in range(300):
        n = int(rng.integers(0, 40)) if trial % 3 else int(rng.integers(200, 1500))
        kind = trial % 5
        if kind == 0:
            values = rng.integers(0, 256, n)
        elif kind == 1:
            values = rng.choice([0, 30, 31, 255], n)
        elif kind == 2:
            values = np.where(rng.random(n) < 0.7, 0, rng.integers(1, 256, n))  # mostly absent
        elif kind == 3:
            values = np.full(n, int(rng.integers(0, 256)))
        else:
            values = np.clip(rng.normal(40, 6, n).astype(np.int64), 0, 255)
        counters = [None if rng.random() < 0.1 else int(v) for v in values]
        for m in (1, 2, 31, 255):
            got = rd.record(counters, m)
            assert got == _by_counts(counters, m), (trial, m)
            if got[0]:
                assert got == _by_quantile(counters, m), (trial, m)
            assert got[0] >= got[1] >= got[2] and got[4] <= got[5] <= got[6] <= got[7] <= got[8]
            assert got[9] >= got[6] and (got[9] == 0) == (got[1] == 0)


def test_records_from_sequences():
    """the whole path: sequences, canonical k-mers, the floor of a solid and of a full database"""
    k = 3
    db = {ref.canonical("ACG"): 7, ref.canonical("GTA"): 1}
    sequences = ["ACGTAC", "acgta", "ACNGT", "", "AC", "TACGT"]  # ACG CGT GTA TAC | acg cgt gta | - | - | - | TAC ACG CGT
    # (CGT is ACG's reverse complement and TAC is GTA's)
    assert rd.window_counters(db, sequences, k) == [[7, 7, 1, 1], [7, 7, 1], [None, None, None], [], [], [1, 7, 7]]
    assert rd.read_depth(db, sequences, k, floor=1)[0] == (4, 4, 0, 16, 1, 1, 1, 7, 7, 1)
    assert rd.read_depth(db, sequences, k)[0] == (4, 2, 0, 14, 0, 0, 0, 7, 7, 7)  # a solid database's floor: the 1s read as 0
    assert rd.read_depth(db, sequences, k, min_count=8, floor=1)[0] == (4, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert rd.read_depth(db, sequences, k)[2:5] == [(0,) * 10] * 3
    arr = rd.as_array(rd.read_depth(db, sequences, k))
    assert arr.dtype.itemsize == 40 and arr[0].tobytes() == bytes([4, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                                                   14, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 7, 7, 0, 0])


def test_splitmix64_known_answers():
    assert [rd.draw(0, i) for i in range(3)] == [3793791033, 1853398634, 113532184]
    assert rd.splitmix64(0, 1) == 0xE220A8397B1DCDAF  # the generator's published first output from state 0
    assert rd.draw(5, 0) == rd.splitmix64(5, 1) >> 32 and rd.draw((1 << 64) - 1, 0) == rd.splitmix64(0x9E3779B97F4A7C14, 0) >> 32  # the state wraps


def test_the_rule_in_integers():
    #      clean present saturated sum lowest q1 median q3 highest present_median
    rec = lambda s: (10, 10, 0, 10 * s, s, s, s, s, s, s)  # noqa: E731
    assert rd.bin_of((0,) * 10, 0) == "U" and rd.bin_of((0,) * 10, 0, min_depth=5, target=1) == "U"
    assert [rd.bin_of(rec(s), 0, min_depth=3, max_depth=40) for s in (0, 2, 3, 40, 41, 255)] == list("BBAABB")
    # u(0, 0) = 3793791033 of 2^32: a read of depth s is kept at target T when u s < T 2^32, that is T / s > 0.8833...
    assert [rd.bin_of(rec(100), 0, target=t) for t in (88, 89, 100, 120)] == list("BAAA")
    assert rd.bin_of(rec(100), 2, target=3) == "A"  # u(0, 2) = 113532184 of 2^32 = 0.0264...
    assert rd.bin_of(rec(100), 2, target=2) == "B"
    assert rd.bin_of(rec(20), 0, target=20) == "A" and rd.bin_of(rec(21), 0, target=20, max_depth=20) == "B"
    assert rd.bin_of((10, 3, 0, 90, 0, 0, 0, 40, 50, 40), 0, min_depth=1) == "B"
    assert rd.bin_of((10, 3, 0, 90, 0, 0, 0, 40, 50, 40), 0, by="present-median", min_depth=1) == "A"
    recs = [rec(60)] * 4000
    kept = rd.bins_of(recs, target=30).count("A")
    assert 1850 < kept < 2150  # half of them, give or take: the draws are uniform
    assert rd.bins_of(recs, target=30) != rd.bins_of(recs, target=30, seed=1)
