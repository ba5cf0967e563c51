"""The k-mer counter behind find-unique-kmers (tbk_count_kernels.hip, tbk_count.cpp) at every kernel it can launch.

tbk_launch_count picks tbk_count_kernel<W, M64> from the table's bucket selection: W = 0 (plain) to 8 m-mers per span, m-mers of
up to 16 bases on the 32-bit path or 17 to 32 on the 64-bit one.  Which one a table gets follows from k and its capacity
(tbk_mz_params), and small test tables only ever get a few of them - never the 64-bit path, which is the one a table for a real
parental library takes.  TBK_COUNT_W, TBK_COUNT_M and TBK_COUNT_LOAD are read each time a table is allocated, so
the tests here pin them in-process, assert through KmerCounter.stats() that the table runs the (w, m, o) the case is about, and
compare counts, histograms and A-minus-B lists with oracle/unique_oracle.py's numpy counter - exactly: they are integers and strings.

  test_every_kernel_against_the_oracle   the (k, W, m) matrix, A and B often with different bucket selection
  test_pass_and_lane_boundaries          read ends and stream ends at every offset around a pass (2048) and a lane (32)
  test_saturation_and_cutoffs            counters of exactly 1, 2, 3, 254, 255, 256, 300 against B counters of 0, 1, 2
  test_load_and_growth                   TBK_COUNT_LOAD at and beyond its clamps, tables that start at 16 buckets
  test_multi_piece_add                   one add of four pieces (> 3 x 64 M window starts), the table growing between them
  test_multi_piece_add_in_passes         the same add with passes = 3: the rebuild between the pieces falls into class 0
  test_clamp_keeps_a_counter_below_the_carry   one counter past 2^32 window starts with seven witnesses in its bucket; with the
                                         table kernels' grid capped at one block too (the clamp's later trips)

The matrix runs W = 0 at k = 15, 21, 32, every W from 1 to 8 with m <= 16 (45 triples, m = 4 .. 16, and W = 9, which is clamped
to 8) and every W from 1 to 8 with m >= 17 (47 triples, m = 17 .. 32, and W = 9); the whole file takes 37 s on an MI355X, 27 s of
it the oracle's counts of the 202 Mbase library.

What the file notices, from libraries built with one error each (once, on an MI355X, against this file alone):
  the 64-bit branch of mmer_order reads the reverse strand at fsh     64 cases: 55 of the matrix (64-bit table on either side), 8 of
  the 64-bit path's hsel goes through tbk_scramble                    69 cases: 60 of the matrix ... load_and_growth, 1 of saturation
  the counting kernel leaves home with leaving_home = false           111 cases: 87 of the matrix, all 24 of load_and_growth
  raw >= 1 for raw >= 2 in the unique kernel                          126 cases, all four of saturation_and_cutoffs among them
  count_lookup(b) < 1 for < 2                                         125 cases, all four of saturation_and_cutoffs among them
  no clamp launch in counter_run                                      test_clamp_keeps_a_counter_below_the_carry
The first two and the last pass tests/test_gpu_unique.py.  An `ok` test without its "+ k" passes everything: load_chunk reads bytes
past `total` as not-ACGT and the separated stream ends in an 'N', so no window ever depended on it.
"""
import concurrent.futures
import os
import time

import numpy as np
import pytest

from oracle import unique_oracle as uo

pytestmark = pytest.mark.gpu

_RC = str.maketrans("ACGT", "TGCA")
_KNOBS = ("TBK_COUNT_W", "TBK_COUNT_M", "TBK_COUNT_LOAD")


def _rc(s):
    return s.translate(_RC)[::-1]


def _rand(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


class _Pinned:
    """A KmerCounter with the TBK_COUNT_* knobs pinned: they are put back before every call that may allocate a table (creation
    and every add - a table that grows asks again), and after each the table must run the bucket selection the case names.
    With passes > 1 a table is also rebuilt while the later classes are replayed - inside finish(), histogram(), unique() and
    database() - so those go through the helper too: pinned before, (w, m, o) checked after."""

    def __init__(self, mp, k, capacity, w=None, m=None, load=None, expect=None, passes=1, store_limit=0):
        from trio_binning_amd import kmers

        self.mp, self.k, self.expect, self.passes = mp, k, tuple(expect), passes
        self.env = dict(zip(_KNOBS, (w, m, load)))
        self._pin()
        self.c = kmers.KmerCounter(k, capacity, passes=passes, store_limit=store_limit)
        self.stats()

    def _pin(self):
        for name, v in self.env.items():
            if v is None:
                self.mp.delenv(name, raising=False)
            else:
                self.mp.setenv(name, str(v))

    def stats(self):
        st = self.c.stats()
        assert (st["w"], st["m"], st["o"], st["t"]) == self.expect + (0,), (self.k, self.env, st)
        return st

    def add(self, reads):
        self.add_packed(*uo.pack(reads))

    def add_packed(self, bases, offsets):
        self._pin()
        self.c.add(bases, offsets)
        self.stats()

    def finish(self):
        self._pin()
        self.c.finish()
        return self.stats()

    def histogram(self):
        self._pin()
        hist = self.c.histogram()
        self.stats()
        return hist

    def unique(self, other, lo, hi, out):
        """unique() of two counters in passes finishes both: `other` is finished under its own pins first, so that no table of
        its is rebuilt under this counter's."""
        if self.passes > 1:
            other.finish()
        self._pin()
        n = self.c.unique(other.c, lo, hi, out)
        self.stats()
        other.stats()
        return n

    def database(self):
        self._pin()
        db = self.c.database()
        self.stats()
        return db

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.c.close()


def _expect(k, w, m):
    """(w, m, o) of a table pinned to W = w, M = m: tbk_mz_params takes them unchanged when the span fits k with k's parity."""
    if w == 0:
        return (0, 0, 0)
    span = m + w - 1
    assert span <= k and (k - span) % 2 == 0, (k, w, m)
    return (w, m, (k - span) // 2)


def _compare(ca, cb, oa, ob, k, tmp_path, windows):
    """Distinct count, whole histogram and the A-minus-B lists of two counters against the oracle's counts (keys, counts)."""
    hist = ca.histogram()
    want = uo.histogram_np(oa[1])
    assert ca.stats()["distinct"] == oa[0].size
    assert [int(x) for x in hist] == [int(x) for x in want]
    for lo, hi in windows:
        out = str(tmp_path / f"u_{lo}_{hi}.txt")
        n = ca.unique(cb, lo, hi, out)
        got = uo.read_list_np(out, k)
        expected = uo.unique_np(oa, ob, lo, hi)
        assert n == got.size == expected.size and np.array_equal(got, expected), (k, lo, hi, n, expected.size)
        os.unlink(out)


# ---- 2. every kernel ------------------------------------------------------------------------------------------------
# (k, W, m): every W from 1 to 8 on either path; m = 16 beside m = 17 at neighbouring W (k = 21, 22, 32); m = 24 / 25 / 31 / 32;
# tiny m (4, 8), where a few hundred canonical m-mers share all the k-mers and nearly every key leaves its home bucket
_M32 = [
    (15, 1, 15), (16, 1, 16), (21, 1, 15), (32, 1, 16), (32, 1, 4), (22, 1, 8),
    (16, 2, 15), (21, 2, 16), (31, 2, 16), (19, 2, 12), (15, 2, 4), (27, 2, 8),
    (19, 3, 15), (22, 3, 16), (32, 3, 16), (16, 3, 4), (32, 3, 12),
    (21, 4, 16), (22, 4, 15), (31, 4, 16), (25, 4, 8), (15, 4, 12),
    (21, 5, 15), (22, 5, 16), (32, 5, 16), (16, 5, 12), (22, 5, 4),
    (21, 6, 16), (32, 6, 15), (31, 6, 16), (25, 6, 16), (21, 6, 4), (31, 6, 8), (19, 6, 12),
    (21, 7, 15), (22, 7, 16), (32, 7, 16), (16, 7, 8), (32, 7, 4),
    (22, 8, 15), (25, 8, 16), (31, 8, 16), (27, 8, 12), (15, 8, 8), (21, 8, 4),
]
_M64 = [
    (19, 1, 17), (21, 1, 17), (32, 1, 32), (31, 1, 31), (25, 1, 25), (32, 1, 24), (22, 1, 18),
    (22, 2, 17), (21, 2, 18), (32, 2, 17), (32, 2, 31), (31, 2, 24), (27, 2, 20), (31, 2, 28),
    (21, 3, 17), (22, 3, 18), (31, 3, 25), (32, 3, 28), (19, 3, 17),
    (22, 4, 17), (32, 4, 17), (21, 4, 18), (31, 4, 24), (32, 4, 25), (31, 4, 28),
    (21, 5, 17), (22, 5, 18), (31, 5, 25), (32, 5, 28), (27, 5, 17),
    (22, 6, 17), (32, 6, 17), (31, 6, 18), (32, 6, 25), (31, 6, 24), (25, 6, 20),
    (25, 7, 17), (31, 7, 17), (32, 7, 18), (31, 7, 25), (32, 7, 24),
    (25, 8, 18), (32, 8, 17), (31, 8, 18), (32, 8, 25), (31, 8, 24), (27, 8, 20),
]
# (k, TBK_COUNT_W, TBK_COUNT_M, expected (w, m, o)): plain mode at k >= 15, and W = 9, which is clamped to 8
_EDGE = [(15, 0, None, (0, 0, 0)), (21, 0, None, (0, 0, 0)), (32, 0, None, (0, 0, 0)), (31, 9, 16, (8, 16, 4)), (32, 9, 17, (8, 17, 4))]
_MATRIX = [(k, w, m, _expect(k, w, m)) for k, w, m in _M32 + _M64] + _EDGE
assert _expect(31, 6, 16) == (6, 16, 5) and _expect(32, 4, 17) == (4, 17, 6) and _expect(32, 1, 32) == (1, 32, 0)
assert {w for _, w, m in _M32} == set(range(1, 9)) == {w for _, w, m in _M64} and all(m <= 16 for _, _, m in _M32) and all(m >= 17 for _, _, m in _M64)
# what B is pinned to when it is not pinned like A: plain, a 32-bit and (k >= 19) a 64-bit selection
_PARTNERS = {
    15: [(0, None), (1, 15), (2, 4)], 16: [(0, None), (1, 16), (3, 8)], 19: [(0, None), (3, 15), (1, 17)],
    21: [(0, None), (6, 16), (3, 17)], 22: [(0, None), (5, 16), (6, 17)], 25: [(0, None), (6, 16), (7, 17)],
    27: [(0, None), (8, 16), (8, 18)], 31: [(0, None), (6, 16), (4, 24)], 32: [(0, None), (6, 15), (4, 17)],
}


def _stress_reads(rng, k):
    """What rolling code gets wrong: homopolymers and short-period repeats (one canonical k-mer, or two or three, counted hundreds of
    times; (ACGT)n is its own reverse complement), reads of k - 1, k and k + 31 .. k + 33 bases (a lane holds 32 windows), an N at
    the first, last, k-th and (k + 1)-th base."""
    n = 240
    reads = ["A" * n, "AC" * (n // 2), "ACGT" * (n // 4), "AAT" * (n // 3), "t" * (k + 7)]
    reads += [_rand(rng, L) for L in (k - 1, k, k + 1, k + 31, k + 32, k + 33)]
    for at in (0, -1, k - 1, k):
        s = list(_rand(rng, k + 40))
        s[at] = "N"
        reads.append("".join(s))
    return reads


def _two_parent_reads(rng, glen, n_a, n_b):
    from test_gpu_unique import _library, _two_parents

    ga, gb = _two_parents(rng, glen=glen)
    return _library(rng, ga, n_a, 150, lower=0.1), _library(rng, gb, n_b, 150)


@pytest.mark.parametrize("i,k,w,m,expect", [(i,) + c for i, c in enumerate(_MATRIX)], ids=[f"k{k}-W{w}-m{m or 0}" for k, w, m, _ in _MATRIX])
def test_every_kernel_against_the_oracle(gpu, tmp_path, monkeypatch, i, k, w, m, expect):
    """The two-parent library of test_gpu_unique (errors, N, lower case, both strands) plus the stress reads, A in several
    batches and B in one, under pinned (W, m); B is pinned like A in every fourth case and otherwise to plain mode, a 32-bit or a
    64-bit selection, so unique() looks k-mers up in a table laid out by another rule than the one it walks."""
    rng = np.random.default_rng(9000 + i)
    tiny = m is not None and m <= 8
    reads_a, reads_b = _two_parent_reads(rng, 8000, 900, 700)
    stress = _stress_reads(rng, k)
    reads_a += stress + ["", "ACGT", "N" * 40, stress[6], stress[6].lower(), _rc(stress[6])]
    reads_b += ["A" * 100, "AAT" * 30, stress[6], _rc(stress[7]), stress[8], stress[8]]
    order = rng.permutation(len(reads_a))
    reads_a = [reads_a[j] for j in order]
    bw, bm = (w, m) if i % 4 == 0 else _PARTNERS[k][i % 3]
    # tiny m: start at 16 buckets and fill to 0.9, so that the keys that left home also meet full second-choice lines
    cap_a, load = (16, 0.9) if tiny else ((400_000, 1000)[i % 2], None)
    with _Pinned(monkeypatch, k, cap_a, w, m, load, expect) as ca, _Pinned(monkeypatch, k, 200_000, bw, bm, None, expect if i % 4 == 0 else _expect(k, bw, bm)) as cb:
        step = 60 if tiny else 250
        for j in range(0, len(reads_a), step):
            ca.add(reads_a[j:j + step])
        cb.add(reads_b)
        oa, ob = uo.count_kmers_np(*uo.pack(reads_a), k), uo.count_kmers_np(*uo.pack(reads_b), k)
        assert oa[1].max() >= 200 and (oa[1] == 1).sum() > 1000
        _compare(ca, cb, oa, ob, k, tmp_path, ((2, 255), (3, 9), (1, 4), (200, 255)))
        _compare(cb, ca, ob, oa, k, tmp_path, ((2, 255), (4, 6)))


# ---- 3. pass and lane boundaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w,m,expect", [(16, None, None, (2, 15, 0)), (21, None, None, (6, 16, 0)), (32, None, None, (6, 15, 6)),
                                          (32, 4, 17, (4, 17, 6)), (21, 3, 17, (3, 17, 1))],
                         ids=["k16", "k21", "k32", "k32-W4-m17", "k21-W3-m17"])
def test_pass_and_lane_boundaries(gpu, tmp_path, monkeypatch, k, w, m, expect):
    """A pass is 2048 window starts of the separated stream (each read followed by one 'N'), a lane takes 32 of them.  One add per
    batch; the first read's length puts the read boundary at every stream offset from k + 2 before to 2 after the first and the
    second pass boundary and a lane boundary inside a pass, and single-read batches end the stream at every such offset around
    one and two passes.  Every batch is fresh random sequence: a window lost or counted twice changes the histogram.  The first
    batch is the longest, so every later one ends in front of stale bytes of an earlier one in the staging buffer."""
    rng = np.random.default_rng(300 + k + (m or 0))
    batches = [[_rand(rng, 9000), _rand(rng, 40)]]
    for edge in (2048, 4096, 32 * 33):
        for first in range(edge - k - 2, edge + 3):
            batches.append([_rand(rng, first), _rand(rng, k + 40), _rand(rng, 3)])
    for edge in (2048, 4096):
        for sep_total in range(edge - k - 2, edge + 3):
            batches.append([_rand(rng, sep_total - 1)])          # the stream is the read and its 'N'
            batches.append([_rand(rng, sep_total - k - 2), _rand(rng, k)])  # ... or ends with a read of one window
    with _Pinned(monkeypatch, k, 300_000, w, m, None, expect) as ca, _Pinned(monkeypatch, k, 16, w, m, None, expect) as empty:
        for b in batches:
            ca.add(b)
        every = [r for b in batches for r in b]
        oa = uo.count_kmers_np(*uo.pack(every), k)
        assert oa[0].size > 0.9 * sum(max(0, len(r) - k + 1) for r in every)
        none = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64))
        _compare(ca, empty, oa, none, k, tmp_path, ((1, 255), (2, 255)))


# ---- 4. saturation and cut-offs -------------------------------------------------------------------------------------
_A_TIMES, _B_TIMES = (1, 2, 3, 254, 255, 256, 300), (0, 1, 2)


@pytest.mark.parametrize("k,w,m,expect", [(21, None, None, (6, 16, 0)), (32, 4, 17, (4, 17, 6)), (16, 0, None, (0, 0, 0)), (31, 6, 4, (6, 4, 11))],
                         ids=["k21", "k32-W4-m17", "k16-plain", "k31-W6-m4"])
def test_saturation_and_cutoffs(gpu, tmp_path, monkeypatch, k, w, m, expect):
    """21 k-mers, one for every pair of (times in A, times in B), each occurrence a read of exactly k bases on a random strand.
    Counters saturate at 255, A keeps what it saw twice or more, B subtracts what IT saw twice or more (once is not enough)."""
    rng = np.random.default_rng(400 + k)
    kmers_ = set()
    while len(kmers_) < len(_A_TIMES) * len(_B_TIMES):
        s = _rand(rng, k)
        if s != _rc(s):
            kmers_.add(min(s, _rc(s)))
    plan = dict(zip(sorted(kmers_), [(a, b) for a in _A_TIMES for b in _B_TIMES]))
    reads_a = [s if rng.random() < 0.5 else _rc(s) for s, (a, _) in plan.items() for _ in range(a)]
    reads_b = [s if rng.random() < 0.5 else _rc(s) for s, (_, b) in plan.items() for _ in range(b)]
    reads_a = [reads_a[j] for j in rng.permutation(len(reads_a))]
    with _Pinned(monkeypatch, k, 1000, w, m, None, expect) as ca, _Pinned(monkeypatch, k, 1000, w, m, None, expect) as cb:
        for j in range(0, len(reads_a), 700):
            ca.add(reads_a[j:j + 700])
        cb.add(reads_b)
        hist = [int(x) for x in ca.c.histogram()]
        want = [0] * 256
        want[0], want[1], want[2], want[3], want[254], want[255] = 21, 3, 3, 3, 3, 9
        assert hist == want
        hist_b = [int(x) for x in cb.c.histogram()]
        assert hist_b[:3] == [14, 7, 7] and sum(hist_b[3:]) == 0
        for ci, cx in ((0, 255), (1, 255), (2, 2), (254, 254), (255, 255), (255, 1000), (256, 1000), (5, 3), (2, 254), (3, 254)):
            expected = sorted(s for s, (a, b) in plan.items() if a >= 2 and b < 2 and ci <= min(a, 255) <= cx)
            out = str(tmp_path / f"u_{ci}_{cx}.txt")
            n = ca.c.unique(cb.c, ci, cx, out)
            assert open(out).read() == "".join(s + "\n" for s in expected) and n == len(expected), (ci, cx)
            # (5, 3) and (256, 1000) select nothing: an empty file and 0; the others are 2 k-mers per counter value in range
            assert len(expected) == {(0, 255): 12, (1, 255): 12, (2, 2): 2, (254, 254): 2, (255, 255): 6, (255, 1000): 6, (256, 1000): 0,
                                     (5, 3): 0, (2, 254): 6, (3, 254): 4}[(ci, cx)]
        # and the oracle says the same
        _compare(ca, cb, uo.count_kmers_np(*uo.pack(reads_a), k), uo.count_kmers_np(*uo.pack(reads_b), k), k, tmp_path, ((2, 255), (1, 4)))


# ---- 5. load and growth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1, 16])
@pytest.mark.parametrize("load,clamped", [("0.9", 0.9), ("0.05", 0.05), ("2.0", 0.9), ("0.0", 0.05)])
@pytest.mark.parametrize("k,w,m,expect", [(21, None, None, (6, 16, 0)), (31, 4, 18, (4, 18, 5)), (21, 6, 4, (6, 4, 6))], ids=["k21", "k31-W4-m18", "k21-W6-m4"])
def test_load_and_growth(gpu, tmp_path, monkeypatch, k, w, m, expect, load, clamped, capacity):
    """A table that starts at 16 or 18 (or, at load 0.05, 56) lines and is fed 40 small batches: it is rebuilt again and again,
    keeps its pinned bucket selection, and counts what the oracle counts.  TBK_COUNT_LOAD outside 0.05 .. 0.9 is clamped: the
    first table has capacity / (8 * load) + 16 lines."""
    from test_gpu_unique import _library

    rng = np.random.default_rng(500 + k + capacity)
    genome = _rand(rng, 6000)
    reads = _library(rng, genome, 1200, 100, err=0.02) + ["A" * 300, "AC" * 100]
    other = _library(rng, genome, 300, 100, err=0.02)
    with _Pinned(monkeypatch, k, capacity, w, m, load, expect) as ca, _Pinned(monkeypatch, k, capacity, w, m, load, expect) as cb:
        slots0 = ca.stats()["n_slots"]
        assert slots0 == (int(capacity / (8 * clamped)) + 16) * 8
        seen = {slots0}
        for j in range(0, len(reads), 30):
            ca.add(reads[j:j + 30])
            seen.add(ca.stats()["n_slots"])
        cb.add(other)
        assert len(seen) >= 4 and max(seen) > 50 * slots0 and sorted(seen)[-1] == ca.stats()["n_slots"]
        _compare(ca, cb, uo.count_kmers_np(*uo.pack(reads), k), uo.count_kmers_np(*uo.pack(other), k), k, tmp_path, ((2, 255), (3, 9), (1, 4)))


# ---- 6. one add of several pieces -----------------------------------------------------------------------------------
_PIECE = 32768 * 2048  # window starts of a piece while the table has fewer than 2^28 slots (counter_run)


def _deep_library(rng, genome, n_reads, read_len, n_err, n_n):
    """n_reads reads of read_len bases drawn from `genome` (2-bit codes), half of them reverse-complemented, n_err bases replaced at
    random, n_n bases turned into N, one read in sixteen lower case; as (bases, offsets)."""
    rows = np.lib.stride_tricks.sliding_window_view(genome, read_len)[rng.integers(0, genome.size - read_len, n_reads)]
    flip = rng.random(n_reads) < 0.5
    rows[flip] = 3 - rows[flip][:, ::-1]
    flat = rows.reshape(-1)
    flat[rng.integers(0, flat.size, n_err)] = rng.integers(0, 4, n_err).astype(np.uint8)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[rows]
    text.reshape(-1)[rng.integers(0, flat.size, n_n)] = ord("N")
    text[::16] |= 0x20
    return text.reshape(-1), (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len))


@pytest.fixture(scope="module")
def deep(orc):
    """Two parents of a 3 Mbase genome: A at 67x in 20,200 reads of 10 kb (202 M window starts: four pieces), B at 20x; the
    oracle's counts of both, A's histogram from the C oracle as well (it runs beside the numpy counter)."""
    k = 32
    rng = np.random.default_rng(6)
    base = rng.integers(0, 4, 3_000_000).astype(np.uint8)
    ga, gb = base.copy(), base.copy()
    for g in (ga, gb):
        at = rng.integers(0, g.size, g.size // 500)
        g[at] = (g[at] + rng.integers(1, 4, at.size)) % 4
    a = _deep_library(rng, ga, 20_200, 10_000, 200_000, 20_000)
    b = _deep_library(rng, gb, 6_000, 10_000, 60_000, 6_000)
    assert int(a[1][-1]) + 20_200 > 3 * _PIECE + 2048
    with concurrent.futures.ThreadPoolExecutor(1) as pool:
        c_hist = pool.submit(orc.kmer_histogram, a[0], a[1], k, 14_000_000)
        oa = uo.count_kmers_np(a[0], a[1], k)
        ob = uo.count_kmers_np(b[0], b[1], k)
        c_hist = c_hist.result()
    assert 2_000_000 < oa[0].size < 14_000_000
    return k, a, b, oa, ob, c_hist


@pytest.mark.parametrize("w,m,expect,grown", [(None, None, (6, 15, 6), (6, 17, 5)), (6, 15, (6, 15, 6), (6, 15, 6)), (4, 17, (4, 17, 6), (4, 17, 6))],
                         ids=["default", "W6-m15", "W4-m17"])
def test_multi_piece_add(gpu, deep, tmp_path, monkeypatch, w, m, expect, grown):
    """One add of 202 M bases at k = 32 is counted in four launches (first_pass != 0 in three).  The capacity of 1390 k-mers is
    chosen so that the table is rebuilt twice during that add: the doubling rule of counter_run goes from 2440 slots to the first
    table whose 0.85 holds a piece (67.1 M window starts) - 79.95 M slots, 67.96 M at 0.85 - and the second piece (a million
    k-mers are in by then) no longer fits that, so the table doubles between the pieces.  Histogram against the C oracle, lists
    against the numpy counter.

    Left to itself (no knob set) the table changes its bucket selection on the way: it starts at W = 6, m = 15, o = 6, and the
    rebuilt table's capacity of 95.9 M k-mers is past what tbk_mz_params gives 15-base m-mers (6 * 95.9 M > 0.9 * 4^15 / 2), so
    it takes m = 17, o = 5 - the keys move from a table filled by the 32-bit kernel into one the 64-bit kernel goes on with.
    The two pinned cases keep one selection for all four pieces."""
    k, a, b, oa, ob, c_hist = deep
    with _Pinned(monkeypatch, k, 1390, w, m, None, expect) as ca, _Pinned(monkeypatch, k, 30_000_000, w, m, None, expect) as cb:
        assert ca.stats()["n_slots"] == 2440
        ca.expect = grown
        ca.add_packed(*a)
        cb.add_packed(*b)
        first = (int(2928 * 2 ** 14 / 4.8) + 16) * 8   # 2928 = twice 0.6 * 2440; 2928 * 2^14 k-mers is the first capacity that holds a piece
        assert int(0.85 * first) > _PIECE and ca.stats()["n_slots"] == (int(int(first * 0.6) * 2 / 4.8) + 16) * 8
        launches, windows, _ = ca.c.kernel_timing()
        assert launches == 4 and windows == int(a[1][-1]) + a[1].size - 1
        assert [int(x) for x in ca.c.histogram()] == [int(x) for x in c_hist]
        _compare(ca, cb, oa, ob, k, tmp_path, ((2, 255), (20, 60), (1, 4)))


@pytest.mark.parametrize("w,m,expect,grown", [(None, None, (6, 15, 6), (6, 17, 5)), (4, 17, (4, 17, 6), (4, 17, 6))], ids=["default", "W4-m17"])
def test_multi_piece_add_in_passes(gpu, deep, tmp_path, monkeypatch, w, m, expect, grown):
    """The same add with passes = 3: the 202 M positions are retained and counted in several pieces for class 0, then replayed in
    the same pieces for classes 1 and 2.  Three times the capacity of test_multi_piece_add gives a class the same first table of
    2440 slots, so class 0 meets the same rebuild between the first piece and the second (the third of the genome's k-mers that
    is in by then is still more than the 0.85 M slots the first rebuild leaves over a piece); the table after it is larger than
    the first one that holds a piece, which is asserted.  Left to itself the table changes from the 32-bit selection to the
    64-bit one there, in the middle of class 0; the pinned case keeps one 64-bit selection throughout.  Histogram against the C
    oracle, lists against the numpy counter; three passes over the store cost the device well under a second."""
    k, a, b, oa, ob, c_hist = deep
    with _Pinned(monkeypatch, k, 3 * 1390, w, m, None, expect, passes=3) as ca, _Pinned(monkeypatch, k, 90_000_000, w, m, None, expect, passes=3) as cb:
        assert ca.stats()["n_slots"] == 2440
        ca.expect = grown
        ca.add_packed(*a)
        cb.add_packed(*b)
        st = ca.stats()
        positions = int(a[1][-1]) + a[1].size - 1
        first = (int(2928 * 2 ** 14 / 4.8) + 16) * 8  # the first table of the doubling rule whose 0.85 holds a piece (test_multi_piece_add)
        assert int(0.85 * first) > _PIECE and st["n_slots"] > first and positions > 3 * _PIECE
        assert st["store_used_bytes"] == 8 * ((positions + 15) // 16) and st["passes"] == 3 and not st["finished"]
        launches, windows, _ = ca.c.kernel_timing()
        assert launches > 1 and windows == 16 * ((positions + 15) // 16)
        assert [int(x) for x in ca.histogram()] == [int(x) for x in c_hist]
        launches, windows, _ = ca.c.kernel_timing()
        assert launches > 2 and windows == 2 * 16 * ((positions + 15) // 16)  # classes 1 and 2, from the store
        _compare(ca, cb, oa, ob, k, tmp_path, ((2, 255), (20, 60), (1, 4)))


# ---- 7. the clamp ---------------------------------------------------------------------------------------------------
def _mix32(key):
    """tbk_mix32 (tbk_common.h) of an array of keys below 2^32."""
    lo = key.astype(np.uint32)
    h = lo * np.uint32(0x9E3779B1) ^ np.uint32((0x7F4A7C15 * 0x85EBCA77) & 0xFFFFFFFF)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0xC2B2AE3D)
    h ^= h >> np.uint32(13)
    return h


@pytest.fixture
def entry_cap(gpu):
    """set(entry_blocks): the cap of tbk_count_set_grid_caps_ on the launches that stride over table slots, the stream cap left
    at 0; (0, 0) again when the test ends, however it ends"""
    def set_cap(entry_blocks):
        assert gpu.lib.tbk_count_set_grid_caps_(0, entry_blocks) == 0
    try:
        yield set_cap
    finally:
        gpu.lib.tbk_count_set_grid_caps_(0, 0)


@pytest.mark.parametrize("entry_blocks", [0, 1])
def test_clamp_keeps_a_counter_below_the_carry(gpu, tmp_path, monkeypatch, entry_cap, entry_blocks):
    """The eight 32-bit counters of a line are added to as four 64-bit words, so a counter that passed 2^32 would carry into its
    neighbour; counter_run sets every counter above 2^31 back to 2^31 (readers cap at 255) before 2^31 more window starts can have
    been added.  Here poly-A at k = 13 gets more than 2^32 + 2^28 window starts, with seven witnesses seen three times each in the
    other slots of its line - the first of them in the half of poly-A's own word.

    Plain mode (k < 15) makes the placement computable: bucket = (mix32(key) * n_buckets) >> 32, key = the smaller of the k-mer
    and its reverse complement packed with base 0 in the low bits; slots fill in index order.  Without the clamp the first witness
    reads 4.

    entry_blocks = 1: the clamp (and the rebuild, the histogram and the dump) run as one block of 256 threads, so poly-A's
    counter is set back on a later trip of tbk_count_clamp_kernel's loop, as every counter of a real parental library's table is;
    the counting kernel keeps its grid.

    Measured on an MI355X: 3.0 s for the 545 adds of 8 Mbases (4096 launches' worth of same-address adds each), 3.4 s for the test."""
    entry_cap(entry_blocks)
    k, read, per_add = 13, 1 << 20, 8
    batch = uo.pack(["A" * read] * per_add)
    windows = per_add * (read - k + 1)
    none = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64))
    with _Pinned(monkeypatch, k, 1000, None, None, None, (0, 0, 0)) as ca, _Pinned(monkeypatch, k, 16, None, None, None, (0, 0, 0)) as empty:
        ca.add_packed(*batch)
        n_slots = ca.stats()["n_slots"]
        n_buckets = n_slots // 8
        assert n_slots > 8 * 1000
        # canonical 13-mers whose home bucket is poly-A's (key 0)
        keys = np.arange(1, 1 << 26, dtype=np.uint64)
        home = (_mix32(keys).astype(np.uint64) * np.uint64(n_buckets)) >> np.uint64(32)
        home0 = (int(_mix32(np.zeros(1, dtype=np.uint64))[0]) * n_buckets) >> 32
        assert home0 * 8 >= entry_blocks * 256  # poly-A's slot (in its home bucket or a later one) lies past the capped clamp's first trip
        cand = keys[home == np.uint64(home0)]
        names = []
        for key in cand:
            s = "".join("ACGT"[(int(key) >> (2 * j)) & 3] for j in range(k))
            r = _rc(s)
            if int(key) < sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(r)):
                names.append(s)
        assert len(names) >= 7, (n_buckets, len(names))
        witnesses = names[:7]
        for s in witnesses:
            ca.add([s, _rc(s), s])
        added, calls, t0 = windows, 1, time.time()
        while added <= (1 << 32) + (1 << 28):
            ca.add_packed(*batch)
            added += windows
            calls += 1
        seconds = time.time() - t0
        print(f"clamp test: {calls} adds, {added} window starts, {seconds:.1f} s")
        assert ca.stats()["n_slots"] == n_slots and calls == 545
        hist = [int(x) for x in ca.c.histogram()]
        want = [0] * 256
        want[0], want[3], want[255] = 8, 7, 1
        assert hist == want
        out = str(tmp_path / "witnesses.txt")
        n = ca.c.unique(empty.c, 3, 3, out)
        assert n == 7 and open(out).read().split("\n") == sorted(min(s, _rc(s)) for s in witnesses) + [""]
        oa = uo.count_kmers_np(*uo.pack([s for w_ in witnesses for s in (w_, _rc(w_), w_)]), k)
        _compare(ca, empty, (np.concatenate(([0], oa[0])).astype(np.uint64), np.concatenate(([added], oa[1]))), none, k, tmp_path, ((2, 254), (255, 255)))
