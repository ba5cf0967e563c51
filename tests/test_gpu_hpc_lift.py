"""The compression map read backwards on the device (tbk_hpc_lift, tbk_hpc_expand; kmers.HomopolymerCompressor.lift / .expand;
kernels tbk_hpc_lift_kernel and tbk_hpc_expand_kernel in csrc/tbk_hpc.hip) against its numpy restatement (tests/hpc_lift_ref.py):
lift(j) is the position of the j-th set keep bit and lift(total_c) = total; expand puts value j on position lift(j) and 0
everywhere else.  Every comparison is exact and made with fold_case off and on.  The shapes are the smallest at which the
geometry can go wrong: T = a tile of 4096 bases (one scanned count, 64 keep words), 64 = a keep word, 16 = a lane's vector."""
import ctypes as C

import numpy as np
import pytest

import hpc_lift_ref as lref

pytestmark = pytest.mark.gpu

T = 4096


def _pack(reads):
    enc = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    offsets = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        offsets[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return np.frombuffer(b"".join(enc), dtype=np.uint8).copy(), offsets


def _background(n, phase=0):
    """n bytes without two equal neighbours and without an 'A' or 'a'"""
    return np.frombuffer(b"CGT", dtype=np.uint8)[(np.arange(n) + phase) % 3].copy()


def _geometric(rng, total, alphabet=b"ACGTNacgtn"):
    symbols = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), total + 1)]
    return np.repeat(symbols, rng.geometric(0.45, symbols.size))[:total].copy()


@pytest.fixture(scope="module")
def comp(gpu):
    from trio_binning_amd import kmers
    from trio_binning_amd._lib import lib

    lib.tbk_hpc_tile.restype = C.c_uint32
    assert int(lib.tbk_hpc_tile()) == T
    with kmers.HomopolymerCompressor() as c:
        yield c


def _check(comp, bases, offsets, folds=(False, True), seed=0):
    """lift at every position 0 .. total_c in a shuffled order with duplicates, lift at the reads' compressed starts, and expand
    of random bytes, against the reference; returns the reference lift of the last fold"""
    rng = np.random.default_rng(seed)
    total = int(offsets[-1])
    for fold in folds:
        want = lref.lift_np(bases, offsets, fold)
        cb, co = comp.compress(bases, offsets, fold_case=fold)
        assert cb.size + 1 == want.size, fold
        ask = np.concatenate([np.arange(want.size), rng.integers(0, want.size, 70)]).astype(np.uint64)
        rng.shuffle(ask)
        got = comp.lift(ask)
        assert got.dtype == np.uint64 and got.shape == ask.shape
        if not np.array_equal(got, want[ask.astype(np.int64)]):
            bad = np.flatnonzero(got != want[ask.astype(np.int64)])[:6]
            raise AssertionError(f"fold {fold}: lift of {ask[bad].tolist()} gave {got[bad].tolist()} for {want[ask[bad].astype(np.int64)].tolist()}")
        assert np.array_equal(comp.lift(co), offsets), fold  # a read's compressed start lifts to its start
        values = rng.integers(1, 256, cb.size).astype(np.uint8)
        spread = comp.expand(values)
        assert spread.dtype == np.uint8 and spread.size == total
        assert np.array_equal(spread, lref.expand_np(values, want, total)), (fold, np.flatnonzero(spread != lref.expand_np(values, want, total))[:6])
        assert np.array_equal(comp.expand(cb), np.where(lref.keep_np(bases, offsets, fold), bases[:total], 0)), fold  # the kept bytes go back to where they came from
    return want


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1])
def test_batches_beside_a_tile(comp, n):
    rng = np.random.default_rng(n)
    want = _check(comp, _background(n), np.array([0, n], dtype=np.uint64))
    assert np.array_equal(want, np.arange(n + 1))  # nothing dropped: the identity
    _check(comp, _geometric(rng, n), np.array([0, n], dtype=np.uint64))
    _check(comp, _geometric(rng, n, b"Aa"), np.array([0, n // 3, n // 3, n], dtype=np.uint64))


def test_kept_bits_on_the_edges_of_a_vector_a_word_and_a_tile(comp):
    places = [0, 15, 16, 63, 64, T - 1, T]
    n = T + 40
    bases = np.zeros(n, dtype=np.uint8)
    for i, (lo, hi) in enumerate(zip(places, places[1:] + [n])):
        bases[lo:hi] = b"AC"[i % 2]
    want = _check(comp, bases, np.array([0, n], dtype=np.uint64))
    assert want.tolist() == places + [n]
    # and the mirror image: everything kept but the bytes at those places
    bases = _background(n)
    for p in places[1:]:
        bases[p] = bases[p - 1]
    bases[[17, 65, T + 1]] = ord("N")  # (behind a run of three the background would repeat the run's letter)
    want = _check(comp, bases, np.array([0, n], dtype=np.uint64))
    assert want.tolist() == [p for p in range(n) if p not in places[1:]] + [n]


@pytest.mark.parametrize("where", ["middle", "end", "both"])
def test_a_homopolymer_longer_than_two_tiles_leaves_empty_tiles(comp, where):
    long_run = np.full(3 * T + 700, ord("A"), dtype=np.uint8)  # wherever it starts, two whole tiles lie inside it
    parts = [_background(T // 2 + 5)]
    if where in ("middle", "both"):
        parts += [long_run, _background(300, 1)]
    if where in ("end", "both"):
        parts += [long_run]
    bases = np.concatenate(parts)
    n = bases.size
    want = _check(comp, bases, np.array([0, n], dtype=np.uint64))
    tiles_with_a_bit = np.unique(want[:-1] // T)
    assert tiles_with_a_bit.size <= (n + T - 1) // T - 2  # at least two tiles follow one another without a kept bit
    if where != "middle":
        assert int(want[-2]) < n - 2 * T and int(want[-1]) == n  # lift(total_c) comes behind the empty tiles
    bases[bases == ord("A")] = np.frombuffer(b"Aa", dtype=np.uint8)[np.arange(int((bases == ord("A")).sum())) % 2]
    _check(comp, bases, np.array([0, n], dtype=np.uint64))  # folded: the same runs; unfolded: nothing to drop in them
    _check(comp, bases, np.array([0, T, T, n - T - 3, n], dtype=np.uint64))


def test_a_run_that_continues_across_a_read_boundary_keeps_both_first_bytes(comp):
    n = T + 64
    bases = np.full(n, ord("A"), dtype=np.uint8)
    for cut in (15, 16, 17, 63, 64, 65, T - 1, T, T + 1):
        want = _check(comp, bases, np.array([0, cut, n], dtype=np.uint64))
        assert want.tolist() == [0, cut, n]
    cuts = [0, 8, 16, 16, 1024, T, T + 1, n, n]
    want = _check(comp, bases, np.array(cuts, dtype=np.uint64))
    assert want.tolist() == [0, 8, 16, 1024, T, T + 1, n]


def test_empty_reads_first_in_the_middle_and_last(comp):
    bases, offsets = _pack(["", "ACCA", "", "", "GGT", ""])
    want = _check(comp, bases, offsets)
    assert want.tolist() == [0, 1, 3, 4, 6, 7]
    rng = np.random.default_rng(3)
    body = _geometric(rng, 2 * T + 11, b"ACGT")
    _check(comp, body, np.array([0, 0, 0, 900, 900, 900, T, 2 * T + 11, 2 * T + 11], dtype=np.uint64))


def test_only_empty_reads_and_no_reads(comp):
    for offsets in ([0, 0, 0, 0], [0]):
        offsets = np.array(offsets, dtype=np.uint64)
        want = _check(comp, np.zeros(0, dtype=np.uint8), offsets)
        assert want.tolist() == [0]
        assert comp.lift(np.zeros(0, dtype=np.uint64)).size == 0  # n == 0
        assert comp.lift(np.zeros(5, dtype=np.uint64)).tolist() == [0] * 5
        assert comp.expand(np.zeros(0, dtype=np.uint8)).size == 0


def test_every_position_of_three_and_a_half_tiles(comp):
    rng = np.random.default_rng(17)
    n = 3 * T + T // 2
    bases = _geometric(rng, n)
    cuts = np.sort(rng.integers(0, n + 1, 9)).tolist()
    for seed in (1, 2):
        _check(comp, bases, np.array([0] + cuts + [n], dtype=np.uint64), seed=seed)


def test_refusals_leave_the_session_usable(gpu):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(23)
    bases = _geometric(rng, T + 100)
    offsets = np.array([0, 50, T + 100], dtype=np.uint64)
    with kmers.HomopolymerCompressor() as comp:
        with pytest.raises(ValueError):  # a session without a result
            comp.lift(np.zeros(1, dtype=np.uint64))
        want = _check(comp, bases, offsets, folds=(True,))
        total_c = want.size - 1
        assert int(comp.lift(np.array([total_c], dtype=np.uint64))[0]) == T + 100
        with pytest.raises(ValueError):  # a position above total_c
            comp.lift(np.array([0, total_c + 1, 3], dtype=np.uint64))
        assert np.array_equal(comp.lift(np.arange(total_c + 1, dtype=np.uint64)), want)  # the result is still there
        with pytest.raises(ValueError):
            comp.expand(np.zeros(total_c + 1, dtype=np.uint8))
        bad = offsets.copy()
        bad[1] = T + 200
        with pytest.raises(ValueError):
            comp.compress(bases, bad)
        with pytest.raises(ValueError):  # a refused batch leaves no result to lift through
            comp.lift(np.zeros(1, dtype=np.uint64))
        _check(comp, bases, offsets)
