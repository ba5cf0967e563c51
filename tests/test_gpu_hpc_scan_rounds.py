"""The later rounds of the compression's scan (tbk_hpc_scan_kernel in csrc/tbk_hpc.hip): one block scans 8192 tile counts a round
and carries the round's total into the next.  A batch of `tiles` tiles gives it tiles + 1 counts, so only a batch of 8192 tiles -
33.5 Mbases - reaches round two, where out[n - 1], the compressed total that the host brings home, is written from the carry
alone.  tbk_hpc_offsets_kernel, tbk_hpc_lift_kernel (a bisection over the tiles + 1 offsets), tbk_hpc_scatter_kernel and
tbk_hpc_expand_kernel all read what the scan wrote.

tiles = 8191, 8192 and 8193 give 8192 counts (exactly one round), 8193 (the total alone in round two) and 8194 (a tile and the
total in round two); tiles = 16385 gives three rounds, where a carry that is assigned and not added would show.  The reference is
numpy (tests/hpc_ref.py, tests/hpc_lift_ref.py).  Every comparison is exact.

Two contents.  "cuts": read cuts exactly at 8191 T, 8192 T - 1, 8192 T and 8192 T + 1, the scan's round edge.  "run": a
homopolymer longer than a tile laid across 8192 T - in both letter cases where fold_case is on, so that only the folding
makes it one run - which leaves a zero in the last slot of round one and in the first slot of round two and gives the lift
empty tiles at the round edge (a cut at 8192 T would put a kept byte there: the two cannot be one batch).  The three-round
batch has the cuts at the first round edge and the run across the second."""
import ctypes as C

import numpy as np
import pytest

import hpc_lift_ref as lref
import hpc_ref

pytestmark = pytest.mark.gpu

ROUND = 8192  # counts that the scan takes in one round


@pytest.fixture(scope="module")
def comp(gpu):
    from trio_binning_amd import kmers
    from trio_binning_amd._lib import lib

    lib.tbk_hpc_tile.restype = C.c_uint32
    with kmers.HomopolymerCompressor() as c:
        c.tile = int(lib.tbk_hpc_tile())
        yield c


def _batch(T, tiles, fold, content, seed):
    """(bases, offsets, first and end of the long run or None)"""
    rng = np.random.default_rng(seed)
    total = (tiles - 1) * T + 37
    bases = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, total)]
    run = None
    if content != "cuts":
        edge = (2 * ROUND if content == "both" else ROUND) * T
        run = (edge - T - 50, min(edge + T + 50, total))
        assert run[1] - run[0] > T and run[0] < edge < run[1]
        bases[run[0]:run[1]] = ord("A")
        if fold:
            bases[run[0] + 1:run[1]:2] = ord("a")
        bases[run[0] - 1] = ord("C")
        if run[1] < total:
            bases[run[1]] = ord("C")
    cuts = rng.integers(1, total, 2000)
    if content != "run":
        cuts = np.concatenate([cuts, [p for p in ((ROUND - 1) * T, ROUND * T - 1, ROUND * T, ROUND * T + 1) if p < total]])
    else:
        cuts = np.concatenate([cuts, [p for p in ((ROUND - 1) * T - T, ROUND * T - T - 50) if p < total]])  # (the run starts a read)
    if run:
        cuts = cuts[(cuts <= run[0]) | (cuts >= run[1])]  # no read starts inside the run: it stays one run
    cuts = np.concatenate([cuts, cuts[:3], [total]])      # three empty reads, and one behind the last base
    offsets = np.concatenate([[0], np.sort(cuts), [total]]).astype(np.uint64)
    return bases, offsets, run


CASES = [(8191, False, "cuts"), (8191, True, "cuts"), (8192, False, "cuts"), (8192, True, "cuts"), (8193, False, "cuts"), (8193, True, "cuts"),
         (8193, False, "run"), (8193, True, "run"), (16385, False, "both")]


@pytest.mark.parametrize("tiles,fold,content", CASES)
def test_the_scan_past_its_first_round(comp, tiles, fold, content):
    T = comp.tile
    bases, offsets, run = _batch(T, tiles, fold, content, 10 * tiles + int(fold))
    total = int(offsets[-1])
    # not vacuous: the counts the scan gets, and the rounds it takes for them
    counts = tiles + 1
    assert (total + T - 1) // T == tiles and total == (tiles - 1) * T + 37
    assert {8191: counts == ROUND, 8192: counts == ROUND + 1, 8193: counts == ROUND + 2, 16385: counts == 2 * ROUND + 2}[tiles]
    assert (counts + ROUND - 1) // ROUND == {8191: 1, 8192: 2, 8193: 2, 16385: 3}[tiles]

    want_bases, want_offsets = hpc_ref.compress_np(bases, offsets, fold)
    lift = lref.lift_np(bases, offsets, fold)
    total_c = want_bases.size
    assert lift.size == total_c + 1
    tile_offsets = np.searchsorted(lift[:-1], np.arange(tiles + 1, dtype=np.uint64) * np.uint64(T))  # what the scan must write
    if run:
        slot = 2 * ROUND if content == "both" else ROUND  # the first slot of a later round, and the slot before it, count 0
        assert tile_offsets[slot - 1] == tile_offsets[slot] == tile_offsets[slot + 1]
    if content != "run" and tiles > ROUND:
        assert {ROUND * T - 1, ROUND * T, ROUND * T + 1} <= set(offsets.tolist())

    cb, co = comp.compress(bases, offsets, fold_case=fold)
    assert cb.size == total_c, (cb.size, total_c)  # out[n - 1]: in the later rounds the carry alone
    assert np.array_equal(co, want_offsets), np.flatnonzero(co != want_offsets)[:6]
    assert np.array_equal(cb, want_bases), np.flatnonzero(cb != want_bases)[:6]

    rng = np.random.default_rng(tiles)
    ask = [0, total_c - 1, total_c]
    for t in range(ROUND - 2, tiles + 1, 1):  # both neighbours of every compressed tile offset at a round edge
        if min(abs(t - ROUND), abs(t - 2 * ROUND)) <= 2:
            ask += [int(tile_offsets[t]) + d for d in (-1, 0, 1)]
    ask = np.clip(np.concatenate([np.array(ask, dtype=np.int64), rng.integers(0, total_c + 1, 4000)]), 0, total_c)
    got = comp.lift(ask.astype(np.uint64))
    if not np.array_equal(got, lift[ask]):
        bad = np.flatnonzero(got != lift[ask])[:6]
        raise AssertionError(f"lift of {ask[bad].tolist()} gave {got[bad].tolist()} for {lift[ask[bad]].tolist()}")
    assert np.array_equal(comp.lift(co), offsets)  # a read's compressed start lifts to its start

    values = ((np.arange(total_c, dtype=np.uint64) * np.uint64(7)) % np.uint64(251) + np.uint64(1)).astype(np.uint8)
    spread = comp.expand(values)
    want_spread = lref.expand_np(values, lift, total)
    assert spread.dtype == np.uint8 and spread.size == total
    assert np.array_equal(spread, want_spread), np.flatnonzero(spread != want_spread)[:6]
