"""tests/db_query_ref.py's numpy reference (window_ranks, TallyNp) held to its Python loop (window_kmers, Tally) on small random
input - N, lower case, sequences shorter than k, empty ones, k-mers that are their own reverse complement, two batches - before
tests/test_gpu_db_query_scale.py lets it judge the device on a database that the loop cannot follow."""
import numpy as np
import pytest

import db_query_ref as ref


def _pack(sequences):
    bases = np.frombuffer("".join(sequences).encode(), dtype=np.uint8)
    return bases, np.concatenate([[0], np.cumsum([len(s) for s in sequences])]).astype(np.uint64)


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _own_reverse_complement(rng, k):
    half = _seq(rng, k // 2)
    return half + ref.revcomp(half)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("k", [4, 5, 21, 32])
def test_the_numpy_reference_agrees_with_the_loop(k, seed):
    rng = np.random.default_rng(1000 * k + seed)
    genome = _seq(rng, 600)
    own = _own_reverse_complement(rng, k) if k % 2 == 0 else ""
    assert k % 2 or ref.revcomp(own) == own
    held = [genome[:400], own]
    db = {km: 2 + ref.lex_rank(km) % 254 for s in held for km in ref.window_kmers(s, k) if km is not None}
    ranks = np.array(sorted(ref.lex_rank(km) for km in db), dtype=np.uint64)
    counters = np.array([db[km] for km in sorted(db, key=ref.lex_rank)], dtype=np.uint8)
    batches = []
    for b in range(2):
        sequences = []
        for _ in range(int(rng.integers(4, 12))):
            n = int(rng.integers(0, 300))
            p = int(rng.integers(0, len(genome) - n + 1))
            s = list(genome[p:p + n])
            for at in rng.integers(0, max(n, 1), n // 60):
                s[int(at)] = "N" if rng.integers(0, 2) else s[int(at)].lower()
            s = "".join(s)
            sequences.append(ref.revcomp(s.upper()) if rng.integers(0, 3) == 0 else s)
        sequences += ["", _seq(rng, k - 1), _seq(rng, k), "n" * 30, own, "T" + own + "N" + own, genome[:k].lower()]
        batches.append([sequences[i] for i in rng.permutation(len(sequences))])
    loop, fast = ref.Tally(db), ref.TallyNp(ranks, counters)
    for sequences in batches:
        bases, offsets = _pack(sequences)
        min_count = int(rng.choice((2, 2, 100)))
        want_per_read, want_counts = loop.add(sequences, k, min_count)
        per_read, counts = fast.add(bases, offsets, k, min_count)
        assert per_read.dtype == np.uint64 and counts.dtype == np.uint8
        assert np.array_equal(counts, want_counts) and np.array_equal(per_read, want_per_read)
        # the windows themselves: clean where the loop has a k-mer, and the rank is that k-mer's
        rank, clean = ref.window_ranks(bases, offsets, k)
        at = 0
        for s in sequences:
            windows = ref.window_kmers(s, k)
            assert [bool(x) for x in clean[at:at + len(s)]] == [km is not None for km in windows] + [False] * (len(s) - len(windows))
            assert [int(x) for x in rank[at:at + len(windows)]] == [0 if km is None else ref.lex_rank(km) for km in windows]
            at += len(s)
        assert np.array_equal(fast.hist, loop.hist)
        for cuts in ((2, 255), (100, 255), (2, 99), (0, 1000), (200, 100)):
            assert fast.completeness(*cuts) == loop.completeness(*cuts), cuts
        assert np.array_equal(fast.spectrum(), loop.spectrum())
        assert {km: int(fast.copies[i]) for i, km in enumerate(sorted(db, key=ref.lex_rank)) if fast.copies[i]} == loop.copies
    if k % 2 == 0:
        assert loop.copies[ref.canonical(own)] >= 6  # once per window, whichever strand
    assert int(loop.hist[0]) > 0 and int(loop.hist[2:].sum()) > 0 and (k < 21 or int(loop.spectrum()[0].sum()) > 0)


def test_an_empty_database_and_an_empty_batch():
    fast = ref.TallyNp(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    per_read, counts = fast.add(*_pack(["ACGTACGT", ""]), 5)
    assert per_read.tolist() == [[4, 0], [0, 0]] and counts.tolist() == [0] * 8 and int(fast.hist[0]) == 4
    assert fast.completeness() == (0, 0) and int(fast.spectrum().sum()) == 0
    per_read, counts = fast.add(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 5)
    assert per_read.shape == (0, 2) and counts.size == 0
