"""tests/pieces_ref.py, the reference of the read pieces' tests, held to hand-worked cases and to the identities that tie it to
screen_ref.record: with the covered side, every piece and min_length 1 the pieces are the record's stretches - their number, their
summed length `covered`, their maximum `longest` - and the covered and the uncovered pieces of a sequence are disjoint and tile
[0, L).  No device, no library: plain Python against plain Python."""
import numpy as np
import pytest

import db_query_ref as ref
import pieces_ref as pr
import screen_ref as sr


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def test_runs_and_the_selection_by_hand():
    T, F = True, False
    mask = [T, T, F, T, F, F, T, T, T]
    assert pr.runs(mask, True) == [(0, 2), (3, 4), (6, 9)] and pr.runs(mask, False) == [(2, 3), (4, 6)]
    assert pr.runs([], True) == pr.runs([], False) == [] and pr.runs([T], True) == [(0, 1)] and pr.runs([T], False) == []
    assert pr.runs([F, F], False) == [(0, 2)]
    found = [(0, 2), (3, 4), (6, 9), (10, 13)]
    assert pr.select(found) == pr.select(found, min_length=0) == found  # 0 and 1 mean the same
    assert pr.select(found, min_length=2) == [(0, 2), (6, 9), (10, 13)] and pr.select(found, min_length=4) == []
    assert pr.select(found, "longest") == [(6, 9)]  # two of three bases: the first wins
    assert pr.select(found[:2], "longest") == [(0, 2)] and pr.select(found, "longest", 4) == [] and pr.select([], "longest") == []
    assert pr.select([(0, 1), (5, 9)], "longest", 2) == [(5, 9)]


def test_the_pieces_of_a_hand_made_batch():
    k = 3
    #            0123456789012
    sequences = ["AAACCCGGGTTTA", "", "AC", "ACG", "AAANAAA", "NNNN", "aaac"]
    db = {ref.canonical("AAA"): 5, ref.canonical("CCG"): 2, ref.canonical("ACG"): 200}
    # windows of the first: AAA AAC ACC CCC CCG CGG GGG GGT GTT TTT TTA; held AAA (0), CCG (4), CGG = revcomp CCG (5), TTT = revcomp AAA (9)
    assert pr.pieces(db, sequences, k) == [(0, 0, 3), (0, 4, 8), (0, 9, 12), (3, 0, 3), (4, 0, 3), (4, 4, 7), (6, 0, 3)]
    assert pr.pieces(db, sequences, k, side="uncovered") == [(0, 3, 4), (0, 8, 9), (0, 12, 13), (2, 0, 2), (4, 3, 4), (5, 0, 4), (6, 3, 4)]
    assert pr.pieces(db, sequences, k, which="longest") == [(0, 4, 8), (3, 0, 3), (4, 0, 3), (6, 0, 3)]  # of [0,3) and [4,7) the first
    assert pr.pieces(db, sequences, k, min_length=4) == pr.pieces(db, sequences, k, min_length=4, which="longest") == [(0, 4, 8)]
    assert pr.pieces(db, sequences, k, side="uncovered", which="longest", min_length=2) == [(2, 0, 2), (5, 0, 4)]
    # the counter range: [3, 255] holds AAA and ACG, [1, 2] only CCG - and a solid database's floor makes (1, 1) empty
    assert pr.pieces(db, sequences, k, 3, 255) == [(0, 0, 3), (0, 9, 12), (3, 0, 3), (4, 0, 3), (4, 4, 7), (6, 0, 3)]
    assert pr.pieces(db, sequences, k, 1, 2) == [(0, 4, 8)] and pr.pieces(db, sequences, k, 1, 1) == []
    assert pr.pieces(dict(db, **{ref.canonical("GTT"): 1}), sequences, k, 1, 1, floor=1) == [(0, 1, 4), (0, 8, 11), (6, 1, 4)]  # AAC = revcomp GTT; "aaac" ends with it
    # a sequence shorter than k: no covered piece, one whole uncovered one; an empty one: none at all
    assert [p for p in pr.pieces({}, sequences, k, side="uncovered")] == [(i, 0, len(s)) for i, s in enumerate(sequences) if s]
    assert pr.pieces({}, sequences, k) == []
    assert pr.as_array([(1, 2, 3)]).tobytes() == np.array([1, 2, 3], dtype="<u8").tobytes() and pr.as_array([]).size == 0


def test_the_text_of_a_piece_by_hand():
    assert pr.record_text("r1 a comment", "ACGT", "IIII") == "@r1\nACGT\n+\nIIII\n" and pr.record_text("r1", "ACGT", "") == ">r1\nACGT\n"
    assert pr.record_text("r1", "ACGT", None) == ">r1\nACGT\n"
    assert pr.piece_text("r1 x", "ACGTAC", "123456", 1, 4, True) == "@r1:2-4\nCGT\n+\n234\n"
    assert pr.piece_text("r1 x", "ACGTAC", "123456", 1, 4, False) == "@r1\nCGT\n+\n234\n"
    assert pr.piece_text("r1 x", "ACGTAC", "", 0, 2, True) == ">r1:1-2\nAC\n" and pr.piece_text("r1", "ACGTAC", None, 4, 6, True) == ">r1:5-6\nAC\n"
    for suffix in (True, False):  # the whole record keeps its name
        assert pr.piece_text("r1 x", "ACGTAC", "123456", 0, 6, suffix) == pr.record_text("r1 x", "ACGTAC", "123456")
    records = [("a", "ACGTAC", "123456"), ("b", "AAAA", ""), ("c x", "CCCC", "IIII"), ("d", "GG", "!!"), ("e", "TTTT", "JJJJ")]
    found = [(0, 0, 2), (0, 3, 6), (2, 0, 4), (3, 0, 1)]
    assert pr.bins_text(records, found, "ABAUA", True) == ("@a:1-2\nAC\n+\n12\n@a:4-6\nTAC\n+\n456\n@c\nCCCC\n+\nIIII\n", ">b\nAAAA\n", "@d\nGG\n+\n!!\n")


def test_trim_reads_tables_by_hand():
    k = 3
    records = [("r1 c", "AAACCCGGGTTTA", "I" * 13), ("r2", "AC", "II"), ("r3", "CCCCC", ""), ("r4", "AAANAAA", "1234567")]
    db = {ref.canonical("AAA"): 5, ref.canonical("CCG"): 2}
    found, evidence, bins = pr.trim(db, records, k)
    assert (found, bins) == ([(0, 4, 8), (3, 0, 3)], "AUBA") and evidence[0] == (11, 4, 10, 4, 3)
    assert pr.table(records, found, evidence, bins) == "r1\t13\t11\t4\t10\t1\t4\tkept\nr2\t2\t0\t0\t0\t0\t0\tunjudged\nr3\t5\t3\t0\t0\t0\t0\tdropped\nr4\t7\t2\t2\t6\t1\t3\tkept\n"
    assert pr.bed(records, found) == "r1\t4\t8\nr4\t0\t3\n"
    assert pr.summary(records, found, bins, 2, 255, "covered", "longest", 1) == "#kept\t2\t2\t7\n#dropped\t1\t5\n#unjudged\t1\t2\n#cut\t13\n#rule\t2\t255\tcovered\tlongest\t1\n"
    # the other side: r2 has an uncovered piece and no clean window - unjudged all the same; r3 is kept whole
    found, evidence, bins = pr.trim(db, records, k, keep="uncovered", which="all", min_length=2)
    assert (found, bins) == ([(2, 0, 5)], "BUAB")
    assert pr.summary(records, found, bins, 2, 255, "uncovered", "all", 2) == "#kept\t1\t1\t5\n#dropped\t2\t20\n#unjudged\t1\t2\n#cut\t0\n#rule\t2\t255\tuncovered\tall\t2\n"


# ---- against screen_ref.record -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 2, 5, 21, 32))
def test_identities_with_the_evidence(k):
    rng = np.random.default_rng(700 + k)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 900))
    sequences = [genome[:400], "", genome[400:400 + k - 1], genome[420:420 + k], genome[500:800].lower(), "N" * 40, genome[100:300]]
    noisy = list(sequences[0])
    for at in (50, 51, 200, 399):
        noisy[at] = "N"
    sequences.append("".join(noisy))
    windows = [genome[w:w + k] for w in list(range(0, 60)) + list(range(130, 135)) + list(range(380, 400 - k + 1)) + list(range(500, 520)) + [640, 640 + k, 700, 701 + k]]
    db = {ref.canonical(km): 2 + i % 250 for i, km in enumerate(sorted(set(windows)))}
    if k <= 2:
        db = dict(list(sorted(db.items()))[::2])
    counters = sr.window_counters(db, sequences, k)
    lengths = [len(s) for s in sequences]
    some = False
    for min_count, max_count in ((1, 255), (10, 100), (255, 255), (1, 1)):
        m = sr.threshold(min_count)
        covered = pr.pieces_from(counters, lengths, k, min_count, max_count)
        uncovered = pr.pieces_from(counters, lengths, k, min_count, max_count, side="uncovered")
        assert covered == sorted(covered) and uncovered == sorted(uncovered)
        for r, (c, n) in enumerate(zip(counters, lengths)):
            _, _, n_covered, longest, stretches = sr.record(c, n, k, m, max_count)
            mine = [(f, e) for read, f, e in covered if read == r]
            others = [(f, e) for read, f, e in uncovered if read == r]
            assert len(mine) == stretches and sum(e - f for f, e in mine) == n_covered and max([e - f for f, e in mine] + [0]) == longest
            # disjoint, and together they tile [0, L): sorted by first, each begins where the one before ended, sides alternating
            both = sorted([(f, e, True) for f, e in mine] + [(f, e, False) for f, e in others])
            assert [f for f, _, _ in both] == [0] * bool(n) + [e for _, e, _ in both[:-1]] and (both[-1][1] if both else 0) == n
            assert all(a[2] != b[2] for a, b in zip(both, both[1:])) and all(e > f for f, e, _ in both)
            longest_piece = pr.sequence_pieces(c, n, k, m, max_count, which="longest")
            assert longest_piece == [p for p in mine if p[1] - p[0] == longest][:1]  # the first of the longest ones
            for min_length in (0, 1, k, k + 1, 2 * k, 1 << 40):
                assert pr.sequence_pieces(c, n, k, m, max_count, min_length=min_length) == [p for p in mine if p[1] - p[0] >= min_length]
            some = some or (len(mine) > 1 and len(others) > 1)
        assert not (min_count, max_count) == (1, 1) or not covered  # empty after a solid database's floor
    assert some
    assert pr.pieces(db, sequences, k) == pr.pieces_from(counters, lengths, k)
