"""tests/repair_ref.py judged before it judges the device: the rule as a loop (A) against the brute force (B) on seeded random
cases, and both against records worked out by hand at k = 5.  No device."""
import numpy as np
import pytest

import db_query_ref as ref
import repair_ref as rr

K = 5
#        0         1         2         3
#        0123456789012345678901234567890123456789
TRUTH = "CACATAGAGACGCGCATGACACGATACGCAGATAGTAGCA"  # 36 distinct canonical 5-mers, no two equal neighbours
DB = {km: 7 for km in ref.window_kmers(TRUTH, K)}


def _both(db, sequences, k, **kw):
    a, b = rr.repairs(db, sequences, k, **kw), rr.repairs_brute(db, sequences, k, **kw)
    assert a == b
    return a


def test_the_truth_has_no_stretch():
    assert len(set(DB)) == len(TRUTH) - K + 1
    assert _both(DB, [TRUTH, ref.revcomp(TRUTH), TRUTH.lower()], K) == []


def test_an_interior_substitution():
    # base 20 A -> C breaks the k windows 16 .. 20; P = [20], one SUB back to A, seen by all five windows
    s = TRUTH[:20] + "C" + TRUTH[21:]
    assert _both(DB, [s], K) == [(0, 16, 20, 5, 1, rr.SUB, ord("A"), 5, 7)]
    # a lower-case sequence is folded; min_support above k accepts nothing
    assert _both(DB, [s.lower()], K) == [(0, 16, 20, 5, 1, rr.SUB, ord("A"), 5, 7)]
    assert _both(DB, [s], K, min_support=6) == [(0, 16, 0, 5, 0, rr.NONE, 0, 0, 0)]


def test_an_extra_base_inside_a_run_of_three():
    truth = TRUTH[:8] + "TT" + TRUTH[8:]
    db = {km: 7 for km in ref.window_kmers(truth, K)}
    s = TRUTH[:8] + "TTT" + TRUTH[8:]  # the run is bases 8 .. 10
    # the windows that hold all three T start at 6, 7, 8: r = k - 2; P = [8, 10] is the run, and its one DEL is left-aligned to 8;
    # of the edited sequence the windows 4 .. 7 hold both neighbours of the deleted base
    assert _both(db, [s], K) == [(0, 6, 8, 3, 1, rr.DEL, 0, 4, 7)]


def test_a_missing_base():
    s = TRUTH[:20] + TRUTH[21:]  # base 20, an A, is gone: the windows over the joint start at 16 .. 19, r = k - 1
    assert _both(DB, [s], K) == [(0, 16, 20, 4, 1, rr.INS, ord("A"), 5, 7)]


def test_errors_at_both_ends():
    first = "A" + TRUTH[1:]
    assert _both(DB, [first], K) == [(0, 0, 0, 1, 1, rr.SUB, ord("C"), 1, 7)]  # one window holds base 0: support 1 < k
    assert _both(DB, [first], K, min_support=2) == [(0, 0, 0, 1, 0, rr.NONE, 0, 0, 0)]
    # the last base, A -> C: SUB(39, A), and DEL(38) - which leaves ...TAGCC's TAGC + C = the same last window - both with one window
    last = TRUTH[:-1] + "C"
    assert _both(DB, [last], K) == [(0, 35, 39, 1, 2, rr.SUB, ord("A"), 1, 7)]


def test_an_error_two_bases_from_an_n():
    s = TRUTH[:18] + "N" + TRUTH[19] + "C" + TRUTH[21:]  # N at 18, error at 20: the clean windows over 20 start at 19 and 20
    assert _both(DB, [s], K) == [(0, 19, 20, 2, 1, rr.SUB, ord("A"), 2, 7)]


def test_two_errors_closer_than_k_are_long():
    s = TRUTH[:20] + "C" + TRUTH[21:23] + "T" + TRUTH[24:]  # errors at 20 and 23: windows 16 .. 23 hold one of them
    got = _both(DB, [s], K)
    assert got[0] == (0, 16, 0, 8, 0, rr.LONG, 0, 0, 0) and len(got) == 1


def test_counters_below_the_threshold_are_broken():
    db = dict(DB)
    db[ref.canonical(TRUTH[10:15])] = 3
    assert _both(db, [TRUTH], K, min_count=3) == []
    got = _both(db, [TRUTH], K, min_count=4)  # one present window is broken; no edit mends it
    assert [(g[1], g[3], g[5]) for g in got] == [(10, 1, rr.NONE)]
    full = dict(DB)
    full[ref.canonical(TRUTH[10:15])] = 1
    assert _both(full, [TRUTH], K, min_count=1, floor=1) == []
    assert len(_both(full, [TRUTH], K, min_count=2, floor=1)) == 1


def _random_case(rng, k, length):
    """a genome with homopolymer runs of 2 to 9, its database, and a copy with planted one-base errors, N and lower case"""
    genome = []
    while len(genome) < length:
        base = "ACGT"[rng.integers(0, 4)]
        genome += [base] * (int(rng.integers(2, 10)) if rng.random() < 0.3 else 1)
    genome = "".join(genome[:length])
    counters = (2, 3, 7, 40, 255)
    db = {km: counters[(ref.lex_rank(km) + len(km)) % len(counters)] for km in ref.window_kmers(genome, k)}
    s = list(genome)
    for _ in range(max(2, length // (4 * k))):
        at = int(rng.integers(0, len(s)))
        what = rng.integers(0, 5)
        if what == 0:
            s[at] = "ACGT"[rng.integers(0, 4)]
        elif what == 1:
            del s[at]
        elif what == 2:
            s.insert(at, "ACGT"[rng.integers(0, 4)])
        elif what == 3:
            s[at] = "N"
        else:
            s[at] = s[at].lower()
    return db, "".join(s)


@pytest.mark.parametrize("k", (4, 5, 21))
def test_the_rule_equals_the_brute_force(k):
    rng = np.random.default_rng(1700 + k)
    kinds, several = set(), 0
    for case in range(30 if k < 21 else 8):
        db, s = _random_case(rng, k, 60 + 12 * k)
        batch = [s, "", s[:k - 1], ref.revcomp(s.upper().replace("N", "A"))[:3 * k]]
        for min_count, min_support in ((2, 1), (3, k // 2 + 1), (2, k)):
            a = rr.repairs(db, batch, k, min_count, min_support)
            assert a == rr.repairs_brute(db, batch, k, min_count, min_support), (case, min_count, min_support)
            kinds |= {rec[5] for rec in a}
            several += sum(rec[4] > 1 for rec in a)
    assert kinds >= {rr.SUB, rr.DEL, rr.INS}  # not vacuous: every kind of edit
    assert k == 21 or (kinds == {rr.NONE, rr.SUB, rr.DEL, rr.INS, rr.LONG} and several)  # (where runs reach k: ambiguity too)


def test_as_array_and_apply_edits():
    records = rr.as_array([(3, 16, 20, 5, 1, rr.SUB, ord("A"), 5, 7)])
    assert records.dtype.itemsize == 40 and records.tobytes()[24:34] == bytes([5, 0, 0, 0, 1, 0, 1, 65, 5, 7]) and not records["pad"].any()
    assert rr.first_difference(records, records.copy()) is None and rr.first_difference(records, records[:0]) is not None
    assert rr.apply_edits("ACGTACGT", [(rr.SUB, 1, "T"), (rr.DEL, 4, ""), (rr.INS, 7, "G")]) == "ATGTCGGT"
