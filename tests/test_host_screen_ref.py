"""tests/screen_ref.py held to a second formulation and to hand-worked records, before it judges the device.  The second
formulation never looks at a base: every held window is an interval [w, w + k - 1]; the sorted intervals are merged where one
begins at most one past the end of the union so far; covered is the sum of the merged lengths, longest their maximum, stretches
their number."""
import numpy as np
import pytest

import db_query_ref as ref
import screen_ref as sr


def _by_intervals(db, sequence, k, m, max_count):
    windows = ref.window_kmers(sequence, k)
    clean = [w for w, km in enumerate(windows) if km is not None]
    held = [w for w in clean if m <= db.get(windows[w], 0) <= max_count]
    merged = []
    for lo, hi in sorted((w, w + k - 1) for w in held):
        if merged and lo <= merged[-1][1] + 1:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    lengths = [hi - lo + 1 for lo, hi in merged]
    assert all(hi < len(sequence) for _, hi in merged)  # coverage never reaches past the sequence's end
    return len(clean), len(held), sum(lengths), max(lengths, default=0), len(lengths)


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


@pytest.mark.parametrize("k", (1, 2, 3, 5, 8, 21, 32))
def test_the_two_formulations_agree(k):
    rng = np.random.default_rng(2600 + k)
    genome = _seq(rng, 700)
    kept = sorted({km for i, km in enumerate(ref.window_kmers(genome, k)) if (i // 7) % 3 != 1})
    if k <= 5:
        kept = kept[::3]
    db = {km: (1, 2, 5, 10, 20, 127, 255)[i % 7] for i, km in enumerate(kept)}
    noisy = list(genome[100:500])
    for at in (0, 57, 58, 200, 399):
        noisy[at] = "N"
    sequences = [genome, "", genome[5:5 + max(k - 1, 0)], genome[9:9 + k], genome[20:20 + k + 1], "".join(noisy), genome[300:600].lower(),
                 ref.revcomp(genome[50:650]), "N" * (2 * k), _seq(rng, 300)]
    some = 0
    for floor in (1, 2):
        for min_count, max_count in ((1, 255), (10, 20), (255, 255), (1, 1), (2, 2), (3, 200)):
            m = sr.threshold(min_count, floor)
            got = sr.evidence(db, sequences, k, min_count, max_count, floor)
            assert got == [_by_intervals(db, s, k, m, max_count) for s in sequences], (k, floor, min_count, max_count)
            assert got[1] == got[2] == (0,) * 5 and got[8] == (0,) * 5
            if (floor, min_count, max_count) == (2, 1, 1):
                assert all(r[1:] == (0, 0, 0, 0) for r in got)  # a range that is empty after the floor holds nothing
            some += sum(r[4] > 1 for r in got)
    assert some  # not vacuous: sequences with several stretches


def test_hand_worked_records():
    k = 3
    #    positions 0123456789
    s = "ACGTTGCAAT"
    # windows: ACG CGT GTT TTG TGC GCA CAA AAT; canonical: ACG ACG AAC CAA GCA GCA CAA AAT
    assert ref.window_kmers(s, k) == ["ACG", "ACG", "AAC", "CAA", "GCA", "GCA", "CAA", "AAT"]
    db = {"ACG": 5, "CAA": 2, "AAT": 1}
    # floor 2, (1, 255): held windows 0, 1, 3, 6 -> covered 0..5 and 6..8: positions 0..8, one stretch of 9
    assert sr.evidence(db, [s], k) == [(8, 4, 9, 9, 1)]
    # (5, 255): held windows 0, 1 -> covered 0..3
    assert sr.evidence(db, [s], k, 5, 255) == [(8, 2, 4, 4, 1)]
    # (1, 2): m = 2, held windows 3 and 6 -> covered 3..5 and 6..8, which touch: exactly k apart is one stretch of 2k
    assert sr.evidence(db, [s], k, 1, 2) == [(8, 2, 6, 6, 1)]
    # a full database, (1, 1): only AAT, the last window -> covered 7..9, up to the sequence's last base
    assert sr.evidence(db, [s], k, 1, 1, floor=1) == [(8, 1, 3, 3, 1)]
    # the same on a solid one: nothing
    assert sr.evidence(db, [s], k, 1, 1) == [(8, 0, 0, 0, 0)]
    # k + 1 apart: two stretches.  Windows of ACGNNACG..: an N takes its k windows out of `clean`
    t = "ACGAACGT"  # windows ACG CGA GAA AAC ACG CGT -> canonical ACG CGA GAA AAC ACG ACG
    assert sr.evidence({"ACG": 9}, [t], k) == [(6, 3, 7, 4, 2)]  # held 0, 4, 5: covered 0..2 and 4..7
    u = "ACGNACG"
    assert sr.evidence({"ACG": 9}, [u], k) == [(2, 2, 6, 3, 2)]
    # lower case folds; the reverse complement is the same k-mer; nothing joins across sequences
    assert sr.evidence({"ACG": 9}, ["acg", "CGT", "AC", ""], k) == [(1, 1, 3, 3, 1), (1, 1, 3, 3, 1), (0,) * 5, (0,) * 5]


def test_the_rule_and_the_tables():
    rec = (10, 5, 40, 25, 2)
    assert sr.bin_of(rec, 100) == "A"
    assert sr.bin_of((0, 0, 0, 0, 0), 100) == "U"
    assert sr.bin_of((10, 0, 0, 0, 0), 100) == "B"  # min_hits 1
    assert sr.bin_of((10, 0, 0, 0, 0), 100, min_hits=0) == "A"
    assert sr.bin_of(rec, 100, min_share="0.5") == "A" and sr.bin_of(rec, 100, min_share="0.500000001") == "B"
    assert sr.bin_of(rec, 100, min_covered="0.4") == "A" and sr.bin_of(rec, 100, min_covered="0.41") == "B"
    assert sr.bin_of(rec, 100, min_stretch=25) == "A" and sr.bin_of(rec, 100, min_stretch=26) == "B"
    assert sr.bin_of((3, 1, 3, 3, 1), 9, min_share="0.333333333") == "A" and sr.bin_of((3, 1, 3, 3, 1), 9, min_share="0.333333334") == "B"
    assert sr.table(["r1", "r2"], ["ACGT" * 25, "AC"], [rec, (0,) * 5], "AU") == "r1\t100\t10\t5\t40\t25\t2\tmatched\nr2\t2\t0\t0\t0\t0\t0\tunjudged\n"
    assert sr.summary(["ACGT", "AC", "A", "ACG"], "AUBA", 2, 255, 1, "0.5", "0", 0) == \
        "#matched\t2\t7\n#unmatched\t1\t1\n#unjudged\t1\t2\n#rule\t2\t255\t1\t0.5\t0\t0\n"
