"""The brute-force reference of the het-mer pairs (tests/db_hetmer_ref.py) against cases worked by hand, and the class structure
include/tbk.h states - partner classes are equivalence classes of 4 or 2 canonical k-mers - over every canonical k-mer of
k = 1, 3, 5 (and 7) and over random subsets with random counters.  No device."""
import numpy as np
import pytest

import db_hetmer_ref as ref


def _db(entries):
    """{kmer: counter} -> (ascending ranks, counters)"""
    pairs = sorted((ref.rank_of(s), c) for s, c in entries.items())
    return np.array([p[0] for p in pairs], dtype=np.uint64), np.array([p[1] for p in pairs], dtype=np.uint8)


def _run(entries, lo, hi, **kw):
    k = len(next(iter(entries)))
    assert all(s == ref.canonical(s) and len(s) == k for s in entries)
    got = ref.hetmers(*_db(entries), k, lo, hi, **kw)
    ref.check_invariants(got)
    got["named"] = [(ref.kmer_of(a, k), ref.kmer_of(b, k), ca, cb, sa, sb) for a, b, ca, cb, sa, sb in got["records"]]
    return got


def test_strings_and_ranks_agree():
    for k in (1, 3, 5):
        for s in ref.all_canonical(k):
            r = ref.rank_of(s)
            assert ref.kmer_of(r, k) == s and ref.kmer_of(ref.revcomp_rank(r, k), k) == ref.revcomp(s) and ref.canonical_rank(r, k) == r
            assert {ref.kmer_of(p, k) for p, *_ in ref.partner_ranks(r, k)} == ref.middle_partners(s)
    # kept: the partner is a variant as it stands; flipped: it is a variant's reverse complement - with mirrored flanks alone
    assert ref.partner_ranks(ref.rank_of("AAA"), 3) == tuple((ref.rank_of(s), True, False) for s in ("ACA", "AGA", "ATA"))
    assert ref.partner_ranks(ref.rank_of("CAG"), 3) == ((ref.rank_of("CCG"), True, True),)  # CCG; CGG flips to CCG; CTG is CAG itself
    for k in (3, 5, 7):
        m = (k - 1) // 2
        for s in ref.all_canonical(k):
            flips = any(flipped for _, _, flipped in ref.partner_ranks(ref.rank_of(s), k))
            assert flips == (ref.revcomp(s[:m]) == s[m + 1:])


def test_k1_is_one_class_of_two():
    assert ref.all_canonical(1) == ["A", "C"] and ref.middle_partners("A") == {"C"} and ref.middle_partners("C") == {"A"}
    got = _run({"A": 7, "C": 3}, 1, 255)
    assert (got["candidates"], got["pairs"], list(got["partners"])) == (2, 1, [0, 2, 0, 0])
    assert got["named"] == [("C", "A", 3, 7, 0, 0)] and got["spec"][3, 7] == 1 and got["origin"][0, 0] == 1
    assert _run({"A": 7, "C": 3}, 4, 255)["pairs"] == 0  # C out of range: A is a candidate without a partner
    assert list(_run({"A": 7, "C": 3}, 4, 255)["partners"]) == [1, 0, 0, 0]


def test_aat_has_the_single_partner_act():
    # ATT is AAT's reverse complement (a variant that is the k-mer itself); ACT and AGT are one canonical k-mer (merged variants)
    assert ref.middle_partners("AAT") == {"ACT"} and ref.middle_partners("ACT") == {"AAT"}
    assert ref.variant_kinds(ref.rank_of("AAT"), 3) == (1, 1) and ref.variant_kinds(ref.rank_of("ACT"), 3) == (1, 1)
    got = _run({"AAT": 20, "ACT": 22, "CCC": 9}, 2, 255)
    assert got["named"] == [("AAT", "ACT", 20, 22, 0, 0)] and list(got["partners"]) == [1, 2, 0, 0]


def test_a_class_of_four_with_one_member_out_of_range_is_a_triple_and_no_pair():
    four = {"AAA": 10, "ACA": 11, "AGA": 12, "ATA": 13}
    assert ref.middle_partners("AAA") == {"ACA", "AGA", "ATA"}
    whole = _run(four, 1, 255)
    assert list(whole["partners"]) == [0, 0, 0, 4] and whole["pairs"] == 0
    triple = _run(four, 1, 12)
    assert triple["candidates"] == 3 and list(triple["partners"]) == [0, 0, 3, 0] and triple["pairs"] == 0
    two = _run(four, 11, 12)
    assert list(two["partners"]) == [0, 2, 0, 0] and two["named"] == [("ACA", "AGA", 11, 12, 0, 0)]
    one = _run(four, 13, 13)
    assert list(one["partners"]) == [1, 0, 0, 0] and one["pairs"] == 0


def test_minor_is_the_lower_counter_and_on_a_tie_the_lower_rank():
    assert _run({"ACA": 30, "AGA": 30}, 1, 255)["named"] == [("ACA", "AGA", 30, 30, 0, 0)]
    assert _run({"ACA": 31, "AGA": 30}, 1, 255)["named"] == [("AGA", "ACA", 30, 31, 0, 0)]
    got = _run({"ACA": 31, "AGA": 30}, 1, 255)
    assert got["spec"][30, 31] == 1 and got["spec"].sum() == 1


def test_classes_of_the_members_come_from_the_partners_ranges():
    y = {ref.rank_of("ACA"): 5, ref.rank_of("AGA"): 1}
    z = {ref.rank_of("AGA"): 200}
    got = _run({"ACA": 31, "AGA": 30, "CCC": 4}, 1, 255, y=y, y_range=(2, 255), z=z, z_range=(1, 255))
    assert got["named"] == [("AGA", "ACA", 30, 31, 2, 1)] and got["origin"][2, 1] == 1  # y's AGA is below y's range
    got = _run({"ACA": 31, "AGA": 30}, 1, 255, y=y, z=z, z_range=(1, 199))
    assert got["named"] == [("AGA", "ACA", 30, 31, 1, 1)]
    assert _run({"ACA": 31, "AGA": 30}, 1, 255, z=z)["named"] == [("AGA", "ACA", 30, 31, 2, 0)]  # y not given: bit 0 stays 0


def test_records_come_in_the_order_of_the_lower_ranked_member():
    entries = {"AAT": 9, "ACT": 3, "ACA": 2, "AGA": 8, "AAC": 5}
    got = _run(entries, 1, 255)
    assert got["named"] == [("ACT", "AAT", 3, 9, 0, 0), ("ACA", "AGA", 2, 8, 0, 0)]  # found from AAT (rank 3), then from ACA (rank 4)


@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_partner_classes_are_equivalence_classes_of_four_or_two(k):
    every = ref.all_canonical(k)
    partners = {s: ref.middle_partners(s) for s in every}
    m = (k - 1) // 2
    sizes = set()
    for s, ps in partners.items():
        flanks_mirror = ref.revcomp(s[:m]) == s[m + 1:]
        assert len(ps) == (1 if flanks_mirror else 3)
        for p in ps:
            assert s in partners[p]                      # symmetric
            assert partners[p] | {p} == ps | {s}         # transitive: one class
        sizes.add(len(ps) + 1)
    assert sizes == ({2} if k == 1 else {2, 4})
    if k == 1:
        assert every == ["A", "C"]


@pytest.mark.parametrize("k", [3, 5])
def test_invariants_over_random_subsets(k):
    every = [ref.rank_of(s) for s in ref.all_canonical(k)]
    rng = np.random.default_rng(40 + k)
    kinds = set()
    for trial in range(60):
        keep = rng.random(len(every)) < rng.choice([0.2, 0.5, 0.9, 1.0])
        keys = np.array([r for r, on in zip(every, keep) if on], dtype=np.uint64)
        counts = rng.integers(1, 256, keys.size).astype(np.uint8)
        lo = int(rng.integers(1, 200))
        hi = int(rng.integers(lo, 256))
        got = ref.hetmers(keys, counts, k, lo, hi)
        ref.check_invariants(got)
        assert got["pairs"] == len(got["records"])
        firsts = [min(a, b) for a, b, *_ in got["records"]]
        assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)
        for a, b, ca, cb, *_ in got["records"]:
            assert ca < cb or (ca == cb and a < b)
        kinds |= {j for j in range(4) if got["partners"][j]}
    assert kinds == {0, 1, 2, 3}
