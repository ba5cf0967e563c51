"""tests/rank_db.py against a plain dict {canonical k-mer: counter}: the same answers for present and absent k-mers, asked with
the canonical k-mer or through db_query_ref.canonical, the first and the last entry found, and the references that take it
(repair_ref, screen_ref) answering as they do on the dict.  No device."""
import numpy as np
import pytest

import db_query_ref as ref
import rank_db
import repair_ref as rr
import screen_ref as sr


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _pair(k, seed, n=300):
    """(dict, RankDb) of a few hundred random canonical k-mers, and the random k-mers they were made from"""
    rng = np.random.default_rng(seed)
    drawn = [_seq(rng, k) for _ in range(n)]
    plain = {ref.canonical(km): int(c) for km, c in zip(drawn, rng.integers(1, 256, n))}
    ranks = np.array(sorted(ref.lex_rank(km) for km in plain), dtype=np.uint64)
    by_rank = {ref.lex_rank(km): c for km, c in plain.items()}
    counters = np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
    return plain, rank_db.RankDb(ranks, counters, k), drawn, rng


@pytest.mark.parametrize("k", (5, 21))
def test_the_mapping_answers_as_a_dict_does(k):
    plain, db, drawn, rng = _pair(k, 50 + k)
    assert len(db) == len(plain) > 100
    others = [_seq(rng, k) for _ in range(300)]
    absent = [km for km in others if ref.canonical(km) not in plain]
    assert len(absent) > (20 if k == 5 else 290)  # (of the 512 canonical 5-mers the dict holds about a third)
    for km in drawn + others:
        c = ref.canonical(km)
        assert db.get(c, 0) == plain.get(c, 0) and (c in db) == (c in plain), km
        assert db.get(ref.canonical(ref.revcomp(km)), 0) == plain.get(c, 0), km  # either strand leads to the same entry
        assert db.get(c) == plain.get(c) and db.get(c, 7) == plain.get(c, 7), km
    for km in absent:
        assert db.get(ref.canonical(km), 0) == 0 and ref.canonical(km) not in db
        with pytest.raises(KeyError):
            db[ref.canonical(km)]
    for km, c in plain.items():
        assert db[km] == c
    # the first and the last entry, and their neighbours in rank
    first, last = min(plain, key=ref.lex_rank), max(plain, key=ref.lex_rank)
    assert rank_db.kmer_string(db.ranks[0], k) == first and rank_db.kmer_string(db.ranks[-1], k) == last
    assert db.get(first, 0) == plain[first] > 0 and db.get(last, 0) == plain[last] > 0
    for rank in (int(db.ranks[0]) - 1, int(db.ranks[-1]) + 1):
        if 0 <= rank < 1 << (2 * k):
            assert db.get(rank_db.kmer_string(rank, k), 0) == 0
    # a k-mer of another length is no entry
    assert db.get("A" * (k + 1), 0) == 0 and "A" * (k - 1) not in db


def test_an_empty_mapping():
    db = rank_db.RankDb(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), 5)
    assert len(db) == 0 and db.get("AAAAA", 0) == 0 and "AAAAA" not in db


@pytest.mark.parametrize("k", (5, 21))
def test_the_references_answer_on_it_as_on_the_dict(k):
    rng = np.random.default_rng(70 + k)
    genome = _seq(rng, 260)
    plain = {km: 2 + (ref.lex_rank(km) % 9) for i, km in enumerate(ref.window_kmers(genome, k)) if i % 7}
    ranks = np.array(sorted(ref.lex_rank(km) for km in plain), dtype=np.uint64)
    by_rank = {ref.lex_rank(km): c for km, c in plain.items()}
    db = rank_db.RankDb(ranks, [by_rank[int(r)] for r in ranks], k)
    hurt = genome[:100] + "G" + genome[100:200].lower() + "N" + genome[201:]
    batch = [hurt, ref.revcomp(genome[50:120]), "", genome[:k - 1]]
    assert rr.repairs(db, batch, k, 2, 1) == rr.repairs(plain, batch, k, 2, 1)
    assert rr.repairs(db, batch, k, 5, 2) == rr.repairs(plain, batch, k, 5, 2) != []
    assert sr.evidence(db, batch, k, 1, 255) == sr.evidence(plain, batch, k, 1, 255)
    assert sr.evidence(db, batch, k, 4, 6) == sr.evidence(plain, batch, k, 4, 6)
