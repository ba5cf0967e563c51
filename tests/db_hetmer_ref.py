"""The het-mer pairs of a count database by brute force, straight from the definitions in include/tbk.h (tbk_kmerdb_hetmers):
Python integers, strings and dicts, nothing of the library.  Ranks are lexicographic: base 0 in the top bits, A C G T = 0 1 2 3.

Partners: for a canonical k-mer x of odd k, put each of the three other bases at the middle position m = (k - 1) / 2, make each
result canonical (the lexicographic minimum of a k-mer and its reverse complement) and drop x itself; what remains, as a set.
Candidates: entries with a counter in [lo, hi].  A pair: a candidate with exactly one partner among the candidates, and that
partner; minor = the lower counter, on a tie the lower rank; found from its lower-ranked member, in that order."""
import functools

import numpy as np

BASES = "ACGT"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ---- strings ------------------------------------------------------------------------------------------------------------------
def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def canonical(s):
    return min(s, revcomp(s))


def middle_partners(x):
    """the middle partners of the canonical k-mer x, a set of strings"""
    assert len(x) % 2 == 1 and x == canonical(x)
    m = (len(x) - 1) // 2
    return {canonical(x[:m] + b + x[m + 1:]) for b in BASES if b != x[m]} - {x}


def rank_of(s):
    r = 0
    for c in s:
        r = r * 4 + BASES.index(c)
    return r


def kmer_of(rank, k):
    return "".join(BASES[(int(rank) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def all_canonical(k):
    """every canonical k-mer, ascending"""
    return [s for s in (kmer_of(r, k) for r in range(4 ** k)) if s == canonical(s)]


# ---- ranks --------------------------------------------------------------------------------------------------------------------
def revcomp_rank(r, k):
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (r & 3))
        r >>= 2
    return out


def canonical_rank(r, k):
    return min(r, revcomp_rank(r, k))


@functools.lru_cache(maxsize=None)
def partner_ranks(x, k):
    """((rank, kept, flipped), ...) for the middle partners of the canonical rank x, ascending: kept when some variant IS the partner
    (it kept the orientation), flipped when some variant had to be reverse-complemented to give it.  A comparison of a k-mer with
    its reverse complement that the flanks decide does not depend on the middle base, so a variant flips only when the flanks
    mirror each other - and then the partner is both: ACT is AAT's variant as it stands, and the reverse complement of AGT."""
    assert k % 2 == 1
    bit = 2 * ((k - 1) // 2)
    got = {}
    for d in (1, 2, 3):
        v = x ^ (d << bit)
        c = canonical_rank(v, k)
        if c != x:
            kept, flipped = got.get(c, (False, False))
            got[c] = (kept or c == v, flipped or c != v)
    return tuple((c, kept, flipped) for c, (kept, flipped) in sorted(got.items()))


def variant_kinds(x, k):
    """(self_variants, merged_variants) of the canonical rank x: variants that canonicalise to x itself, and variants that
    canonicalise to a k-mer an earlier variant gave"""
    bit = 2 * ((k - 1) // 2)
    canon = [canonical_rank(x ^ (d << bit), k) for d in (1, 2, 3)]
    selfs = sum(c == x for c in canon)
    others = [c for c in canon if c != x]
    return selfs, len(others) - len(set(others))


def _held(db, key, lo_hi):
    if db is None:
        return 0
    c = db.get(key, 0)
    return 1 if lo_hi[0] <= c <= lo_hi[1] else 0


def as_dict(keys, counts):
    return {int(key): int(c) for key, c in zip(keys, counts)}


def hetmers(keys, counts, k, lo, hi, y=None, y_range=(1, 255), z=None, z_range=(1, 255)):
    """What tbk_kmerdb_hetmers returns for the database (keys ascending, counts) and the partners y and z, each None or a dict
    rank -> counter: candidates, partners (4), pairs, spec (256 x 256), origin (4 x 4) and records, a list of
    (minor, major, c_minor, c_major, cls_minor, cls_major) in the order the call hands them out."""
    held = as_dict(keys, counts)
    assert len(held) == len(keys) and all(int(a) < int(b) for a, b in zip(keys[:-1], keys[1:]))
    cand = {key: c for key, c in held.items() if lo <= c <= hi}
    partners = [0, 0, 0, 0]
    spec = np.zeros((256, 256), dtype=np.uint64)
    origin = np.zeros((4, 4), dtype=np.uint64)
    records = []
    for x in sorted(cand):
        inside = [p for p, *_ in partner_ranks(int(x), k) if p in cand]
        partners[len(inside)] += 1
        if len(inside) != 1 or inside[0] < x:
            continue
        p = inside[0]
        assert [q for q, *_ in partner_ranks(p, k) if q in cand] == [x]  # classes are equivalence classes
        minor, major = (x, p) if cand[x] <= cand[p] else (p, x)
        cls = [_held(y, key, y_range) | (_held(z, key, z_range) << 1) for key in (minor, major)]
        spec[cand[minor], cand[major]] += 1
        origin[cls[0], cls[1]] += 1
        records.append((minor, major, cand[minor], cand[major], cls[0], cls[1]))
    return {"candidates": len(cand), "partners": np.array(partners, dtype=np.uint64), "pairs": len(records), "spec": spec, "origin": origin,
            "records": records}


def check_invariants(got):
    """what the class structure makes of any result, the device's included"""
    partners, pairs = [int(v) for v in got["partners"]], int(got["pairs"])
    assert sum(partners) == int(got["candidates"])
    assert partners[1] == 2 * pairs and partners[2] % 3 == 0 and partners[3] % 4 == 0
    spec = np.asarray(got["spec"]).reshape(256, 256)
    assert int(spec.sum()) == pairs and int(np.asarray(got["origin"]).sum()) == pairs
    assert not spec[0].any() and not spec[:, 0].any() and not np.tril(spec, -1).any()
