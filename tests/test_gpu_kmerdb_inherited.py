"""Three count databases to the k-mers a child inherited (tbk_kmerdb_inherited, tbk_kmerdb_inherited_table;
kmers.KmerDatabase.unique / unique_set with ``child=``): of A's k-mers with a counter in range, those B lacks and the child holds
with a counter in the child's range.

Crafted databases are written as tests/test_gpu_kmerdb_table.py writes them, and every expectation is numpy's:
packed_keys(a[(ca in range) & ~isin(a, b) & isin(a, child[cc in range])], k).  The new flag kernel searches B and the child only
between the places where the first and the last rank of a tile of 1024 entries would stand, so beside the partners of the
two-database test there are two that aim at those bounds: `dense_between` packs thousands of the partner's ranks between two
neighbouring entries of A - in the middle of a tile and across a tile's edge - so that the bounded range is many times a tile,
and `one_tile` puts all of the partner inside the span of one tile (the second, where A has one), so that every other tile's
bounds are equal.  `below`, `above` and `equal` put the bounds at 0 and at n.  Counted libraries are checked against
oracle.unique_oracle.count_kmers_np, set for set."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_kmerdb import RANGES, _database, _library, _oracle_counts, _two_parents
from test_gpu_kmerdb_table import EDGE, KS, SIZES, TILE, _counters, _distinct_ranks, _room, _write_db, packed_keys

pytestmark = pytest.mark.gpu

KINDS = ("disjoint", "every_second", "first_and_last", "below", "above", "equal", "dense_between", "one_tile")
CHILD_RANGES = ((2, 255), (1, 255), (5, 12), (9, 3))  # all; clamped to 2; narrow; one that no counter meets
DENSE = 5000                                           # ranks packed into one gap of A: about five tiles' worth
FILE_ROUTE = {2: 4, 5: 500, 16: 3 * TILE + 17, 17: TILE + 1, 21: 3 * TILE + 17, 31: TILE - 1, 32: TILE + 1}  # k -> the size whose dumps are read back


def _cases():
    """the cases of test_gpu_kmerdb_table: every k at every size it has room for, the several-hundred-tile database at k = 21 and 32"""
    return [(k, n) for k in KS for n in SIZES if 2 * n <= _room(k) and (n < 100 * TILE or k in (21, 32))] + [(2, 4), (5, 500)]


def _craft_a(k, n_a, top_rank=False):
    """A (ranks, counters) and as many ranks A lacks; with top_rank the last entry of A is 2^64 - 1 (k = 32)"""
    rng = np.random.default_rng(7000 * k + n_a)
    both = _distinct_ranks(rng, k, 2 * n_a)
    pick = np.zeros(2 * n_a, dtype=bool)
    pick[rng.permutation(2 * n_a)[:n_a]] = True
    a, rest = both[pick], both[~pick]
    if top_rank:
        assert k == 32
        a[-1] = np.uint64((1 << 64) - 1)
        rest = rest[rest < a[-1]]
    assert (a[1:] > a[:-1]).all() and int(a[0]) >= EDGE
    return rng, a, rest, _counters(rng, n_a)


def _between(a, i, m, top):
    """up to m consecutive ranks above a[i] and below a[i + 1] (up to the top rank when a[i] is A's last entry)"""
    room = (int(a[i + 1]) if i + 1 < a.size else top + 1) - int(a[i]) - 1
    return np.uint64(int(a[i]) + 1) + np.arange(max(0, min(m, room)), dtype=np.uint64)


def _partners(k, a, rest):
    top = (1 << (2 * k)) - 1
    low = np.array([0, 1, 3], dtype=np.uint64)
    n = a.size
    # the widest gap among the entries in the middle of the first tile, and the gap that straddles the first tile's edge
    first = min(n, TILE)
    inner = np.arange(first // 4, max(3 * first // 4, first // 4 + 1))
    gaps = a[np.minimum(inner + 1, n - 1)] - a[inner]
    mid = int(inner[int(np.argmax(gaps))])
    dense = [_between(a, mid, DENSE, top), a[mid:mid + 2], a[::5]]
    if n > TILE:
        dense += [_between(a, TILE - 1, DENSE, top), a[TILE - 1:TILE + 1]]
    tile = a[TILE:2 * TILE] if n > TILE else a
    inside = rest[(rest > tile[0]) & (rest < tile[-1])]
    return {
        "disjoint": rest,
        "every_second": a[::2],
        "first_and_last": np.unique(a[[0, -1]]),
        "below": low,
        "above": np.uint64(top) - low[::-1],
        "equal": a,
        "dense_between": np.unique(np.concatenate(dense)),
        "one_tile": np.unique(np.concatenate([tile[::2], inside])),
    }


def _in_range(c, lo, hi):
    return (c >= max(2, lo)) & (c <= min(255, hi))


def _check_set(da, db, dc, lo, hi, clo, chi, want, k, what):
    if want.size == 0:
        with pytest.raises(ValueError, match="empty k-mer list"):
            da.unique_set(db, lo, hi, child=dc, child_min=clo, child_max=chi)
        return
    with da.unique_set(db, lo, hi, child=dc, child_min=clo, child_max=chi) as hs:
        assert (hs.num_kmers, hs.k, hs.device, hs.origin) == (want.size, k, da.device, "databases"), what
        got = hs.keys()
        assert got.dtype == np.uint64 and np.array_equal(got, want), (what, int(np.argmax(got != want)) if got.size == want.size else got.size)


def _check_file(da, db, dc, lo, hi, clo, chi, ranks, k, path, what):
    """the file route byte for byte: the text of those ranks, one k-mer per line"""
    from oracle import unique_oracle as uo

    n = da.unique(db, lo, hi, str(path), child=dc, child_min=clo, child_max=chi)
    want = "".join(s + "\n" for s in uo.kmer_strings(ranks, k)).encode()
    assert n == ranks.size and open(path, "rb").read() == want, what


def _run_pairs(tmp_path, k, a, ca, partners, pairs, a_ranges, dump):
    """Every (B kind, child kind) of `pairs` at every A range and child range; `dump`: these also through the file route.
    Returns how many selections were sets and how many empty."""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(k + a.size)
    files, counters = {}, {}
    for kind in sorted({kind for pair in pairs for kind in pair}):
        counters[kind] = _counters(rng, partners[kind].size)
        files[kind] = _write_db(tmp_path / (kind + ".tbkdb"), k, partners[kind], counters[kind])
    seen = {"sets": 0, "empty": 0}
    with kmers.KmerDatabase.load(_write_db(tmp_path / "a.tbkdb", k, a, ca)) as da:
        for kind_b, kind_c in pairs:
            b, child, cc = partners[kind_b], partners[kind_c], counters[kind_c]
            with kmers.KmerDatabase.load(files[kind_b]) as db, kmers.KmerDatabase.load(files[kind_c]) as dc:
                absent = ~np.isin(a, b)
                for clo, chi in CHILD_RANGES:
                    held = np.isin(a, child[_in_range(cc, clo, chi)])
                    for lo, hi in a_ranges:
                        ranks = a[_in_range(ca, lo, hi) & absent & held]
                        seen["empty" if ranks.size == 0 else "sets"] += 1
                        what = (kind_b, kind_c, lo, hi, clo, chi)
                        _check_set(da, db, dc, lo, hi, clo, chi, packed_keys(ranks, k), k, what)
                        if dump and (lo, hi) in ((2, 255), (3, 20), (9, 3)):
                            _check_file(da, db, dc, lo, hi, clo, chi, ranks, k, tmp_path / "dump.txt", what)
                # the databases are as they were
                assert np.array_equal(da.entries()[0], a) and np.array_equal(da.entries()[1], ca)
                assert np.array_equal(db.entries()[0], b) and np.array_equal(dc.entries()[0], child) and np.array_equal(dc.entries()[1], cc)
    return seen


@pytest.mark.parametrize("k,n_a", _cases())
def test_crafted_databases(gpu, tmp_path, k, n_a):
    """Each kind once as B and once as the child at every size: kind j of B meets kind j + shift of the child."""
    rng, a, rest, ca = _craft_a(k, n_a, top_rank=(k == 32 and n_a == TILE + 1))
    if k == 32 and n_a >= 63:
        assert int(a[-1]) >> 63 == 1 and int(a[0]) >> 63 == 0
    partners = _partners(k, a, rest)
    if k >= 16 and n_a > TILE:  # where k has the room, the bounded range really is many times a tile, twice
        d = partners["dense_between"]
        assert ((d > a[TILE - 1]) & (d < a[TILE])).sum() == DENSE and d.size >= 2 * DENSE + n_a // 5
        assert np.isin(a[TILE:2 * TILE:2], partners["one_tile"]).all() and partners["one_tile"][0] == a[TILE]
    shift = 1 + (k + n_a) % (len(KINDS) - 1)
    pairs = [(KINDS[j], KINDS[(j + shift) % len(KINDS)]) for j in range(len(KINDS))]
    a_ranges = RANGES if n_a <= TILE + 1 else ((2, 255), (3, 20))
    seen = _run_pairs(tmp_path, k, a, ca, partners, pairs, a_ranges, dump=FILE_ROUTE[k] == n_a)
    assert seen["empty"] >= len(pairs) * len(a_ranges) and (seen["sets"] > 0 or n_a <= 4)


def test_every_kind_meets_every_other(gpu, tmp_path):
    """n = 1025 (one whole tile and a tile of one entry) at k = 21: the full cross of B's kinds and the child's."""
    k, n_a = 21, TILE + 1
    rng, a, rest, ca = _craft_a(k, n_a)
    partners = _partners(k, a, rest)
    pairs = [(kb, kc) for kb in KINDS for kc in KINDS]
    seen = _run_pairs(tmp_path, k, a, ca, partners, pairs, ((2, 255), (3, 20)), dump=False)
    assert seen["sets"] >= 100 and seen["empty"] >= 2 * len(pairs)


def test_the_child_equal_to_a_changes_nothing(gpu, tmp_path):
    """With A itself as the child at [2,255] the third condition always holds: the list is today's unique_set(b, lo, hi)."""
    from trio_binning_amd import kmers

    k, n_a = 21, 3 * TILE + 17
    rng, a, rest, ca = _craft_a(k, n_a)
    partners = _partners(k, a, rest)
    with kmers.KmerDatabase.load(_write_db(tmp_path / "a.tbkdb", k, a, ca)) as da, \
            kmers.KmerDatabase.load(_write_db(tmp_path / "child.tbkdb", k, a, ca)) as dc:
        for kind in ("every_second", "dense_between", "one_tile", "disjoint"):
            b = partners[kind]
            with kmers.KmerDatabase.load(_write_db(tmp_path / "b.tbkdb", k, b, _counters(rng, b.size))) as db:
                for lo, hi in ((2, 255), (3, 20), (5, 5)):
                    want = packed_keys(a[_in_range(ca, lo, hi) & ~np.isin(a, b)], k)
                    assert want.size > 0
                    with da.unique_set(db, lo, hi) as two, da.unique_set(db, lo, hi, child=dc) as three, da.unique_set(db, lo, hi, child=da) as own:
                        assert np.array_equal(two.keys(), want) and np.array_equal(three.keys(), want) and np.array_equal(own.keys(), want)
                        assert three.num_kmers == two.num_kmers and three.origin == two.origin == "databases"


def test_refusals_leave_no_table_and_sound_databases(gpu, tmp_path):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(6)
    a21, a16 = _distinct_ranks(rng, 21, 100), _distinct_ranks(rng, 16, 100)
    c21, c16 = _counters(rng, 100), _counters(rng, 100)
    lib = gpu.lib
    with kmers.KmerDatabase.load(_write_db(tmp_path / "a21.tbkdb", 21, a21, c21)) as d21, \
            kmers.KmerDatabase.load(_write_db(tmp_path / "b21.tbkdb", 21, a21[::2], c21[::2])) as half, \
            kmers.KmerDatabase.load(_write_db(tmp_path / "a16.tbkdb", 16, a16, c16)) as d16:
        out = str(tmp_path / "no.txt").encode()
        for trio in ((d21, half, d16), (d21, d16, half), (d16, d21, half)):
            h, n = C.c_void_p(1), C.c_uint64(5)
            rc = lib.tbk_kmerdb_inherited_table(trio[0]._h, trio[1]._h, trio[2]._h, 2, 255, 2, 255, C.byref(h))
            assert rc == gpu.TBK_ERR_INVALID and "different k" in gpu.last_error() and not h.value
            rc = lib.tbk_kmerdb_inherited(trio[0]._h, trio[1]._h, trio[2]._h, 2, 255, 2, 255, out, C.byref(n))
            assert rc == gpu.TBK_ERR_INVALID and "different k" in gpu.last_error() and not (tmp_path / "no.txt").exists()
        for trio in ((None, half._h, d21._h), (d21._h, None, d21._h), (d21._h, half._h, None)):
            h, n = C.c_void_p(1), C.c_uint64(5)
            assert lib.tbk_kmerdb_inherited_table(trio[0], trio[1], trio[2], 2, 255, 2, 255, C.byref(h)) == gpu.TBK_ERR_INVALID and not h.value
            assert lib.tbk_kmerdb_inherited(trio[0], trio[1], trio[2], 2, 255, 2, 255, out, C.byref(n)) == gpu.TBK_ERR_INVALID
        assert lib.tbk_kmerdb_inherited_table(d21._h, half._h, d21._h, 2, 255, 2, 255, None) == gpu.TBK_ERR_INVALID
        assert lib.tbk_kmerdb_inherited(d21._h, half._h, d21._h, 2, 255, 2, 255, None, C.byref(n)) == gpu.TBK_ERR_INVALID
        # an empty selection: the list refuses as an empty list file does, the file is empty
        h = C.c_void_p(1)
        rc = lib.tbk_kmerdb_inherited_table(d21._h, d21._h, d21._h, 2, 255, 2, 255, C.byref(h))
        assert rc == gpu.TBK_ERR_FORMAT and "empty k-mer list" in gpu.last_error() and not h.value
        assert d21.unique(d21, 2, 255, str(tmp_path / "empty.txt"), child=d21) == 0 and (tmp_path / "empty.txt").read_bytes() == b""
        with pytest.raises(ValueError, match="different k"):
            d21.unique_set(half, 2, 255, child=d16)
        # a child that holds nothing leaves nothing; a B that holds nothing takes nothing away
        with kmers.KmerDatabase.load(_write_db(tmp_path / "none.tbkdb", 21, a21[:0], np.zeros(0, dtype=np.uint8))) as none:
            with pytest.raises(ValueError, match="empty k-mer list"):
                d21.unique_set(half, 2, 255, child=none)
            assert d21.unique(half, 2, 255, str(tmp_path / "empty.txt"), child=none) == 0
            with d21.unique_set(none, 2, 255, child=half) as hs:
                assert np.array_equal(hs.keys(), packed_keys(a21[::2], 21))
        # a closed handle is refused like a NULL one
        closed = kmers.KmerDatabase.load(str(tmp_path / "b21.tbkdb"))
        closed.close()
        for trio in ((closed, half, d21), (d21, closed, d21), (d21, half, closed)):
            with pytest.raises(ValueError):
                trio[0].unique_set(trio[1], 2, 255, child=trio[2])
            with pytest.raises(ValueError):
                trio[0].unique(trio[1], 2, 255, str(tmp_path / "no.txt"), child=trio[2])
        assert not (tmp_path / "no.txt").exists()
        # after each of these the databases still answer
        assert np.array_equal(d21.entries()[0], a21) and np.array_equal(half.entries()[0], a21[::2]) and np.array_equal(d16.entries()[1], c16)
        with d21.unique_set(half, 2, 255, child=d21) as hs:
            assert np.array_equal(hs.keys(), packed_keys(a21[1::2], 21))


# ---- counted libraries: set for set against the oracle's counts of the three libraries --------------------------------------
def _second_haplotype(rng, genome, snp=1 / 150):
    """the parent's other haplotype: the same genome with a SNP every 150 bases or so"""
    s = list(genome)
    for i in np.nonzero(rng.random(len(s)) < snp)[0]:
        s[int(i)] = "ACGT"[("ACGT".index(s[int(i)]) + int(rng.integers(1, 4))) % 4]
    return "".join(s)


@functools.lru_cache(maxsize=None)
def _trio(k):
    """Each parent's library is read from its two haplotypes; the child's from the first haplotype of each parent, at half the
    per-read error rate and about 9x per haplotype: what a parent holds on its second haplotype alone, the child lacks."""
    rng = np.random.default_rng(900 + k)
    ga, gb = _two_parents(rng, glen=8_000)
    ga2, gb2 = _second_haplotype(rng, ga), _second_haplotype(rng, gb)
    reads_a = _library(rng, ga, 450, 150, lower=0.1) + _library(rng, ga2, 450, 150)
    reads_b = _library(rng, gb, 400, 150) + _library(rng, gb2, 400, 150)
    reads_c = _library(rng, ga, 500, 150, err=0.005) + _library(rng, gb, 500, 150, err=0.005) + ["", "N" * 40, ga[:k]]
    return {"a": reads_a, "b": reads_b, "child": reads_c,
            "na": _oracle_counts(reads_a, k), "nb": _oracle_counts(reads_b, k), "nc": _oracle_counts(reads_c, k)}


def _inherited_np(a, b, child, lo, hi, clo, chi):
    """the selection on the oracle's (keys, counts) of three libraries, as ascending ranks"""
    (ka, ca), (kb, cb), (kc, cc) = a, b, child
    capped, child_capped = np.minimum(ca, 255), np.minimum(cc, 255)
    keep = (ca >= 2) & (capped >= lo) & (capped <= hi)
    held = (cc >= 2) & (child_capped >= clo) & (child_capped <= chi)
    return ka[keep & ~np.isin(ka, kb[cb >= 2]) & np.isin(ka, kc[held])]


@pytest.mark.parametrize("k", [21, 32])
@pytest.mark.parametrize("passes", [1, 3])
def test_counted_libraries_equal_the_oracle(gpu, tmp_path, k, passes):
    from oracle import unique_oracle as uo

    trio = _trio(k)
    with _database(trio["a"], k, passes) as da, _database(trio["b"], k, passes) as db, _database(trio["child"], k, passes) as dc:
        for (lo, hi), (clo, chi) in (((2, 255), (2, 255)), ((3, 200), (3, 255)), ((5, 60), (1, 30))):
            for x, y, nx, ny, name in ((da, db, trio["na"], trio["nb"], "a"), (db, da, trio["nb"], trio["na"], "b")):
                ranks = _inherited_np(nx, ny, trio["nc"], lo, hi, clo, chi)
                both = uo.unique_np(nx, ny, lo, hi)
                assert 100 < ranks.size < both.size - 100, "the child must hold many of a parent's own k-mers and lack many"
                with x.unique_set(y, lo, hi, child=dc, child_min=clo, child_max=chi) as hs:
                    assert np.array_equal(hs.keys(), packed_keys(ranks, k)) and hs.num_kmers == ranks.size
                path = tmp_path / (name + ".txt")
                assert x.unique(y, lo, hi, str(path), child=dc, child_min=clo, child_max=chi) == ranks.size
                assert open(path).read().split("\n")[:-1] == uo.kmer_strings(ranks, k)
