"""Full count databases on the device (include/tbk.h): tbk_kmerdb_union, tbk_kmerdb_solid, what the subtractions and the
query session do with a full database.

Crafted databases are files this test writes itself (tests/kmerdb_files.py with the full magic) and every expectation is
numpy's: np.union1d of the two key sets, the counters summed in 64 bits and clipped to 255, np.bincount for the histogram.
The union is rank-based - an entry's place is its own index plus its lower bound in the other database less the shared keys
before it, flagged per tile of 1024 entries of A - so the shapes aim at the tile edges of either input (every size around
TILE in both orders, partners equal to A, every second entry of A, packed into one gap of A), at the merged positions around
a tile edge, at empty inputs, at ranks with the top bit set (k = 32) and at the counter pairs that saturate."""
import ctypes as C

import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
from test_gpu_kmerdb_table import EDGE, TILE, _distinct_ranks, _room, _write_db

pytestmark = pytest.mark.gpu

FULL = b"TBKKMFB1"
FULL_HPC = b"TBKKMFH1"
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
KS = (2, 16, 17, 21, 31, 32)
DENSE = 2500  # ranks packed into one gap of A: more than two tiles' worth
# (ca, cb) -> the united counter; 0: the other database does not hold the key
PAIRS = {(1, 1): 2, (1, 254): 255, (254, 2): 255, (200, 100): 255, (255, 255): 255, (255, 1): 255, (1, 0): 1, (0, 255): 255}


def _full_hist(counts):
    hist = np.bincount(np.asarray(counts, dtype=np.uint8), minlength=256).astype(np.uint64)
    assert hist[0] == 0
    hist[0] = len(counts)
    return hist


def _write_full(path, k, keys, counts, reads=1, bases=21, magic=FULL):
    with open(path, "wb") as fh:
        fh.write(kf.file_bytes(k, keys, counts, _full_hist(counts), reads=reads, bases=bases, magic=magic))
    return str(path)


def _counters(rng, n):
    """1..255: a third of them 1, a sixth 254 or 255, so that sums land on every side of 255"""
    u = rng.random(n)
    return np.where(u < 0.34, 1, np.where(u < 0.5, rng.integers(254, 256, n), rng.integers(2, 254, n))).astype(np.uint8)


def _expected(a, ca, b, cb):
    keys = np.union1d(a, b)
    total = np.zeros(keys.size, dtype=np.int64)
    total[np.searchsorted(keys, a)] += ca.astype(np.int64)
    total[np.searchsorted(keys, b)] += cb.astype(np.int64)
    counts = np.minimum(total, 255).astype(np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[0] = keys.size
    return keys, counts, hist


def _plant(a, ca, b, cb):
    """the counter pairs of PAIRS on the first shared and own keys there are; returns the pairs planted"""
    shared = np.intersect1d(a, b)
    own_a, own_b = np.setdiff1d(a, b), np.setdiff1d(b, a)
    planted = set()
    both = [p for p in PAIRS if 0 not in p]
    for key, (x, y) in zip(shared, both):
        ca[np.searchsorted(a, key)], cb[np.searchsorted(b, key)] = x, y
        planted.add((x, y))
    if own_a.size:
        ca[np.searchsorted(a, own_a[0])] = 1
        planted.add((1, 0))
    if own_b.size:
        cb[np.searchsorted(b, own_b[-1])] = 255
        planted.add((0, 255))
    return planted


def _check_union(da, db, a, ca, b, cb, what, tmp_path=None):
    keys, counts, hist = _expected(a, ca, b, cb)
    with da.union(db) as du:
        assert (du.k, du.device, du.floor, du.compressed, len(du)) == (da.k, da.device, 1, da.compressed, keys.size), what
        got_keys, got_counts = du.entries()
        assert np.array_equal(got_keys, keys), (what, int(np.argmax(got_keys != keys)) if got_keys.size == keys.size else got_keys.size)
        assert np.array_equal(got_counts, counts), (what, int(np.argmax(got_counts != counts)))
        assert np.array_equal(du.histogram(), hist), what
        sa, sb, su = da.stats(), db.stats(), du.stats()
        assert (su["reads_added"], su["bases_added"], su["bytes"]) == (sa["reads_added"] + sb["reads_added"], sa["bases_added"] + sb["bases_added"], 9 * keys.size), what
        if tmp_path is not None:  # the round trip: saved, loaded (which checks order, counters and tally on the device) and compared
            from trio_binning_amd import kmers

            path = str(tmp_path / "union.tbkdb")
            du.save(path)
            assert open(path, "rb").read() == kf.file_bytes(da.k, keys, counts, hist, reads=su["reads_added"], bases=su["bases_added"],
                                                            magic=FULL_HPC if da.compressed else FULL), what
            assert kmers.database_file_info(path)["floor"] == 1
            with kmers.KmerDatabase.load(path) as back:
                assert back.floor == 1 and np.array_equal(back.entries()[0], keys) and np.array_equal(back.entries()[1], counts)
                assert np.array_equal(back.histogram(), hist) and back.stats() == su
    # both inputs are as they were
    assert np.array_equal(da.entries()[0], a) and np.array_equal(da.entries()[1], ca) and np.array_equal(db.entries()[0], b) and np.array_equal(db.entries()[1], cb), what


def _between(a, i, m, top):
    """up to m consecutive ranks above a[i] and below a[i + 1]"""
    room = (int(a[i + 1]) if i + 1 < a.size else top + 1) - int(a[i]) - 1
    return np.uint64(int(a[i]) + 1) + np.arange(max(0, min(m, room)), dtype=np.uint64)


def _partners(k, a, pool, sizes):
    """B by kind of overlap with A; `pool`: ascending ranks A lacks - 4 * TILE below A, one between every two of A's, 4 * TILE
    above; `sizes`: an iterator the kinds that have a size to choose draw it from"""
    top = (1 << (2 * k)) - 1
    n = a.size
    out = {"equal": a, "every_second": a[::2]}
    if n:
        below, above, inside = pool[pool < a[0]], pool[pool > a[-1]], pool[(pool > a[0]) & (pool < a[-1])]
        out["all_of_b_below_a"] = below[below.size - next(sizes):]
        out["all_of_b_above_a"] = above[:next(sizes)]
        out["alternating"] = np.concatenate([below[-1:], inside, above[:1]])[:next(sizes)]  # strictly: b a b a ... for as long as B lasts
    else:
        out["a_is_empty"] = pool[:next(sizes)]
    if n >= 2:
        out["first_and_last_shared"] = np.unique(np.concatenate([a[[0, -1]], inside[:max(0, next(sizes) - 2)]]))
        first = min(n, TILE)
        inner = np.arange(first // 4, max(3 * first // 4, first // 4 + 1))
        gaps = a[np.minimum(inner + 1, n - 1)] - a[inner]
        mid = int(inner[int(np.argmax(gaps))])
        out["dense_between_mid_tile"] = _between(a, mid, DENSE, top)
        if n > TILE:
            out["dense_between_across_a_tile_edge"] = _between(a, TILE - 1, DENSE, top)
    return out


def _deal(rng, k, n_a):
    """A of n_a ranks and the pool of ranks A lacks, from one ascending draw: 4 * TILE of the pool's below A, then A and the
    pool alternately, then 4 * TILE of the pool's above"""
    ranks = _distinct_ranks(rng, k, 2 * n_a + 8 * TILE)
    a = ranks[4 * TILE:4 * TILE + 2 * n_a:2]
    pool = np.setdiff1d(ranks, a)
    assert a.size == n_a and pool.size == n_a + 8 * TILE and (n_a < 2 or (a[1:] > a[:-1]).all())
    return a, pool


@pytest.mark.parametrize("k", [k for k in KS if k != 2])
def test_crafted_unions_at_every_size_and_overlap(gpu, tmp_path, k):
    import itertools

    from trio_binning_amd import kmers

    rng = np.random.default_rng(31 * k)
    sizes = itertools.cycle(SIZES[::-1] + SIZES[::2])  # (14 values against 9 sizes of A and 4 draws a turn: every size meets several of A's)
    seen, kinds, met, ran = set(), set(), set(), 0
    for i, n_a in enumerate(SIZES):
        a, pool = _deal(rng, k, n_a)
        if k == 32 and n_a >= 63:
            assert int(a[-1]) >> 63 == 1 and int(pool[0]) >> 63 == 0  # ranks on both sides of 2^63
        ca = _counters(rng, n_a)
        for j, (kind, b) in enumerate(sorted(_partners(k, a, pool, sizes).items())):
            assert b.size < 2 or (b[1:] > b[:-1]).all()
            if kind == "alternating" and b.size > 2 and n_a > b.size:
                assert (a[:b.size - 1] > b[:-1]).all() and (a[:b.size - 1] < b[1:]).all()
            cb, ca_k = _counters(rng, b.size), ca.copy()
            seen |= _plant(a, ca_k, b, cb)
            pa, pb = _write_full(tmp_path / "a.tbkdb", k, a, ca_k, reads=3, bases=300), _write_full(tmp_path / "b.tbkdb", k, b, cb, reads=5, bases=700)
            with kmers.KmerDatabase.load(pa) as da, kmers.KmerDatabase.load(pb) as db:
                assert da.floor == 1 and db.floor == 1
                _check_union(da, db, a, ca_k, b, cb, (k, n_a, kind, "a+b"), tmp_path if (i + j) % 7 == 0 else None)
                _check_union(db, da, b, cb, a, ca_k, (k, n_a, kind, "b+a"))  # the other order: the sizes swap roles
            kinds.add(kind)
            met.add(b.size)
            ran += 2
    assert seen == set(PAIRS), sorted(set(PAIRS) - seen)
    assert met >= set(SIZES), sorted(set(SIZES) - met)
    assert kinds >= {"equal", "every_second", "all_of_b_below_a", "all_of_b_above_a", "a_is_empty", "alternating", "first_and_last_shared",
                     "dense_between_mid_tile", "dense_between_across_a_tile_edge"} and ran >= 100


def test_every_size_pair_meets(gpu, tmp_path):
    """(n_a, n_b) over the whole grid of SIZES, alternating keys with every fifth of B's shared: k = 21"""
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(77)
    ranks = _distinct_ranks(rng, k, 2 * max(SIZES))
    made = {}
    for n in SIZES:
        for side in (0, 1):
            keys = ranks[side:2 * n:2].copy()  # A the even places of one draw, B the odd ones ...
            if side:
                keys[::5] = ranks[0:2 * n:2][::5]  # ... but for every fifth entry, which is its neighbour in A (where A reaches that far)
            assert keys.size == n and (n < 2 or (keys[1:] > keys[:-1]).all())
            counts = _counters(rng, keys.size)
            made[n, side] = (keys, counts, _write_full(tmp_path / "s{}_{}.tbkdb".format(n, side), k, keys, counts))
    for n_a in SIZES:
        a, ca, pa = made[n_a, 0]
        with kmers.KmerDatabase.load(pa) as da:
            for n_b in SIZES:
                b, cb, pb = made[n_b, 1]
                with kmers.KmerDatabase.load(pb) as db:
                    _check_union(da, db, a, ca, b, cb, (n_a, n_b))


def _merged(a, b):
    """the merge with both copies kept, A before B on ties: (keys, from_b)"""
    cat = np.concatenate([a, b])
    order = np.argsort(cat, kind="stable")
    return cat[order], order >= a.size


@pytest.mark.parametrize("later", [0, 1])
@pytest.mark.parametrize("d", [TILE - 1, TILE, TILE + 1, 2 * TILE])
def test_the_two_copies_of_a_key_on_either_side_of_a_merged_position(gpu, tmp_path, d, later):
    """merged positions d - 1 and d are A's and B's copy of one key (later = 0), or two different keys with the pair one
    position later (later = 1); below them A and B alternate without sharing anything, above them both go on"""
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(d + later)
    ranks = _distinct_ranks(rng, k, d + 3 * TILE)
    low = ranks[:d - 1 + later]          # d - 1 (+ 1) own keys below the pair
    shared = ranks[d - 1 + later]
    rest = ranks[d + later:]
    a = np.concatenate([low[0::2], [shared], rest[0::3]])
    b = np.unique(np.concatenate([low[1::2], [shared], rest[1::3], rest[2::300]]))
    keys, from_b = _merged(a, b)
    p = d - 1 + later
    assert keys[p] == keys[p + 1] == shared and not from_b[p] and from_b[p + 1] and (keys[:p][1:] > keys[:p][:-1]).all()
    if later:
        assert keys[d - 1] != keys[d] and keys[d] == keys[d + 1]
    else:
        assert keys[d - 1] == keys[d]
    ca, cb = _counters(rng, a.size), _counters(rng, b.size)
    ca[np.searchsorted(a, shared)], cb[np.searchsorted(b, shared)] = 200, 100
    with kmers.KmerDatabase.load(_write_full(tmp_path / "a.tbkdb", k, a, ca)) as da, kmers.KmerDatabase.load(_write_full(tmp_path / "b.tbkdb", k, b, cb)) as db:
        _check_union(da, db, a, ca, b, cb, (d, later, "a+b"))
        _check_union(db, da, b, cb, a, ca, (d, later, "b+a"))


@pytest.mark.parametrize("top_in", ["a", "b", "both"])
def test_k32_ranks_with_the_top_bit_and_the_last_rank(gpu, tmp_path, top_in):
    from trio_binning_amd import kmers

    k, last = 32, np.uint64((1 << 64) - 1)
    rng = np.random.default_rng(32)
    ranks = _distinct_ranks(rng, k, 4 * TILE + 10)
    ranks = ranks[ranks < last]
    high = ranks[ranks >= np.uint64(1 << 63)]
    assert high.size > TILE and (ranks < np.uint64(1 << 63)).sum() > TILE
    a = np.unique(np.concatenate([ranks[0::2], [np.uint64(1 << 63)], high[1::3]]))
    b = np.unique(np.concatenate([ranks[1::2], [np.uint64(1 << 63)], [np.uint64((1 << 63) - 1)]]))
    if top_in in ("a", "both"):
        a = np.append(a, last)
    if top_in in ("b", "both"):
        b = np.append(b, last)
    assert np.intersect1d(a, b).size > TILE // 4 and int(np.intersect1d(a, b)[-1]) >> 63 == 1
    ca, cb = _counters(rng, a.size), _counters(rng, b.size)
    with kmers.KmerDatabase.load(_write_full(tmp_path / "a.tbkdb", k, a, ca)) as da, kmers.KmerDatabase.load(_write_full(tmp_path / "b.tbkdb", k, b, cb)) as db:
        _check_union(da, db, a, ca, b, cb, (top_in, "a+b"), tmp_path)
        _check_union(db, da, b, cb, a, ca, (top_in, "b+a"))
        with da.union(db) as du:
            assert int(du.entries()[0][-1]) == (1 << 64) - 1


def test_k2_all_16_ranks_in_both_and_the_small_sizes(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 2
    rng = np.random.default_rng(2)
    every = np.arange(16, dtype=np.uint64)
    sets = [every, every, every[:0], every[5:6], every[::2], every[1::2], every[[0, 15]], every[3:9]]
    for i, a in enumerate(sets):
        for j, b in enumerate(sets):
            ca, cb = _counters(rng, a.size), _counters(rng, b.size)
            if a.size == 16 and b.size == 16:
                for at, (x, y) in enumerate(p for p in PAIRS if 0 not in p):
                    ca[at], cb[at] = x, y
            pa, pb = _write_full(tmp_path / "a.tbkdb", k, a, ca), _write_full(tmp_path / "b.tbkdb", k, b, cb)
            with kmers.KmerDatabase.load(pa) as da, kmers.KmerDatabase.load(pb) as db:
                _check_union(da, db, a, ca, b, cb, (i, j), tmp_path if i == 0 else None)


def test_the_counter_pairs(gpu, tmp_path):
    """every pair of PAIRS in one union, on keys that sit on both sides of A's first tile edge"""
    from trio_binning_amd import kmers

    k = 17
    rng = np.random.default_rng(9)
    a = _distinct_ranks(rng, k, TILE + 40)
    both = [p for p in PAIRS if 0 not in p]
    at = np.array([TILE - 3, TILE - 2, TILE - 1, TILE, TILE + 1, TILE + 2])
    assert len(both) == at.size
    ca = np.full(a.size, 1, dtype=np.uint8)  # (1, 0) for every own key of A
    b = np.concatenate([a[at], [np.uint64(1), np.uint64((1 << 34) - 1)]])
    b.sort()
    cb = np.full(b.size, 255, dtype=np.uint8)  # (0, 255) for the two own keys of B
    for i, (x, y) in zip(at, both):
        ca[i], cb[np.searchsorted(b, a[i])] = x, y
    keys, counts, hist = _expected(a, ca, b, cb)
    for i, (x, y) in zip(at, both):
        assert counts[np.searchsorted(keys, a[i])] == PAIRS[x, y]
    assert counts[0] == 255 and counts[-1] == 255 and (counts[1:TILE - 3] == 1).all()
    with kmers.KmerDatabase.load(_write_full(tmp_path / "a.tbkdb", k, a, ca)) as da, kmers.KmerDatabase.load(_write_full(tmp_path / "b.tbkdb", k, b, cb)) as db:
        _check_union(da, db, a, ca, b, cb, "a+b", tmp_path)
        _check_union(db, da, b, cb, a, ca, "b+a")


def test_compressed_databases_unite_among_themselves(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(4)
    ranks = _distinct_ranks(rng, k, 3000)
    a, b = ranks[::2], ranks[::3]
    ca, cb = _counters(rng, a.size), _counters(rng, b.size)
    pa, pb = _write_full(tmp_path / "a.tbkdb", k, a, ca, magic=FULL_HPC), _write_full(tmp_path / "b.tbkdb", k, b, cb, magic=FULL_HPC)
    with kmers.KmerDatabase.load(pa) as da, kmers.KmerDatabase.load(pb) as db:
        assert da.compressed and da.floor == 1
        _check_union(da, db, a, ca, b, cb, "compressed", tmp_path)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def zoo(gpu, tmp_path):
    """full and floor-2 databases of several k and both spaces, loaded: {name: (database, keys, counts)}"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(6)
    out = {}
    for name, k, magic in (("full21", 21, FULL), ("other21", 21, FULL), ("full16", 16, FULL), ("fullh21", 21, FULL_HPC)):
        keys, counts = _distinct_ranks(rng, k, 1500), _counters(rng, 1500)
        out[name] = (kmers.KmerDatabase.load(_write_full(tmp_path / (name + ".tbkdb"), k, keys, counts, magic=magic)), keys, counts)
    for name in ("solid21", "solid21b", "solid21c"):
        keys, counts = _distinct_ranks(rng, 21, 1200), np.maximum(_counters(rng, 1200), 2)
        out[name] = (kmers.KmerDatabase.load(_write_db(tmp_path / (name + ".tbkdb"), 21, keys, counts)), keys, counts)
    yield out
    for db, _, _ in out.values():
        db.close()


def _unchanged(zoo):
    for name, (db, keys, counts) in zoo.items():
        got = db.entries()
        assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts), name


def test_union_refusals_leave_no_database(gpu, zoo):
    lib = gpu.lib
    h = lambda name: zoo[name][0]._h
    for x, y, words in (("solid21", "full21", ["first", "without the once-seen k-mers", "cannot be united exactly"]),
                        ("full21", "solid21", ["second", "without the once-seen k-mers", "cannot be united exactly"]),
                        ("solid21", "solid21b", ["without the once-seen k-mers"]),
                        ("full21", "full16", ["different k", "21", "16"]),
                        ("full16", "full21", ["different k"]),
                        ("full21", "fullh21", ["homopolymer-compressed", "plain"]),
                        ("fullh21", "full21", ["homopolymer-compressed", "plain"])):
        out = C.c_void_p(1)
        rc = lib.tbk_kmerdb_union(h(x), h(y), C.byref(out))
        msg = gpu.last_error()
        assert rc == gpu.TBK_ERR_INVALID and not out.value and all(w in msg for w in words), (x, y, rc, msg)
    for x, y in ((None, h("full21")), (h("full21"), None), (None, None)):
        out = C.c_void_p(1)
        assert lib.tbk_kmerdb_union(x, y, C.byref(out)) == gpu.TBK_ERR_INVALID and not out.value
    assert lib.tbk_kmerdb_union(h("full21"), h("other21"), None) == gpu.TBK_ERR_INVALID
    with pytest.raises(ValueError, match="cannot be united exactly"):
        zoo["full21"][0].union(zoo["solid21"][0])
    _unchanged(zoo)
    # and the device goes on: the next union answers
    (da, a, ca), (db, b, cb) = zoo["full21"], zoo["other21"]
    _check_union(da, db, a, ca, b, cb, "after the refusals")


def test_solid_refusals(gpu, zoo):
    lib = gpu.lib
    out = C.c_void_p(1)
    rc = lib.tbk_kmerdb_solid(zoo["solid21"][0]._h, C.byref(out))
    assert rc == gpu.TBK_ERR_INVALID and not out.value and "not a full one" in gpu.last_error()
    out = C.c_void_p(1)
    assert lib.tbk_kmerdb_solid(None, C.byref(out)) == gpu.TBK_ERR_INVALID and not out.value
    assert lib.tbk_kmerdb_solid(zoo["full21"][0]._h, None) == gpu.TBK_ERR_INVALID
    _unchanged(zoo)


@pytest.mark.parametrize("place", [0, 1, 2])
def test_the_subtractions_and_list_builders_refuse_a_full_database_in_every_position(gpu, zoo, tmp_path, place):
    lib = gpu.lib
    names = ["solid21", "solid21b", "solid21c"]
    names[place] = "full21"
    a, b, c = (zoo[n][0]._h for n in names)
    path = str(tmp_path / "dump.txt").encode()
    n, out = C.c_uint64(7), C.c_void_p(1)
    calls = [("tbk_kmerdb_inherited", lambda: lib.tbk_kmerdb_inherited(a, b, c, 2, 255, 2, 255, path, C.byref(n))),
             ("tbk_kmerdb_inherited_table", lambda: lib.tbk_kmerdb_inherited_table(a, b, c, 2, 255, 2, 255, C.byref(out)))]
    if place < 2:
        calls += [("tbk_kmerdb_unique", lambda: lib.tbk_kmerdb_unique(a, b, 2, 255, path, C.byref(n))),
                  ("tbk_kmerdb_unique_table", lambda: lib.tbk_kmerdb_unique_table(a, b, 2, 255, C.byref(out)))]
    for name, call in calls:
        out.value = 1
        rc = call()
        msg = gpu.last_error()
        assert rc == gpu.TBK_ERR_INVALID and "tbk_kmerdb_solid" in msg and "full" in msg, (name, place, rc, msg)
        if name.endswith("_table"):
            assert not out.value, name
    assert not (tmp_path / "dump.txt").exists()
    _unchanged(zoo)
    # the solid form of that database is taken, in the same position
    with zoo["full21"][0].solid() as solid:
        dbs = [zoo[n][0] for n in ("solid21", "solid21b", "solid21c")]
        dbs[place] = solid
        assert dbs[0].unique(dbs[1], 2, 255, str(tmp_path / "ok.txt"), child=dbs[2]) >= 0


# ---- tbk_kmerdb_solid ---------------------------------------------------------------------------------------------------------
def _check_solid(tmp_path, k, keys, counts, what, magic=FULL):
    from trio_binning_amd import kmers

    hist = _full_hist(counts)
    keep = counts >= 2
    with kmers.KmerDatabase.load(_write_full(tmp_path / "full.tbkdb", k, keys, counts, reads=9, bases=900, magic=magic)) as full:
        with full.solid() as solid:
            assert (solid.k, solid.floor, solid.compressed, len(solid), solid.device) == (k, 2, magic == FULL_HPC, int(keep.sum()), full.device), what
            got = solid.entries()
            assert np.array_equal(got[0], keys[keep]) and np.array_equal(got[1], counts[keep]), what
            assert np.array_equal(solid.histogram(), hist) and int(solid.histogram()[1]) == int((counts == 1).sum()), what  # rows carried over
            assert solid.stats() == {"reads_added": 9, "bases_added": 900, "bytes": 9 * int(keep.sum())}
            path = str(tmp_path / "solid.tbkdb")
            solid.save(path)
            # byte for byte the floor-2 file of those entries and that histogram, under the old magic
            assert open(path, "rb").read() == kf.file_bytes(k, keys[keep], counts[keep], hist, reads=9, bases=900,
                                                            magic=b"TBKKMDH1" if magic == FULL_HPC else kf.MAGIC), what
            with kmers.KmerDatabase.load(path) as back:
                assert back.floor == 2 and len(back) == int(keep.sum())
        assert np.array_equal(full.entries()[0], keys) and np.array_equal(full.entries()[1], counts)


@pytest.mark.parametrize("k", KS)
def test_solid_of_crafted_databases(gpu, tmp_path, k):
    rng = np.random.default_rng(500 + k)
    for n in SIZES:
        if n > _room(k):
            continue
        keys, counts = _distinct_ranks(rng, k, n) if n else np.zeros(0, dtype=np.uint64), _counters(rng, n)
        _check_solid(tmp_path, k, keys, counts, (k, n, "mixed"))
        if n:
            _check_solid(tmp_path, k, keys, np.ones(n, dtype=np.uint8), (k, n, "all counters 1"))  # an empty, valid database
            _check_solid(tmp_path, k, keys, np.maximum(counts, 2), (k, n, "no counter 1"))
            edge = np.where(np.arange(n) % TILE < TILE // 2, 1, 7).astype(np.uint8)  # half of every tile
            _check_solid(tmp_path, k, keys, edge, (k, n, "half tiles"))
    if k == 21:
        keys, counts = _distinct_ranks(rng, k, 2000), _counters(rng, 2000)
        _check_solid(tmp_path, k, keys, counts, "compressed", magic=FULL_HPC)


def test_loading_refuses_a_full_file_whose_content_disagrees(gpu, tmp_path):
    """the device check with floor 1: a counter 0, and a tally of row 1 that is not the header's"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(8)
    keys, counts = _distinct_ranks(rng, 21, 3000), _counters(rng, 3000)
    good = _write_full(tmp_path / "good.tbkdb", 21, keys, counts)
    zero = counts.copy()
    zero[1234] = 0
    hist = _full_hist(counts)
    (tmp_path / "zero.tbkdb").write_bytes(kf.file_bytes(21, keys, zero, hist, magic=FULL))
    with pytest.raises(ValueError, match="below 1"):
        kmers.KmerDatabase.load(str(tmp_path / "zero.tbkdb"))
    swapped = counts.copy()
    i, j = int(np.argmax(counts == 1)), int(np.argmax(counts == 7))
    assert counts[i] == 1 and counts[j] == 7
    swapped[i] = 7  # one counter 1 fewer, one 7 more: the rows still sum to n
    (tmp_path / "tally.tbkdb").write_bytes(kf.file_bytes(21, keys, swapped, hist, magic=FULL))
    with pytest.raises(ValueError, match="counters are 1, the header's histogram states"):
        kmers.KmerDatabase.load(str(tmp_path / "tally.tbkdb"))
    with kmers.KmerDatabase.load(good) as db:
        assert db.floor == 1 and len(db) == 3000


# ---- the query session on a full database ----------------------------------------------------------------------------------------
def test_query_on_a_full_database_counts_presence(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(12)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 3000))
    held = sorted({km for km in ref.window_kmers(genome[:2400], k)})  # the database holds the first 2400 bases' k-mers
    cs = rng.integers(1, 256, len(held))
    cs[rng.random(len(held)) < 0.5] = 1
    db = dict(zip(held, (int(c) for c in cs)))
    assert sum(1 for c in db.values() if c == 1) > 500 and sum(1 for c in db.values() if c >= 2) > 500
    ranks = np.array(sorted(ref.lex_rank(km) for km in db), dtype=np.uint64)
    by_rank = {ref.lex_rank(km): c for km, c in db.items()}
    counts = np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8)
    seqs = [genome[100:1500], genome[2000:3000].lower(), genome[:300] + "N" + genome[300:700], "ACGT"]
    bases, offsets = kmers.pack_reads(seqs)
    want_counts = np.zeros(bases.size, dtype=np.uint8)
    want = {1: np.zeros((len(seqs), 2), dtype=np.uint64), 2: np.zeros((len(seqs), 2), dtype=np.uint64)}
    at = 0
    for r, s in enumerate(seqs):
        for w, km in enumerate(ref.window_kmers(s, k)):
            if km is not None:
                c = db.get(km, 0)
                want_counts[at + w] = c
                for lo in (1, 2):
                    want[lo][r, 0] += 1
                    want[lo][r, 1] += c >= lo
        at += len(s)
    assert (want_counts == 1).sum() > 300 and want[1][:, 1].sum() > want[2][:, 1].sum() > 0 and (want[1][:, 1] < want[1][:, 0]).any()
    with kmers.KmerDatabase.load(_write_full(tmp_path / "full.tbkdb", k, ranks, counts)) as full, full.solid() as solid:
        with full.query() as q:
            per_read, got_counts = q.add(bases, offsets, 1, return_counts=True)
            assert np.array_equal(per_read, want[1])            # presence: the c = 1 entries are found
            assert np.array_equal(got_counts, want_counts) and (got_counts == 1).any()  # and the per-base counts carry c = 1
            hist = q.histogram()
            assert int(hist[1]) == int((want_counts == 1).sum())
            seen1, solid1 = q.completeness(1, 255)
            assert solid1 == len(db) and 0 < seen1 <= solid1
            assert q.completeness(0, 255) == (seen1, solid1)    # clamped to the floor
            seen2, solid2 = q.completeness(2, 255)
            assert solid2 == int((counts >= 2).sum()) and seen2 < seen1
            q.reset()
            assert np.array_equal(q.add(bases, offsets, 2), want[2])
            with solid.query() as qs:  # min_count = 2 answers as the solid database does, and the solid one clamps 1 to 2
                assert np.array_equal(qs.add(bases, offsets, 2), want[2])
                assert qs.completeness(2, 255) == (seen2, solid2)
                qs.reset()
                assert np.array_equal(qs.add(bases, offsets, 1), want[2]) and qs.completeness(1, 255) == (seen2, solid2)
                solid_counts = qs.add(bases, offsets, 2, return_counts=True)[1]
                assert np.array_equal(solid_counts, np.where(want_counts >= 2, want_counts, 0))
