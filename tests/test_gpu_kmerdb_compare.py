"""Count databases held against each other on the device (include/tbk.h): tbk_kmerdb_joint_spectrum and
tbk_kmerdb_origin_spectrum, kmers.KmerDatabase.joint_spectrum / origin_spectrum and the compare_databases command on top.

Crafted databases are files this test writes itself (tests/kmerdb_files.py through the helpers of the table and union tests)
and every expectation is numpy's (tests/db_compare_ref.py): integer counts, compared exactly.  Both kernels stride over tiles
of 1024 entries of the database they walk, bisect between the tile's bounds in the partner and tally in LDS - the joint one
only a low-counter corner of the matrix, whose side is a power of two up to 128 - so the shapes aim at the tile edges of
either side (every size around a wave, a block round and a tile, in both orders), at partners that fall into one gap, at
empty sides, at ranks with the top bit set (k = 32), at counters on both sides of every possible corner edge, at one cell
heavier than 16 bits, and at the later trips of the strided loops (tbk_count_set_grid_caps_)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import db_compare_ref as ref
from test_gpu_kmerdb_table import TILE, _distinct_ranks, _write_db
from test_gpu_kmerdb_union import _write_full

pytestmark = pytest.mark.gpu

FULL_HPC = b"TBKKMFH1"
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
KS = (2, 16, 21, 31, 32)
FLOORS = ((2, 2), (1, 1), (1, 2))
VALUES = (1, 2, 63, 64, 65, 127, 128, 254, 255)  # on both sides of the edge of a corner of 64, 128 (and 2, 256)
DENSE = 2500  # ranks packed into one gap: more than two tiles' worth
RANGES = (((1, 255), (1, 255)), ((2, 255), (2, 255)), ((65, 255), (1, 63)), ((64, 64), (128, 128)), ((1, 1), (255, 255)))
EMPTY = np.zeros(0, dtype=np.uint64)


def _counters(rng, n, floor):
    """floor..255: most of them low, where a spectrum lives, the rest anywhere"""
    return np.where(rng.random(n) < 0.6, rng.integers(floor, 40, n), rng.integers(floor, 256, n)).astype(np.uint8)


def _write(path, k, keys, counts, floor, **kw):
    return _write_full(path, k, keys, counts, **kw) if floor == 1 else _write_db(path, k, keys, counts)


def _plant(x, cx, y, cy, floor_x, floor_y):
    """every pair of VALUES the floors allow on shared keys spread over all of them, every value on keys one side alone holds;
    returns the pairs planted (0: the other side does not hold the key)"""
    vx, vy = [v for v in VALUES if v >= floor_x], [v for v in VALUES if v >= floor_y]
    shared, own_x, own_y = np.intersect1d(x, y), np.setdiff1d(x, y), np.setdiff1d(y, x)
    pairs = [(a, b) for a in vx for b in vy]
    planted = set()
    for key, (a, b) in zip(shared[::max(1, shared.size // len(pairs))], pairs):
        cx[np.searchsorted(x, key)], cy[np.searchsorted(y, key)] = a, b
        planted.add((a, b))
    for key, a in zip(own_x[::max(1, own_x.size // len(vx))], vx):
        cx[np.searchsorted(x, key)] = a
        planted.add((a, 0))
    for key, b in zip(own_y[::max(1, own_y.size // len(vy))], vy):
        cy[np.searchsorted(y, key)] = b
        planted.add((0, b))
    return planted


def _widest_gap(x):
    """the place in x's first tile whose successor lies farthest above it"""
    first = min(x.size, TILE) - 1
    return int(np.argmax(x[1:first + 1] - x[:first]))


def _cases(rng, k, sizes=SIZES):
    """(name, x, y): y by kind of overlap with x, x at every size.  Every pair is compared in both orders, so each kind also
    runs with the sides exchanged and y's sizes are x's too."""
    if k == 2:  # 16 ranks in all
        every = np.arange(16, dtype=np.uint64)
        sets = [every, EMPTY, every[5:6], every[::2], every[1::2], every[[0, 15]], every[3:9]]
        for (i, x), (j, y) in itertools.product(enumerate(sets), enumerate(sets)):
            yield ("k2", i, j), x, y
        return
    other = itertools.cycle(SIZES[::-1])
    for n in sizes:
        ranks = _distinct_ranks(rng, k, n + 2 * max(SIZES))
        x = ranks[np.sort(rng.choice(ranks.size, size=n, replace=False))]
        pool = np.setdiff1d(ranks, x)  # below, between and above x's
        assert x.size == n and pool.size == 2 * max(SIZES)
        if k == 32 and n >= 63:
            assert int(x[-1]) >> 63 == 1 and int(x[0]) >> 63 == 0  # ranks on both sides of 2^63
        yield ("equal", n), x, x
        yield ("every_second", n), x, x[::2]
        yield ("disjoint", n), x, np.sort(rng.choice(pool, size=next(other), replace=False))
        yield ("mixed", n), x, np.union1d(x[1::3], pool[:next(other):2])
        yield ("y_empty", n), x, EMPTY
        if n >= 2:
            i = _widest_gap(x)
            dense = x[i] + np.uint64(1) + np.arange(min(DENSE, int(x[i + 1] - x[i]) - 1), dtype=np.uint64)
            assert dense.size == DENSE and x[i] < dense[0] and dense[-1] < x[i + 1]
            yield ("dense_in_one_gap", n), x, dense
    yield ("both_empty", 0), EMPTY, EMPTY


def _joint_both_ways(dx, dy, x, cx, y, cy, what):
    """the device's spectrum in both orders: its own invariants first, then the reference cell by cell"""
    want = ref.joint_spectrum(x, cx, y, cy)
    union = np.union1d(x, y).size
    for got, expect, rows, cols in ((dx.joint_spectrum(dy), want, cx, cy), (dy.joint_spectrum(dx), want.T, cy, cx)):
        ref.check_joint_invariants(got, rows, cols, union)
        assert np.array_equal(got, expect), (what, [(int(i), int(j), int(got[i, j]), int(expect[i, j])) for i, j in zip(*np.nonzero(got != expect))][:8])


def _load_pair(kmers, tmp_path, k, x, cx, y, cy, floors, **kw):
    return (kmers.KmerDatabase.load(_write(tmp_path / "x.tbkdb", k, x, cx, floors[0], **kw)),
            kmers.KmerDatabase.load(_write(tmp_path / "y.tbkdb", k, y, cy, floors[1], **kw)))


# ---- 1 and 3: the joint spectrum against the reference, and its invariants on the device's own output -------------------------
@pytest.mark.parametrize("k", KS)
def test_joint_spectrum_at_every_size_overlap_and_floor(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(100 + k)
    seen, kinds, met = {f: set() for f in FLOORS}, set(), set()
    for floors in FLOORS:
        for name, x, y in _cases(rng, k):
            cx, cy = _counters(rng, x.size, floors[0]), _counters(rng, y.size, floors[1])
            seen[floors] |= _plant(x, cx, y, cy, *floors)
            dx, dy = _load_pair(kmers, tmp_path, k, x, cx, y, cy, floors)
            with dx, dy:
                assert (dx.floor, dy.floor) == floors
                _joint_both_ways(dx, dy, x, cx, y, cy, (k, floors, name))
            kinds.add(name[0])
            met |= {x.size, y.size}
    if k != 2:
        assert kinds == {"equal", "every_second", "disjoint", "mixed", "y_empty", "dense_in_one_gap", "both_empty"} and met >= set(SIZES) | {DENSE}
        for fx, fy in FLOORS:  # every pair and every lone value the floors allow was on some key
            vx, vy = [v for v in VALUES if v >= fx], [v for v in VALUES if v >= fy]
            assert seen[fx, fy] >= set(itertools.product(vx, vy)) | {(v, 0) for v in vx} | {(0, v) for v in vy}


def test_joint_spectrum_of_compressed_databases(gpu, tmp_path):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(5)
    ranks = _distinct_ranks(rng, 21, 3000)
    x, y = ranks[::2], ranks[::3]
    cx, cy = _counters(rng, x.size, 1), _counters(rng, y.size, 1)
    dx, dy = _load_pair(kmers, tmp_path, 21, x, cx, y, cy, (1, 1), magic=FULL_HPC)
    with dx, dy:
        assert dx.compressed and dy.compressed
        _joint_both_ways(dx, dy, x, cx, y, cy, "compressed")


# ---- 2: one cell far heavier than 16 bits, inside the LDS corner and outside it -----------------------------------------------
def test_a_heavy_cell_inside_the_corner_and_one_outside(gpu, tmp_path):
    """70 000 shared keys with (5, 7) - inside a corner of any size - and 70 000 with (200, 130), outside every one: a private
    counter narrower than 32 bits wraps, a lost global add shows.  Uncapped every block tallies 1024 entries; with the grid
    capped to one block that block's cells take all 70 000."""
    from trio_binning_amd import kmers

    n = 70_000
    rng = np.random.default_rng(70)
    keys = _distinct_ranks(rng, 21, 2 * n)
    where = rng.permutation(2 * n) < n
    cx, cy = np.where(where, 5, 200).astype(np.uint8), np.where(where, 7, 130).astype(np.uint8)
    want = np.zeros((256, 256), dtype=np.uint64)
    want[5, 7], want[200, 130] = n, n
    assert np.array_equal(ref.joint_spectrum(keys, cx, keys, cy), want)
    dx, dy = _load_pair(kmers, tmp_path, 21, keys, cx, keys, cy, (2, 2))
    with dx, dy:
        assert np.array_equal(dx.joint_spectrum(dy), want) and np.array_equal(dy.joint_spectrum(dx), want.T)
        table = np.zeros((4, 256), dtype=np.uint64)
        table[3, 5], table[1, 200] = n, n  # y holds every key; itself, as z, in [1, 100] only those with 7
        assert np.array_equal(dx.origin_spectrum(dy, dy, (1, 255), (1, 100)), table)
        try:
            gpu.lib.tbk_count_set_grid_caps_(0, 1)
            assert np.array_equal(dx.joint_spectrum(dy), want) and np.array_equal(dy.joint_spectrum(dx), want.T)
            assert np.array_equal(dx.origin_spectrum(dy, dy, (1, 255), (1, 100)), table)
        finally:
            gpu.lib.tbk_count_set_grid_caps_(0, 0)


# ---- 5: the origin spectrum against the reference ---------------------------------------------------------------------------------
def _origin_all_ranges(db, dy, dz, x, cx, y, cy, z, cz, what):
    for y_range, z_range in RANGES:
        got = db.origin_spectrum(dy, dz, y_range, z_range)
        ref.check_origin_invariants(got, cx)
        want = ref.origin_spectrum(x, cx, y, cy, y_range, z, cz, z_range)
        assert np.array_equal(got, want), (what, y_range, z_range, [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in zip(*np.nonzero(got != want))][:8])


@pytest.mark.parametrize("k", KS)
def test_origin_spectrum_at_every_size_overlap_and_range(gpu, tmp_path, k):
    """base at every size, y by every kind of overlap, z the partner of the case before (independent of y); floors of base, y
    and z in turn 2/2/2, 1/1/1 and 1/2/1"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(200 + k)
    for floors in ((2, 2, 2), (1, 1, 1), (1, 2, 1)):
        z = np.arange(4, 11, dtype=np.uint64) if k == 2 else _distinct_ranks(rng, k, 777)
        for name, x, y in _cases(rng, k):
            cx, cy, cz = (_counters(rng, keys.size, floor) for keys, floor in zip((x, y, z), floors))
            _plant(x, cx, y, cy, floors[0], floors[1])
            _plant(x, cx.copy(), z, cz, floors[0], floors[2])  # (the partner's side of the pairs; the base keeps the ones it has)
            dx, dy = _load_pair(kmers, tmp_path, k, x, cx, y, cy, floors[:2])
            with dx, dy, kmers.KmerDatabase.load(_write(tmp_path / "z.tbkdb", k, z, cz, floors[2])) as dz:
                _origin_all_ranges(dx, dy, dz, x, cx, y, cy, z, cz, (k, floors, name))
                _origin_all_ranges(dy, dz, dx, y, cy, z, cz, x, cx, (k, floors, name, "y as base"))
            z = y


def test_origin_ranges_are_taken_literally(gpu, tmp_path):
    """a full partner that holds the key with counter 1 does not count from 2 up; a range that misses the partner's counter by
    one on either side; min == max; and every range that is none"""
    from trio_binning_amd import kmers

    base, cb = np.array([10, 20, 30, 40, 50], dtype=np.uint64), np.array([2, 3, 3, 9, 255], dtype=np.uint8)
    y, cy = np.array([10, 20, 30, 45], dtype=np.uint64), np.array([1, 64, 2, 7], dtype=np.uint8)       # full
    z, cz = np.array([20, 40, 50, 60], dtype=np.uint64), np.array([65, 2, 255, 2], dtype=np.uint8)     # floor 2

    def cells(table):
        return {(int(i), int(j)): int(table[i, j]) for i, j in zip(*np.nonzero(table))}

    with kmers.KmerDatabase.load(_write_db(tmp_path / "b.tbkdb", 21, base, cb)) as db, \
            kmers.KmerDatabase.load(_write_full(tmp_path / "y.tbkdb", 21, y, cy)) as dy, kmers.KmerDatabase.load(_write_db(tmp_path / "z.tbkdb", 21, z, cz)) as dz:
        # (1, 255): y holds 10, 20, 30; z holds 20, 40, 50
        assert cells(db.origin_spectrum(dy, dz)) == {(1, 2): 1, (3, 3): 1, (1, 3): 1, (2, 9): 1, (2, 255): 1}
        # from 2 up the once-seen 10 of the full partner does not count
        assert cells(db.origin_spectrum(dy, dz, (2, 255), (2, 255))) == {(0, 2): 1, (3, 3): 1, (1, 3): 1, (2, 9): 1, (2, 255): 1}
        # y's 64 on key 20 missed by one from above and from below, z's 65 likewise
        assert cells(db.origin_spectrum(dy, dz, (65, 255), (1, 64))) == {(0, 2): 1, (0, 3): 2, (2, 9): 1, (0, 255): 1}
        assert cells(db.origin_spectrum(dy, dz, (1, 63), (66, 255))) == {(1, 2): 1, (0, 3): 1, (1, 3): 1, (0, 9): 1, (2, 255): 1}
        # min == max
        assert cells(db.origin_spectrum(dy, dz, (64, 64), (65, 65))) == {(0, 2): 1, (3, 3): 1, (0, 3): 1, (0, 9): 1, (0, 255): 1}
        assert cells(db.origin_spectrum(dy, dz, (1, 1), (255, 255))) == {(1, 2): 1, (0, 3): 2, (0, 9): 1, (2, 255): 1}
        for want in (ref.origin_spectrum(base, cb, y, cy, (65, 255), z, cz, (1, 64)),):
            assert np.array_equal(db.origin_spectrum(dy, dz, (65, 255), (1, 64)), want)
        spec = (C.c_uint64 * 1024)()
        bad = ((0, 5), (5, 4), (1, 256), (256, 256), (0, 0), (0, 255), (255, 1), (1, 0xFFFFFFFF))
        for lo, hi in bad:
            for args in ((lo, hi, dz._h, 1, 255), (1, 255, dz._h, lo, hi)):
                rc = gpu.lib.tbk_kmerdb_origin_spectrum(db._h, dy._h, args[0], args[1], args[2], args[3], args[4], spec)
                assert rc == gpu.TBK_ERR_INVALID and "1 <= min <= max <= 255" in gpu.last_error(), (lo, hi, rc, gpu.last_error())
            with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
                db.origin_spectrum(dy, dz, (lo, hi), (1, 255))
        with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
            db.origin_spectrum(dy, dz, (1, 255), (-1, 255))
        assert not any(spec)
        assert cells(db.origin_spectrum(dy, dz)) == {(1, 2): 1, (3, 3): 1, (1, 3): 1, (2, 9): 1, (2, 255): 1}


# ---- 4: the later trips of both strided loops -------------------------------------------------------------------------------------
def test_later_trips_give_the_same_spectra(gpu, tmp_path):
    """the 3 * TILE + 17 cases (4 tiles; their dense partners 3) with the grids capped to 1, 2, 3 and 5 blocks"""
    from trio_binning_amd import kmers

    k, floors = 21, (1, 2)
    rng = np.random.default_rng(44)
    made = []
    z = _distinct_ranks(rng, k, 2 * TILE + 5)
    cz = _counters(rng, z.size, 1)
    for name, x, y in _cases(rng, k, sizes=(3 * TILE + 17,)):
        cx, cy = _counters(rng, x.size, floors[0]), _counters(rng, y.size, floors[1])
        _plant(x, cx, y, cy, *floors)
        made.append((name, x, cx, y, cy))
    assert {m[0][0] for m in made} >= {"equal", "every_second", "disjoint", "mixed", "dense_in_one_gap", "y_empty"}
    for name, x, cx, y, cy in made:
        dx, dy = _load_pair(kmers, tmp_path, k, x, cx, y, cy, floors)
        with dx, dy, kmers.KmerDatabase.load(_write(tmp_path / "z.tbkdb", k, z, cz, 1)) as dz:
            try:
                for cap in (1, 2, 3, 5):
                    assert gpu.lib.tbk_count_set_grid_caps_(0, cap) == 0
                    _joint_both_ways(dx, dy, x, cx, y, cy, (cap, name))
                    _origin_all_ranges(dx, dy, dz, x, cx, y, cy, z, cz, (cap, name))
                    _origin_all_ranges(dz, dx, dy, z, cz, x, cx, y, cy, (cap, name, "z as base"))
            finally:
                gpu.lib.tbk_count_set_grid_caps_(0, 0)


# ---- 6: agreement with the selections that exist ----------------------------------------------------------------------------------
def _trio(rng, k, n, father_unrelated=False):
    """(A, B, child) as (keys, counters >= 2): the child's keys are half of A's own, half of B's own, most of what both hold and
    some of its own; with an unrelated father, B is replaced by a key set drawn apart from the family's"""
    ranks = _distinct_ranks(rng, k, 4 * n)
    kind = rng.integers(0, 4, ranks.size)  # 0: A alone, 1: B alone, 2: both, 3: neither parent
    a, b = ranks[(kind == 0) | (kind == 2)], ranks[(kind == 1) | (kind == 2)]
    take = rng.random(ranks.size)
    child = ranks[((kind < 2) & (take < 0.5)) | ((kind == 2) & (take < 0.95)) | ((kind == 3) & (take < 0.02))]
    if father_unrelated:
        b = np.union1d(ranks[(kind == 3) & (take > 0.5)], b[::50])  # what the child got from B is in neither parent now
    return [(keys, _counters(rng, keys.size, 2)) for keys in (a, b, child)]


@pytest.mark.parametrize("cuts", [((2, 255), (2, 255), 2), ((5, 30), (3, 200), 4), ((39, 39), (2, 2), 255)])
def test_trio_figures_agree_with_unique_set(gpu, tmp_path, cuts):
    from trio_binning_amd import compare_databases as cd, kmers

    range_a, range_b, child_min = cuts
    (a, ca), (b, cb), (c, cc) = _trio(np.random.default_rng(6), 21, 3 * TILE + 17)
    paths = [_write_db(tmp_path / (name + ".tbkdb"), 21, keys, counts) for name, keys, counts in (("a", a, ca), ("b", b, cb), ("c", c, cc))]
    with kmers.KmerDatabase.load(paths[0]) as da, kmers.KmerDatabase.load(paths[1]) as db, kmers.KmerDatabase.load(paths[2]) as dc:
        tables = (dc.origin_spectrum(da, db, (2, 255), (2, 255)), da.origin_spectrum(db, dc, (2, 255), (child_min, 255)),
                  db.origin_spectrum(da, dc, (2, 255), (child_min, 255)))
        figures = dict(line.split("\t") for line in cd.report_trio(*tables, 21, False, range_a, range_b, child_min))
        for hap, own, other, (lo, hi) in (("a", da, db, range_a), ("b", db, da, range_b)):
            def size(**child):
                try:
                    with own.unique_set(other, lo, hi, **child) as hs:
                        return hs.num_kmers
                except ValueError as exc:
                    assert "empty k-mer list" in str(exc)
                    return 0
            assert int(figures["unique_" + hap]) == size(), (hap, cuts)
            assert int(figures["inherited_" + hap]) == size(child=dc, child_min=child_min, child_max=255), (hap, cuts)
        if cuts[2] == 2:
            assert int(figures["unique_a"]) > TILE and 0.4 < float(figures["inherited_a_share"]) < 0.6  # (the crafted trio is one)


# ---- 7: the contract ----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def zoo(gpu, tmp_path):
    """{name: (database, keys, counts)}: full and floor-2 databases of two k and both spaces, and an empty one"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(7)
    out = {}
    for name, k, floor, magic, n in (("full21", 21, 1, None, 1500), ("solid21", 21, 2, None, 1200), ("full16", 16, 1, None, 1500),
                                     ("fullh21", 21, 1, FULL_HPC, 1500), ("empty21", 21, 2, None, 0)):
        keys, counts = _distinct_ranks(rng, k, n) if n else EMPTY, _counters(rng, n, floor)
        path = _write(tmp_path / (name + ".tbkdb"), k, keys, counts, floor, **({"magic": magic} if magic else {}))
        out[name] = (kmers.KmerDatabase.load(path), keys, counts)
    yield out
    for db, _, _ in out.values():
        db.close()


def _unchanged(zoo, hists):
    for name, (db, keys, counts) in zoo.items():
        got = db.entries()
        assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts) and np.array_equal(db.histogram(), hists[name]), name


def test_refusals_and_successes_leave_the_databases_as_they_were(gpu, zoo):
    lib = gpu.lib
    h = lambda name: None if name is None else zoo[name][0]._h
    hists = {name: db.histogram() for name, (db, _, _) in zoo.items()}
    joint, origin = (C.c_uint64 * 65536)(), (C.c_uint64 * 1024)()

    def works():
        (dx, x, cx), (dy, y, cy), (de, _, _) = zoo["full21"], zoo["solid21"], zoo["empty21"]
        _joint_both_ways(dx, dy, x, cx, y, cy, "after a refusal")
        assert np.array_equal(dx.origin_spectrum(dy, de, (2, 255)), ref.origin_spectrum(x, cx, y, cy, (2, 255), EMPTY, EMPTY, (1, 255)))
        _unchanged(zoo, hists)

    works()
    for x, y, words in (("full21", "full16", ["different k", "21", "16"]), ("full16", "solid21", ["different k"]),
                        ("full21", "fullh21", ["homopolymer-compressed", "plain"]), ("fullh21", "solid21", ["homopolymer-compressed", "plain"]),
                        (None, "full21", ["NULL"]), ("full21", None, ["NULL"]), (None, None, ["NULL"])):
        rc = lib.tbk_kmerdb_joint_spectrum(h(x), h(y), joint)
        msg = gpu.last_error()
        assert rc == gpu.TBK_ERR_INVALID and all(w in msg for w in words), (x, y, rc, msg)
        for trio in ((x, y, "full21"), (x, "full21", y), ("full21", x, y)) if (x is None or y is None) else ((x, y, x), (x, x, y), (y, x, x)):
            rc = lib.tbk_kmerdb_origin_spectrum(h(trio[0]), h(trio[1]), 1, 255, h(trio[2]), 1, 255, origin)
            msg = gpu.last_error()
            assert rc == gpu.TBK_ERR_INVALID and all(w in msg for w in words), (trio, rc, msg)
        works()
    assert lib.tbk_kmerdb_joint_spectrum(h("full21"), h("solid21"), None) == gpu.TBK_ERR_INVALID
    assert lib.tbk_kmerdb_origin_spectrum(h("full21"), h("solid21"), 1, 255, h("solid21"), 1, 255, None) == gpu.TBK_ERR_INVALID
    assert not any(joint) and not any(origin)  # a refused call writes nothing
    with pytest.raises(ValueError, match="different k"):
        zoo["full21"][0].joint_spectrum(zoo["full16"][0])
    with pytest.raises(ValueError, match="homopolymer-compressed"):
        zoo["full21"][0].origin_spectrum(zoo["solid21"][0], zoo["fullh21"][0])
    works()


# ---- 8: the command, end to end -------------------------------------------------------------------------------------------------------
def test_the_command_on_two_databases(gpu, tmp_path, capsys):
    from trio_binning_amd import compare_databases as cd

    k = 21
    rng = np.random.default_rng(8)
    ranks = _distinct_ranks(rng, k, 3 * TILE)
    x, y = ranks[rng.random(ranks.size) < 0.6], ranks[rng.random(ranks.size) < 0.5]
    cx, cy = _counters(rng, x.size, 1), _counters(rng, y.size, 2)
    _plant(x, cx, y, cy, 1, 2)
    px, py = _write_full(tmp_path / "x.tbkdb", k, x, cx), _write_db(tmp_path / "y.tbkdb", k, y, cy)
    want = ref.joint_spectrum(x, cx, y, cy)
    matrix = str(tmp_path / "joint.tsv")
    cd.main([px, py, "--matrix", matrix])
    out = capsys.readouterr().out
    assert out == "\n".join(cd.report_two(want, k, False, 1, 2)) + "\n"
    lines = dict(line.split("\t") for line in out.splitlines())
    assert (int(lines["kmers_x"]), int(lines["kmers_y"]), int(lines["shared"]), int(lines["union"])) == (x.size, y.size, np.intersect1d(x, y).size, np.union1d(x, y).size)
    assert np.array_equal(cd.read_matrix(matrix), want)
    head = [l for l in open(matrix) if l.startswith("#")]
    assert px in head[1] and "floor 1" in head[1] and py in head[2] and "floor 2" in head[2]
    # the other order, no matrix; and an empty database against itself: every ratio nan
    cd.main([py, px])
    assert capsys.readouterr().out == "\n".join(cd.report_two(want.T, k, False, 2, 1)) + "\n"
    pe = _write_db(tmp_path / "e.tbkdb", k, EMPTY, np.zeros(0, dtype=np.uint8))
    cd.main([pe, pe])
    assert capsys.readouterr().out == "\n".join(cd.report_two(np.zeros((256, 256), dtype=np.uint64), k, False, 2, 2)) + "\n"


@pytest.mark.parametrize("father_unrelated", [False, True])
def test_the_command_on_a_trio(gpu, tmp_path, capsys, father_unrelated):
    """a crafted trio, and the same with the father replaced by an unrelated key set: the exact figures of the reference on the
    solid forms of the files (A is given as a full file), no threshold"""
    from trio_binning_amd import compare_databases as cd

    k, range_a, range_b, child_min = 21, (3, 60), (2, 255), 3
    rng = np.random.default_rng(9)
    (a, ca), (b, cb), (c, cc) = _trio(rng, k, 2 * TILE + 100, father_unrelated)
    ones = _distinct_ranks(rng, k, 500)
    ones = ones[~np.isin(ones, a)]  # once-seen k-mers of A's full file, some of them B's or the child's: the solid form drops them
    full_a = np.union1d(a, ones)
    full_ca = np.ones(full_a.size, dtype=np.uint8)
    full_ca[np.searchsorted(full_a, a)] = ca
    pa, pb, pc = _write_full(tmp_path / "A.tbkdb", k, full_a, full_ca), _write_db(tmp_path / "B.tbkdb", k, b, cb), _write_db(tmp_path / "child.tbkdb", k, c, cc)
    held = (child_min, 255)
    want = (ref.origin_spectrum(c, cc, a, ca, (2, 255), b, cb, (2, 255)), ref.origin_spectrum(a, ca, b, cb, (2, 255), c, cc, held),
            ref.origin_spectrum(b, cb, a, ca, (2, 255), c, cc, held))
    spectra = str(tmp_path / "trio.tsv")
    cd.main([pa, pb, "--child-database", pc, "--spectra", spectra, "--min-count-a", "3", "--max-count-a", "60", "--min-count-b", "2",
             "--max-count-b", "255", "--min-count-child", "3"])
    out = capsys.readouterr().out
    assert out == "\n".join(cd.report_trio(*want, k, False, range_a, range_b, child_min)) + "\n"
    back = cd.read_spectra(spectra)
    assert len(back) == 3 and all(np.array_equal(got, table) for (_, got), table in zip(back, want))
    assert [title for title, _ in back] == [
        "base = child {}; first = A {} [2,255]; second = B {} [2,255]".format(pc, pa, pb),
        "base = A {}; first = B {} [2,255]; second = child {} [3,255]".format(pa, pb, pc),
        "base = B {}; first = A {} [2,255]; second = child {} [3,255]".format(pb, pa, pc)]
    # what the lines say, from the key sets alone
    lines = dict(line.split("\t") for line in out.splitlines())
    solid_child = c[cc >= child_min]
    assert int(lines["child_solid"]) == solid_child.size
    assert int(lines["child_in_neither"]) == int((~np.isin(solid_child, a) & ~np.isin(solid_child, b)).sum())
    own_a = a[(ca >= 3) & (ca <= 60) & ~np.isin(a, b)]
    assert int(lines["unique_a"]) == own_a.size and int(lines["inherited_a"]) == int(np.isin(own_a, solid_child).sum())
