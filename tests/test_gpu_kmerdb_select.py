"""A selection from count databases that stays a database, on the device (include/tbk.h: tbk_kmerdb_select;
kmers.KmerDatabase.select; the select_database and hapmers commands on top).

Crafted databases are files this test writes itself (tests/kmerdb_files.py through the helpers of the table, union and compare
tests) and every expectation is numpy's (tests/db_select_ref.py): keys, counters and histogram rows, compared exactly.  The
kernels take one block per tile of 1024 entries of the base, find the tile's bounds in up to two partners and bisect between
them, so the shapes aim at the tile edges (every size around a wave, a block round and a tile), at partners that fall into one
gap of the base, at empty sides, at the base as its own partner, at ranks with the top bit set (k = 32), at counters on both
sides of every range edge, and at a tile selected whole beside tiles not selected at all.  No launch of the selection's own
kernels strides over tiles; the tally of the result's counters does, and tests/test_gpu_counter_grid.py takes its later trips."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import db_compare_ref as cref
import db_select_ref as ref
import kmerdb_files as kf
from test_gpu_kmerdb import _fastq, _library, _two_parents
from test_gpu_kmerdb_compare import DENSE, FULL_HPC, _cases, _counters, _plant, _trio
from test_gpu_kmerdb_table import TILE, _distinct_ranks, _write_db, packed_keys
from test_gpu_kmerdb_union import _write_full

pytestmark = pytest.mark.gpu

FULL = b"TBKKMFB1"
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
KS = (2, 16, 21, 31, 32)
FLOORS = ((2, 2, 2), (1, 1, 1), (1, 2, 2), (2, 1, 2))  # base, first partner, second partner
VALUES = (1, 2, 127, 128, 254, 255)
RANGES = ((1, 255), (2, 255), (64, 64), (1, 1), (255, 255), (65, 255))
R, E = ref.REQUIRE, ref.EXCLUDE
RULE_NAMES = {ref.BASE: "base", ref.MIN: "min", ref.SUM: "sum"}
EMPTY = np.zeros(0, dtype=np.uint64)


def _write(path, k, keys, counts, floor, **kw):
    return _write_full(path, k, keys, counts, **kw) if floor == 1 else _write_db(path, k, keys, counts)


def _select(base, base_range, partners, rule):
    """partners: (database, keys, counts, (min, max), mode) -> KmerDatabase.select"""
    groups = {R: [], E: []}
    for db, _, _, (lo, hi), mode in partners:
        groups[mode].append((db, lo, hi))
    return base.select(base_range[0], base_range[1], require=groups[R], exclude=groups[E], counter=RULE_NAMES[rule])


def _select_raw(gpu, base, base_range, partners, rule, n_partners=None, size=None):
    """the library's call itself, partners in the order given: (status, handle)"""
    o = gpu.SelectOptions()
    gpu.lib.tbk_select_options_init(C.byref(o))
    assert (o.size, o.min_count, o.max_count, o.counter) == (C.sizeof(gpu.SelectOptions), 1, 255, 0)
    o.min_count, o.max_count, o.counter = base_range[0], base_range[1], rule
    if size is not None:
        o.size = size
    arr = (gpu.SelectPartner * max(1, len(partners)))()
    for slot, (db, _, _, (lo, hi), mode) in zip(arr, partners):
        slot.db, slot.min_count, slot.max_count, slot.mode = (None if db is None else db._h.value), lo, hi, mode
    h = C.c_void_p(1)
    rc = gpu.lib.tbk_kmerdb_select(None if base is None else base._h, arr, len(partners) if n_partners is None else n_partners, C.byref(o), C.byref(h))
    return rc, h


def _want(x, cx, base_range, partners, rule):
    return ref.select(x, cx, base_range, [(keys, counts, rng_, mode) for _, keys, counts, rng_, mode in partners], rule)


def _same(db, want, base, what):
    keys, counts, hist = want
    assert (len(db), db.floor, db.k, db.compressed, db.device) == (keys.size, 1, base.k, base.compressed, base.device), what
    got = db.entries()
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts), (what, got[0].size, keys.size)
    assert np.array_equal(db.histogram(), hist), what
    stats = db.stats()
    assert (stats["reads_added"], stats["bases_added"], stats["bytes"]) == (0, 0, 9 * keys.size), what


def _check(base, x, cx, base_range, partners, rule, what):
    want = _want(x, cx, base_range, partners, rule)
    with _select(base, base_range, partners, rule) as got:
        _same(got, want, base, what)
    return want[0].size


# ---- 1: sizes and overlaps ------------------------------------------------------------------------------------------------------------
def _shapes(me, other):
    """the selections run on every (base, partner) of the size cases: `me` and `other` are (database, keys, counts)"""
    return (
        ((1, 255), [other + ((1, 255), R)], ref.SUM),
        ((2, 255), [other + ((1, 255), E)], ref.BASE),
        ((1, 255), [other + ((2, 255), R), other + ((128, 255), E)], ref.MIN),
        ((1, 255), [me + ((1, 255), R), other + ((1, 255), E)], ref.SUM),  # the base as its own partner
        ((1, 200), [me + ((1, 1), E)], ref.MIN),
        ((1, 255), [me + ((2, 255), R), me + ((1, 127), R)], ref.SUM),
    )


@pytest.mark.parametrize("k", KS)
def test_selection_at_every_size_and_overlap(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(300 + k)
    kinds, met, kept = set(), set(), {"some": 0, "none": 0, "all": 0}
    for name, x, y in _cases(rng, k):
        cx, cy = _counters(rng, x.size, 1), _counters(rng, y.size, 2)
        _plant(x, cx, y, cy, 1, 2)
        with kmers.KmerDatabase.load(_write_full(tmp_path / "x.tbkdb", k, x, cx)) as dx, kmers.KmerDatabase.load(_write_db(tmp_path / "y.tbkdb", k, y, cy)) as dy:
            for me, other in (((dx, x, cx), (dy, y, cy)), ((dy, y, cy), (dx, x, cx))):
                for base_range, partners, rule in _shapes(me, other):
                    n = _check(me[0], me[1], me[2], base_range, partners, rule, (k, name, me[1].size, base_range, [p[3:] for p in partners], rule))
                    kept["none" if n == 0 else "all" if n == me[1].size else "some"] += 1
            # the inputs are as they were
            assert np.array_equal(dx.entries()[0], x) and np.array_equal(dx.entries()[1], cx) and np.array_equal(dy.entries()[1], cy)
        kinds.add(name[0])
        met |= {x.size, y.size}
    assert all(kept.values()), kept
    if k == 2:
        assert 16 in met and 0 in met  # all 16 ranks, and their subsets
    else:
        assert kinds == {"equal", "every_second", "disjoint", "mixed", "y_empty", "dense_in_one_gap", "both_empty"} and met >= set(SIZES) | {DENSE}


# ---- 2: modes, floors, rules, ranges ---------------------------------------------------------------------------------------------------
def _spread_counters(rng, n, floor):
    """floor..255 without 64: the counter the crafted whole tile alone holds"""
    c = _counters(rng, n, floor)
    c[c == 64] = 63
    return c


def _crafted_three(rng, k, n, floors):
    """(x, cx), (y, cy), (z, cz): y and z overlap x in a third and in half of its keys and hold keys of their own; on keys all
    three hold, every pair of VALUES the floors allow stands between the base and either partner; with four tiles, tile 1 of
    the base holds the only counters 64 - a tile selected whole by [64, 64] beside tiles not selected at all."""
    ranks = _distinct_ranks(rng, k, 3 * n)
    x = ranks[np.sort(rng.choice(ranks.size, size=n, replace=False))]
    pool = np.setdiff1d(ranks, x)
    y, z = np.union1d(x[1::3], pool[:n // 2]), np.union1d(x[::2], pool[n // 3:n])
    cx, cy, cz = (_spread_counters(rng, keys.size, floor) for keys, floor in zip((x, y, z), floors))
    whole = slice(TILE, 2 * TILE) if n > 2 * TILE else slice(0, 0)
    cx[whole] = 64
    outside = np.ones(n, dtype=bool)
    outside[whole] = False
    shared = x[outside & np.isin(x, y) & np.isin(x, z)]
    vx, vy, vz = ([v for v in VALUES if v >= floor] for floor in floors)
    assert shared.size >= 72
    for j, key in enumerate(shared[:: shared.size // 72][:72]):
        cx[np.searchsorted(x, key)] = vx[j % len(vx)]
        cy[np.searchsorted(y, key)] = vy[(j // len(vx)) % len(vy)]
        cz[np.searchsorted(z, key)] = vz[(j // len(vx) + j % len(vx)) % len(vz)]
    for (p, cp, vp) in ((y, cy, vy), (z, cz, vz)):  # every pair the floors allow met on some shared key
        at = np.isin(x, p)
        assert set(zip(cx[at].tolist(), cref.counter_in(p, cp, x[at]).tolist())) >= set(itertools.product(vx, vp))
    return (x, cx), (y, cy), (z, cz)


@pytest.mark.parametrize("n", [TILE + 1, 3 * TILE + 17])
def test_every_mode_floor_rule_and_range(gpu, tmp_path, n):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(400 + n)
    mode_shapes = [()] + [(m,) for m in (R, E)] + list(itertools.product((R, E), (R, E)))
    turn = itertools.count()
    seen = {"none": 0, "whole_tile": 0, "sum_saturated": 0, "min_from_partner": 0, "min_from_base": 0, "triples": set()}
    for floors in FLOORS:
        (x, cx), (y, cy), (z, cz) = _crafted_three(rng, k, n, floors)
        paths = [_write(tmp_path / (name + ".tbkdb"), k, keys, counts, floor) for name, keys, counts, floor in
                 (("x", x, cx, floors[0]), ("y", y, cy, floors[1]), ("z", z, cz, floors[2]))]
        with kmers.KmerDatabase.load(paths[0]) as dx, kmers.KmerDatabase.load(paths[1]) as dy, kmers.KmerDatabase.load(paths[2]) as dz:
            assert (dx.floor, dy.floor, dz.floor) == floors
            both = ((dy, y, cy), (dz, z, cz))
            for modes, rule, _ in itertools.product(mode_shapes, (ref.BASE, ref.MIN, ref.SUM), range(3)):
                t = next(turn)
                ranges = (RANGES[t % 6], RANGES[(t // 6) % 6], RANGES[(t // 36) % 6])
                seen["triples"].add(ranges)
                partners = [p + (ranges[1 + i], mode) for i, (p, mode) in enumerate(zip(both, modes))]
                want = _want(x, cx, ranges[0], partners, rule)
                rc, h = _select_raw(gpu, dx, ranges[0], partners, rule)  # (the library's call: the partners in this order)
                assert rc == 0 and h.value, (gpu.last_error(), floors, modes, rule, ranges)
                with kmers.KmerDatabase(h) as got:
                    _same(got, want, dx, (floors, modes, rule, ranges))
                seen["none"] += want[0].size == 0
                required = [cref.counter_in(p[1], p[2], want[0]) for p, mode in zip(both, modes) if mode == R]
                if required and want[0].size:
                    mine = cref.counter_in(x, cx, want[0])
                    low = np.minimum.reduce(required)
                    if rule == ref.SUM:
                        seen["sum_saturated"] += int(((mine + sum(required) > 255) & (mine < 255)).sum())
                    if rule == ref.MIN:
                        seen["min_from_partner"] += int((low < mine).sum())
                        seen["min_from_base"] += int((low > mine).sum())
            # a range that selects nothing: no partner holds a counter 64
            for rule in (ref.BASE, ref.SUM):
                assert _check(dx, x, cx, (1, 255), [both[0] + ((64, 64), R)], rule, "nothing") == 0
                assert _check(dx, x, cx, (1, 255), [both[1] + ((64, 64), E), both[0] + ((64, 64), R)], rule, "nothing") == 0
            # a tile selected whole beside tiles not selected at all, and the reverse
            if n > 2 * TILE:
                for rule in (ref.BASE, ref.MIN):
                    with dx.select(64, 64, counter=RULE_NAMES[rule]) as got:
                        assert np.array_equal(got.entries()[0], x[TILE:2 * TILE]) and (got.entries()[1] == 64).all() and int(got.histogram()[64]) == TILE
                    assert _check(dx, x, cx, (64, 64), [both[1] + ((1, 255), R)], ref.SUM, "whole tile, half of it held") == np.isin(x[TILE:2 * TILE], z).sum()
                    with dx.select(1, 63, exclude=[(dx, 64, 64)]) as below, dx.select(65, 255) as above:
                        assert len(below) + len(above) == n - TILE
                        assert np.array_equal(np.union1d(below.entries()[0], above.entries()[0]), np.concatenate([x[:TILE], x[2 * TILE:]]))
                seen["whole_tile"] += 1
    assert seen["none"] and seen["sum_saturated"] and seen["min_from_partner"] and seen["min_from_base"], seen
    assert seen["whole_tile"] == (len(FLOORS) if n > 2 * TILE else 0)
    for place in range(3):  # every range in every place
        assert {t[place] for t in seen["triples"]} == set(RANGES)


# ---- 3: agreement with the calls that exist -------------------------------------------------------------------------------------------
def _ranks_of_text(path, k):
    """(ranks, counters) of a counted dump: KMER<tab>COUNT lines"""
    keys, counts = [], []
    for line in open(path):
        kmer, count = line.rstrip("\n").split("\t")
        assert len(kmer) == k
        rank = 0
        for ch in kmer:
            rank = rank * 4 + "ACGT".index(ch)
        keys.append(rank)
        counts.append(int(count))
    return np.array(keys, dtype=np.uint64), np.array(counts, dtype=np.uint8)


@pytest.mark.parametrize("cuts", [((2, 255), (2, 255), 2), ((5, 30), (3, 200), 4)])
def test_hapmer_selection_agrees_with_the_inherited_list_and_the_origin_spectrum(gpu, tmp_path, cuts):
    from trio_binning_amd import kmers

    k = 21
    range_a, range_b, cmin = cuts
    (a, ca), (b, cb), (c, cc) = _trio(np.random.default_rng(6), k, 3 * TILE + 17)
    paths = [_write_db(tmp_path / (name + ".tbkdb"), k, keys, counts) for name, keys, counts in (("a", a, ca), ("b", b, cb), ("c", c, cc))]
    with kmers.KmerDatabase.load(paths[0]) as da, kmers.KmerDatabase.load(paths[1]) as db, kmers.KmerDatabase.load(paths[2]) as dc:
        for own, other, (lo, hi), (p, cp) in ((da, db, range_a, (a, ca)), (db, da, range_b, (b, cb))):
            with own.unique_set(other, lo, hi, child=dc, child_min=cmin, child_max=255) as hs:
                listed = hs.keys()
            assert listed.size > 300
            # base = the child: the same k-mers, in the child's order and with the child's counters
            with dc.select(cmin, 255, require=[(own, lo, hi)], exclude=[other]) as from_child:
                keys, counts = from_child.entries()
                assert set(packed_keys(keys, k).tolist()) == set(listed.tolist()) and keys.size == listed.size
                assert np.array_equal(counts, cref.counter_in(c, cc, keys)) and (keys[1:] > keys[:-1]).all()
                cells = dc.origin_spectrum(own, other, (lo, hi), (1, 255))
                assert len(from_child) == int(cells[1, cmin:].sum())  # the own parent holds it in range, the other parent does not
            # base = the parent: the list's own order, the parent's counters
            with own.select(lo, hi, exclude=[other], require=[(dc, cmin, 255)]) as from_parent:
                keys, counts = from_parent.entries()
                assert np.array_equal(packed_keys(keys, k), listed) and np.array_equal(counts, cref.counter_in(p, cp, keys))
                cells = own.origin_spectrum(other, dc, (1, 255), (cmin, 255))
                assert len(from_parent) == int(cells[2, lo:hi + 1].sum())
            with own.select(lo, hi, exclude=[other]) as unique, own.unique_set(other, lo, hi) as hs:
                assert np.array_equal(packed_keys(unique.entries()[0], k), hs.keys())
                assert len(unique) == int(cells[0, lo:hi + 1].sum() + cells[2, lo:hi + 1].sum())


def test_selection_agrees_with_solid_and_with_the_dump(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(31)
    x = _distinct_ranks(rng, k, 3 * TILE + 17)
    cx = _counters(rng, x.size, 1)
    assert (cx == 1).sum() > 10
    with kmers.KmerDatabase.load(_write_full(tmp_path / "full.tbkdb", k, x, cx)) as full:
        with full.select(2, 255) as picked, full.solid() as solid:
            assert picked.floor == 1 and solid.floor == 2 and len(picked) == len(solid) == int((cx >= 2).sum())
            assert all(np.array_equal(g, w) for g, w in zip(picked.entries(), solid.entries()))
            with picked.solid() as again:  # nothing but counter-1 entries would go: none here
                assert all(np.array_equal(g, w) for g, w in zip(again.entries(), solid.entries()))
        for lo, hi in ((1, 255), (3, 20), (1, 1), (255, 255), (250, 251)):
            path = str(tmp_path / "dump.txt")
            n = full.dump(path, lo, hi)
            with full.select(lo, hi) as picked:
                keys, counts = _ranks_of_text(path, k)
                assert n == len(picked) == keys.size
                assert np.array_equal(picked.entries()[0], keys) and np.array_equal(picked.entries()[1], counts)


# ---- 4: files ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magic", [FULL, FULL_HPC])
def test_a_selection_saves_loads_and_unites(gpu, tmp_path, magic):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(41)
    ranks = _distinct_ranks(rng, k, 4 * TILE + 300)
    x, y = ranks[rng.random(ranks.size) < 0.7], ranks[rng.random(ranks.size) < 0.6]
    cx, cy = _counters(rng, x.size, 1), _counters(rng, y.size, 1)
    _plant(x, cx, y, cy, 1, 1)
    with kmers.KmerDatabase.load(_write_full(tmp_path / "x.tbkdb", k, x, cx, magic=magic)) as dx, \
            kmers.KmerDatabase.load(_write_full(tmp_path / "y.tbkdb", k, y, cy, magic=magic)) as dy:
        assert dx.compressed == (magic == FULL_HPC)
        for rule in (ref.BASE, ref.SUM):
            partners = [(dy, y, cy, (2, 255), R)]
            keys, counts, hist = _want(x, cx, (1, 200), partners, rule)
            path = str(tmp_path / "picked.tbkdb")
            with _select(dx, (1, 200), partners, rule) as picked:
                picked.save(path)
            assert keys.size > TILE and open(path, "rb").read() == kf.file_bytes(k, keys, counts, hist, reads=0, bases=0, magic=magic)
            info = kmers.database_file_info(path)
            assert (info["floor"], info["compressed"], info["n"], info["reads_added"], info["bases_added"]) == (1, magic == FULL_HPC, keys.size, 0, 0)
            with kmers.KmerDatabase.load(path) as back, back.union(back) as twice:
                assert np.array_equal(back.entries()[0], keys) and np.array_equal(back.entries()[1], counts)
                assert np.array_equal(twice.entries()[0], keys)
                assert np.array_equal(twice.entries()[1], np.minimum(2 * counts.astype(np.int64), 255).astype(np.uint8))
        # the empty selection, and a selection from an empty base
        for n, (base, partner) in enumerate(((dx, (dx, 1, 255)), (dy, (dx, 1, 255)))):
            path = str(tmp_path / "empty{}.tbkdb".format(n))
            with (base.select(exclude=[partner]) if n == 0 else base.select(255, 255, require=[(base, 1, 1)])) as none:
                assert len(none) == 0 and none.floor == 1 and not none.histogram().any() and none.entries()[0].size == 0
                none.save(path)
            assert os.path.getsize(path) == 2096 == kf.HEADER
            assert open(path, "rb").read() == kf.file_bytes(k, EMPTY, EMPTY.astype(np.uint8), np.zeros(256, dtype=np.uint64), magic=magic)
            with kmers.KmerDatabase.load(path) as back, back.select(require=[dx], counter="sum") as of_nothing, dx.select(require=[back]) as by_nothing:
                assert (len(back), back.floor, back.k, len(of_nothing), len(by_nothing)) == (0, 1, k, 0, 0)


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def zoo(gpu, tmp_path):
    """{name: (database, keys, counts)}: full and floor-2 databases of two k and both spaces"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(7)
    out = {}
    for name, k, floor, magic, n in (("full21", 21, 1, None, 1500), ("solid21", 21, 2, None, 1200), ("full16", 16, 1, None, 1500),
                                     ("fullh21", 21, 1, FULL_HPC, 1500)):
        keys, counts = _distinct_ranks(rng, k, n), _counters(rng, n, floor)
        path = _write(tmp_path / (name + ".tbkdb"), k, keys, counts, floor, **({"magic": magic} if magic else {}))
        out[name] = (kmers.KmerDatabase.load(path), keys, counts)
    yield out
    for db, _, _ in out.values():
        db.close()


def test_refusals_leave_the_inputs_and_no_database(gpu, zoo):
    from trio_binning_amd import _lib, kmers

    full, solid, full16, fullh = (zoo[name] for name in ("full21", "solid21", "full16", "fullh21"))
    hists = {name: db.histogram() for name, (db, _, _) in zoo.items()}
    ok, bad_ranges = (1, 255), ((0, 5), (5, 4), (1, 256), (256, 256), (0, 0), (255, 1), (1, 0xFFFFFFFF))

    def works():
        partners = [solid + ((2, 255), R), full + ((1, 1), E)]
        rc, h = _select_raw(gpu, full[0], (1, 255), partners, ref.SUM)
        assert rc == 0
        with kmers.KmerDatabase(h) as got:
            _same(got, _want(full[1], full[2], (1, 255), partners, ref.SUM), full[0], "after a refusal")
        for name, (db, keys, counts) in zoo.items():
            got = db.entries()
            assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts) and np.array_equal(db.histogram(), hists[name]), name

    def refused(words, *args, **kw):
        rc, h = _select_raw(gpu, *args, **kw)
        msg = gpu.last_error()
        assert rc == gpu.TBK_ERR_INVALID and not h.value and all(w in msg for w in words), (words, rc, msg)

    works()
    p_ok = solid + (ok, R)
    none = (None, None, None, ok, R)
    refused(["NULL"], None, ok, [p_ok], ref.BASE)
    refused(["NULL"], full[0], ok, [none], ref.BASE)
    refused(["NULL"], full[0], ok, [p_ok, none], ref.BASE)
    for n_partners in (-1, 3, 1 << 20):
        refused(["partners"], full[0], ok, [p_ok, p_ok], ref.BASE, n_partners=n_partners)
    for mode in (0, 3, -1):
        refused(["mode"], full[0], ok, [solid + (ok, mode)], ref.BASE)
        refused(["mode", "second"], full[0], ok, [p_ok, solid + (ok, mode)], ref.BASE)
    for rule in (-1, 3, 100):
        refused(["counter rule"], full[0], ok, [p_ok], rule)
    for bad in bad_ranges:
        refused(["1 <= min <= max <= 255", "base"], full[0], bad, [p_ok], ref.BASE)
        refused(["1 <= min <= max <= 255", "first"], full[0], ok, [solid + (bad, E)], ref.MIN)
        refused(["1 <= min <= max <= 255", "second"], full[0], ok, [p_ok, solid + (bad, R)], ref.SUM)
        with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
            full[0].select(bad[0], bad[1])
        with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
            full[0].select(exclude=[(solid[0], bad[0], bad[1])])
    with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
        full[0].select(-1, 255)
    refused(["different k", "21", "16"], full[0], ok, [full16 + (ok, R)], ref.BASE)
    refused(["different k"], full16[0], ok, [p_ok, full16 + (ok, E)], ref.BASE)
    refused(["homopolymer-compressed", "plain"], full[0], ok, [fullh + (ok, E)], ref.BASE)
    refused(["homopolymer-compressed", "plain"], fullh[0], ok, [fullh + (ok, E), solid + (ok, R)], ref.BASE)
    refused(["tbk_select_options_init"], full[0], ok, [p_ok], ref.BASE, size=0)
    works()
    # NULL options and NULL out
    arr = (gpu.SelectPartner * 1)()
    h = C.c_void_p(1)
    assert gpu.lib.tbk_kmerdb_select(full[0]._h, arr, 0, None, C.byref(h)) == gpu.TBK_ERR_INVALID and not h.value and "NULL" in gpu.last_error()
    o = gpu.SelectOptions()
    gpu.lib.tbk_select_options_init(C.byref(o))
    assert gpu.lib.tbk_kmerdb_select(full[0]._h, arr, 0, C.byref(o), None) == gpu.TBK_ERR_INVALID and "NULL" in gpu.last_error()
    h = C.c_void_p(1)
    assert gpu.lib.tbk_kmerdb_select(full[0]._h, None, 1, C.byref(o), C.byref(h)) == gpu.TBK_ERR_INVALID and not h.value
    # no partners at all may come with a NULL array
    h = C.c_void_p(1)
    assert gpu.lib.tbk_kmerdb_select(full[0]._h, None, 0, C.byref(o), C.byref(h)) == 0
    with kmers.KmerDatabase(h) as got:
        _same(got, _want(full[1], full[2], ok, [], ref.BASE), full[0], "no partner")
    # the method: three partners, a rule that is none, mixed k and spaces - the first two before the library is called
    from unittest.mock import patch

    with patch.object(_lib.lib, "tbk_kmerdb_select", side_effect=AssertionError("the library was called")):
        with pytest.raises(ValueError, match="at most two"):
            full[0].select(require=[solid[0], full[0]], exclude=[solid[0]])
        with pytest.raises(ValueError, match="at most two"):
            full[0].select(exclude=[solid[0], (full[0], 2, 9), solid[0]])
        with pytest.raises(ValueError, match="'base', 'min', 'sum'"):
            full[0].select(counter="max")
    with pytest.raises(ValueError, match="different k"):
        full[0].select(require=[full16[0]])
    with pytest.raises(ValueError, match="homopolymer-compressed"):
        solid[0].select(exclude=[(fullh[0], 2, 255)])
    works()


# ---- 6: the commands ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio(gpu, tmp_path_factory):
    """The library of test_gpu_kmerdb_table's trio (the reference's rule finds [5,35] for both parents) and a child of reads of
    both parents' genomes, counted once with --child --keep-databases: three databases."""
    from trio_binning_amd import find_unique_kmers as fu

    root = tmp_path_factory.mktemp("hapmers")
    k = 21
    rng = np.random.default_rng(277)
    ga, gb = _two_parents(rng, glen=20_000)
    reads_a, reads_b = _library(rng, ga, 3500, 150), _library(rng, gb, 3500, 150)
    rng = np.random.default_rng(279)
    reads_c = _library(rng, ga, 1750, 150) + _library(rng, gb, 1750, 150)
    fa, fb, fc = _fastq(root / "a.fastq", reads_a), _fastq(root / "b.fastq.gz", reads_b, gz=True), _fastq(root / "c.fastq", reads_c)
    out = root / "lists"
    out.mkdir()
    fu.main(["-k", str(k), "-o", str(out), "-s", str(out), "--capacity", "1500000", "--keep-databases", "--child", fc, "--min-count-child", "3", fa, fb])
    return {"k": k, "root": root, "assembly": _fastq(root / "asm.fastq", [ga[:6000], gb[6000:9000]]),
            "db_a": str(out / "haplotypeA.tbkdb"), "db_b": str(out / "haplotypeB.tbkdb"), "db_child": str(out / "child.tbkdb")}


def _entries_of(path):
    from trio_binning_amd import kmers

    with kmers.KmerDatabase.load(path) as db:
        return db.entries() + (db.histogram(), db.floor)


def test_select_database_on_a_toy_trio(trio, tmp_path, capsys):
    from trio_binning_amd import select_database as sd

    (a, ca, _, _), (b, cb, _, _), (c, cc, _, _) = (_entries_of(trio[name]) for name in ("db_a", "db_b", "db_child"))
    out = str(tmp_path / "picked.tbkdb")
    capsys.readouterr()
    # what both parents hold, A's counters from 5 on, summed
    sd.main(["-o", out, "--min-count", "5", "--require", trio["db_b"] + ":2", "--counter", "sum", trio["db_a"]])
    want = ref.select(a, ca, (5, 255), [(b, cb, (2, 255), R)], ref.SUM)
    err = capsys.readouterr().err
    assert want[0].size > 1000 and "{} of the {} k-mers of {} kept".format(want[0].size, a.size, trio["db_a"]) in err
    assert open(out, "rb").read() == kf.file_bytes(trio["k"], *want, magic=FULL)
    # the child's k-mers of neither parent; the base named as its own partner
    sd.main(["-o", out, "--exclude", trio["db_a"], "--exclude", trio["db_b"], trio["db_child"]])
    want = ref.select(c, cc, (1, 255), [(a, ca, (1, 255), E), (b, cb, (1, 255), E)], ref.BASE)
    assert 0 < want[0].size < c.size and open(out, "rb").read() == kf.file_bytes(trio["k"], *want, magic=FULL)
    sd.main(["-o", out, "--require", trio["db_child"] + ":3:40", "--counter", "min", "--max-count", "40", trio["db_child"]])
    want = ref.select(c, cc, (1, 40), [(c, cc, (3, 40), R)], ref.MIN)
    assert want[0].size and open(out, "rb").read() == kf.file_bytes(trio["k"], *want, magic=FULL)
    # an empty selection is written, and stderr says so
    capsys.readouterr()
    sd.main(["-o", out, "--exclude", trio["db_a"], trio["db_a"]])
    err = capsys.readouterr().err
    assert os.path.getsize(out) == 2096 and "none of the {} k-mers".format(a.size) in err and "empty database" in err
    assert _entries_of(out)[0].size == 0


def test_hapmers_on_a_toy_trio_and_its_completeness(trio, tmp_path, capsys):
    from trio_binning_amd import assembly_qv, hapmers as hm, kmers

    k = trio["k"]
    out = str(tmp_path / "hap")
    argv = ["-o", out, trio["db_a"], trio["db_b"], "--child-database", trio["db_child"], "--min-count-child", "3"]
    capsys.readouterr()
    hm.main(argv)
    err = capsys.readouterr().err
    assert err.count("Using counts in range [5,35]") == 2 and "Using counts in range [3,255] for the child" in err
    files = {hap: os.path.join(out, "haplotype{}.hapmers.tbkdb".format(hap)) for hap in "AB"}
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in files.values())
    (a, ca, _, _), (b, cb, _, _), (c, cc, _, _) = (_entries_of(trio[name]) for name in ("db_a", "db_b", "db_child"))
    # what classify-by-kmers --child-database finds: its own selection from the same settled command line
    found = hm.parse_args(argv).databases.load()
    said = capsys.readouterr().err
    try:
        for hap, hs, (own, c_own), (other, c_other) in (("A", found[0], (a, ca), (b, cb)), ("B", found[1], (b, cb), (a, ca))):
            keys, counts, hist, floor = _entries_of(files[hap])
            assert floor == 1 and keys.size == hs.num_kmers > 500
            assert "Found {} {}-mers unique to haplotype {} and inherited by the child".format(keys.size, k, hap) in said
            assert np.array_equal(np.sort(packed_keys(keys, k)), np.sort(hs.keys()))
            assert np.array_equal(counts, cref.counter_in(c, cc, keys)) and counts.min() >= 3
            want = ref.select(c, cc, (3, 255), [(own, c_own, (5, 35), R), (other, c_other, (1, 255), E)], ref.BASE)
            assert open(files[hap], "rb").read() == kf.file_bytes(k, *want, magic=FULL)
            n_own = int(((c_own >= 5) & (c_own <= 35) & ~np.isin(own, other)).sum())
            line = [l for l in err.splitlines() if l.startswith("hapmers: haplotype {}: {} hap-mers".format(hap, keys.size))]
            assert len(line) == 1 and "{:.6f} of the {} k-mers".format(keys.size / n_own, n_own) in line[0] and "child's counts from 3 on" in line[0]
            assert 0.3 < keys.size / n_own <= 1.0  # (the child holds one haplotype of each parent, and those parents have one)
    finally:
        for hs in found:
            hs.close()
    # hap-mer completeness: assembly_qv's completeness on such a database, against the query session itself
    bases, offsets = kmers.pack_reads([open(trio["assembly"]).read().split("\n")[1], open(trio["assembly"]).read().split("\n")[5]])
    for hap in "AB":
        capsys.readouterr()
        assembly_qv.main([trio["assembly"], files[hap], "--min-count", "1"])
        total = [l for l in capsys.readouterr().out.splitlines() if l.startswith("#total")][0].split("\t")
        with kmers.KmerDatabase.load(files[hap]) as db, db.query() as query:
            query.add(bases, offsets, 1)
            seen, solid = query.completeness(1, 255)
            assert solid == len(db)
        assert (int(total[5]), int(total[6]), total[7]) == (seen, solid, assembly_qv.format_completeness(seen, solid)) and seen > 0
