"""The GC x count matrix of a count database and the selection by GC content on the device (include/tbk.h):
tbk_kmerdb_gc_spectrum, the min_gc / max_gc of tbk_select_options, kmers.KmerDatabase.gc_spectrum / select(gc=...), and the
gc_spectrum and select_database commands on top.

Crafted databases are files this test writes itself (tests/kmerdb_files.py through the helpers of the table, union and compare
tests) and every expectation is numpy's (tests/db_gc_ref.py, tests/db_select_ref.py): integer counts, compared exactly.  The
kernel strides over tiles of 1024 entries and tallies (k + 1) x 256 cells in LDS, whole or only the counters below 64, so the
shapes aim at the tile edges (every size around a wave, a block round and a tile), at ranks with the top bit set (k = 32), at
the extreme rows that random keys never reach, at counters on both sides of 64 and at both ends, at a database that is ONE
cell, and at the later trips of the strided loop (tbk_count_set_grid_caps_)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import db_gc_ref as ref
import db_select_ref as sref
import kmerdb_files as kf
from test_gpu_kmerdb import _fastq, _library, _random_dna
from test_gpu_kmerdb_compare import _counters
from test_gpu_kmerdb_table import TILE, _distinct_ranks, _write_db
from test_gpu_kmerdb_union import _write_full

pytestmark = pytest.mark.gpu

FULL, FULL_HPC, SOLID_HPC = b"TBKKMFB1", b"TBKKMFH1", b"TBKKMDH1"
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
KS = (2, 16, 21, 31, 32)
FORMS = ((2, False), (1, False), (1, True), (2, True))  # (floor, homopolymer-compressed): both floors, both magics of each
VALUES = (1, 2, 127, 128, 254, 255)
R, E = sref.REQUIRE, sref.EXCLUDE
EMPTY = np.zeros(0, dtype=np.uint64)


def _write(path, k, keys, counts, floor, compressed=False):
    if floor == 1:
        return _write_full(path, k, keys, counts, magic=FULL_HPC if compressed else FULL)
    if not compressed:
        return _write_db(path, k, keys, counts)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 3
    hist[0] = keys.size + 3
    with open(path, "wb") as fh:
        fh.write(kf.file_bytes(k, keys, counts, hist, reads=1, bases=k, magic=SOLID_HPC))
    return str(path)


def _check(db, keys, counts, k, what):
    """the device's matrix: its own invariants first, then the reference cell by cell; returns it"""
    got = db.gc_spectrum()
    assert got.shape == (k + 1, 256) and got.dtype == np.uint64, what
    assert int(got.sum()) == keys.size == len(db) and not got[:, 0].any(), what
    # the columns sum to the database's own counters: histogram()[1:] of a full database; row 1 of a floor-2 header counts
    # k-mers the database does not hold
    assert np.array_equal(got.sum(axis=0)[db.floor:], db.histogram()[db.floor:]) and not got[:, :db.floor].any(), what
    want = ref.gc_spectrum(keys, counts, k)
    assert np.array_equal(got, want), (what, [(int(g), int(c), int(got[g, c]), int(want[g, c])) for g, c in zip(*np.nonzero(got != want))][:8])
    return got


def _raw(gpu, db):
    """the library's call itself on all its 33 rows: (status, matrix)"""
    spec = np.zeros((33, 256), dtype=np.uint64)
    return gpu.lib.tbk_kmerdb_gc_spectrum(None if db is None else db._h, spec.ctypes.data), spec


def _planted(k):
    """the keys random ranks never give: all-A, all-C, all-G, all-T, alternating CG and GC, and one key of every row 0..k"""
    words = ["A" * k, "C" * k, "G" * k, "T" * k, ("CG" * k)[:k], ("GC" * k)[:k]]
    words += ["C" * g + "A" * (k - g) for g in range(k + 1)] + ["T" * (k - g) + "G" * g for g in range(k + 1)]
    return np.unique(np.array([ref.rank_of(w) for w in words], dtype=np.uint64))


# ---- 1: sizes and k ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_matrix_at_every_size_floor_and_space(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(400 + k)
    forms = itertools.cycle(FORMS)
    if k == 2:
        every = np.arange(16, dtype=np.uint64)
        sets = [every, EMPTY, every[5:6], every[::2], every[1::2], every[[0, 15]], every[3:9], every[[5, 10]]]
    else:
        sets = [_distinct_ranks(rng, k, n) for n in SIZES]
    seen = set()
    for keys in sets:
        for _ in range(2 if keys.size in (0, TILE + 1, 3 * TILE + 17, 16) else 1):  # (these sizes in two forms; 12 sizes step through all four anyway)
            floor, compressed = next(forms)
            counts = _counters(rng, keys.size, floor)
            edge = [v for v in VALUES if v >= floor][: keys.size]
            counts[: len(edge)] = edge
            with kmers.KmerDatabase.load(_write(tmp_path / "x.tbkdb", k, keys, counts, floor, compressed)) as db:
                assert (db.floor, db.compressed, db.k) == (floor, compressed, k)
                _check(db, keys, counts, k, (k, keys.size, floor, compressed))
                rc, all_rows = _raw(gpu, db)
                assert rc == 0 and not all_rows[k + 1:].any() and int(all_rows.sum()) == keys.size  # rows above k are zero
                assert np.array_equal(db.entries()[0], keys) and np.array_equal(db.entries()[1], counts)  # the database is only read
            seen.add((floor, compressed))
        if k == 32 and keys.size >= 63:
            assert int(keys[-1]) >> 63 == 1 and int(keys[0]) >> 63 == 0  # ranks on both sides of 2^63
    assert seen == set(FORMS)


# ---- 2: planted shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 21, 32])
def test_extreme_rows_every_row_and_every_edge_counter(gpu, tmp_path, k):
    """all-A and all-T (row 0), all-C, all-G, CGCG.. and GCGC.. (row k), a key of every row, among random ranks; the planted keys
    take the counters 1, 2, 127, 128, 254, 255 in turn"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(500 + k)
    planted = _planted(k)
    keys = np.union1d(_distinct_ranks(rng, k, 2 * TILE + 100), planted)
    counts = _counters(rng, keys.size, 1)
    at = np.searchsorted(keys, planted)
    counts[at] = [VALUES[j % len(VALUES)] for j in range(planted.size)]
    if k == 32:
        assert int(planted[-1]) == 2**64 - 1 and (planted >> np.uint64(63)).sum() >= k  # all-T, all-G, ... with the top bit set
    with kmers.KmerDatabase.load(_write(tmp_path / "x.tbkdb", k, keys, counts, 1)) as db:
        got = _check(db, keys, counts, k, ("planted", k))
    assert (got.sum(axis=1) > 0).all()  # every row 0..k is non-empty
    assert int(got[0].sum()) >= 2 and int(got[k].sum()) >= 4
    assert all(int(got[:, v].sum()) >= 1 for v in VALUES)
    # the planted keys alone: one or two entries a row, the extreme rows the heaviest
    sub = np.full(planted.size, 255, dtype=np.uint8)
    with kmers.KmerDatabase.load(_write(tmp_path / "p.tbkdb", k, planted, sub, 2)) as db:
        got = _check(db, planted, sub, k, ("planted alone", k))
    assert not got[:, :255].any() and (got[:, 255] >= 1).all()


@pytest.mark.parametrize("counter", [30, 200])
def test_a_database_that_is_one_cell(gpu, tmp_path, counter):
    """3 * 1024 + 17 entries of one GC and one counter: every LDS atomic of a wave (counter 30), or every global one (counter 200,
    beside a tally that keeps the counters below 64), hits one address; with the grid capped to one block that block's cell
    takes them all"""
    from trio_binning_amd import kmers

    k, g, n = 21, 10, 3 * TILE + 17
    rng = np.random.default_rng(60)
    ranks = _distinct_ranks(rng, k, 40_000)
    keys = ranks[ref.gc_of(ranks) == g][:n]
    assert keys.size == n
    counts = np.full(n, counter, dtype=np.uint8)
    want = np.zeros((k + 1, 256), dtype=np.uint64)
    want[g, counter] = n
    assert np.array_equal(ref.gc_spectrum(keys, counts, k), want)
    with kmers.KmerDatabase.load(_write(tmp_path / "x.tbkdb", k, keys, counts, 2)) as db:
        assert np.array_equal(db.gc_spectrum(), want)
        try:
            assert gpu.lib.tbk_count_set_grid_caps_(0, 1) == 0
            assert np.array_equal(db.gc_spectrum(), want)
        finally:
            gpu.lib.tbk_count_set_grid_caps_(0, 0)


# ---- 3: the later trips of the strided loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 32])
def test_later_trips_give_the_same_matrix(gpu, tmp_path, k):
    """3 * 1024 + 17 entries are four tiles: one block takes all four trips, two blocks two each"""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(70 + k)
    planted, n = _planted(k), 3 * TILE + 17
    ranks = _distinct_ranks(rng, k, n)
    keys = np.union1d(ranks[~np.isin(ranks, planted)][: n - planted.size], planted)
    assert keys.size == n
    counts = _counters(rng, keys.size, 1)
    with kmers.KmerDatabase.load(_write(tmp_path / "x.tbkdb", k, keys, counts, 1)) as db:
        whole = _check(db, keys, counts, k, "uncapped")
        try:
            for cap in (1, 2):
                assert gpu.lib.tbk_count_set_grid_caps_(0, cap) == 0
                assert np.array_equal(_check(db, keys, counts, k, ("cap", cap)), whole)
        finally:
            gpu.lib.tbk_count_set_grid_caps_(0, 0)


# ---- 4: selection by GC -------------------------------------------------------------------------------------------------------------
def _select_raw(gpu, base, gc, size=None, base_range=(1, 255)):
    """the library's call itself with no partner: (status, handle)"""
    o = gpu.SelectOptions()
    gpu.lib.tbk_select_options_init(C.byref(o))
    assert (o.size, o.min_count, o.max_count, o.counter, o.min_gc, o.max_gc) == (C.sizeof(gpu.SelectOptions), 1, 255, 0, 0, 32)
    o.min_count, o.max_count = base_range
    if gc is not None:
        o.min_gc, o.max_gc = gc
    if size is not None:
        o.size = size
    h = C.c_void_p(1)
    return gpu.lib.tbk_kmerdb_select(base._h, None, 0, C.byref(o), C.byref(h)), h


def _same(db, want, base, what):
    keys, counts, hist = want
    assert (len(db), db.floor, db.k, db.compressed) == (keys.size, 1, base.k, base.compressed), what
    got = db.entries()
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], counts), (what, got[0].size, keys.size)
    assert np.array_equal(db.histogram(), hist), what


@pytest.fixture(scope="module")
def family(gpu, tmp_path_factory):
    """x (full; the extreme rows planted), y (floor 2: a third of x and keys of its own) and z (full: half of x and others), k = 21"""
    from trio_binning_amd import kmers

    k = 21
    root = tmp_path_factory.mktemp("gc_select")
    rng = np.random.default_rng(80)
    planted, n = _planted(k), 3 * TILE + 17
    ranks = _distinct_ranks(rng, k, 3 * n)
    ranks = ranks[~np.isin(ranks, planted)]
    x = np.union1d(planted, rng.choice(ranks, size=n - planted.size, replace=False))  # x holds every planted key
    pool = np.setdiff1d(ranks, x)
    assert x.size == n and pool.size > n
    y, z = np.union1d(x[1::3], pool[::3]), np.union1d(x[::2], pool[1::3])
    cx, cy, cz = _counters(rng, x.size, 1), _counters(rng, y.size, 2), _counters(rng, z.size, 1)
    at = np.searchsorted(x, _planted(k))
    cx[at] = [VALUES[j % len(VALUES)] for j in range(at.size)]
    dbs = [kmers.KmerDatabase.load(_write(root / (name + ".tbkdb"), k, keys, counts, floor))
           for name, keys, counts, floor in (("x", x, cx, 1), ("y", y, cy, 2), ("z", z, cz, 1))]
    yield {"k": k, "root": root, "x": (dbs[0], x, cx), "y": (dbs[1], y, cy), "z": (dbs[2], z, cz)}
    for db in dbs:
        db.close()


GC_RANGES = ((0, 0), (21, 21), (0, 21), (9, 12), (11, None), (None, 9))


@pytest.mark.parametrize("gc", GC_RANGES)
def test_selection_by_gc_with_counters_partners_and_rules(gpu, family, gc):
    (dx, x, cx), (dy, y, cy), (dz, z, cz) = family["x"], family["y"], family["z"]
    bounds = (0 if gc[0] is None else gc[0], 32 if gc[1] is None else gc[1])
    kept = 0
    for base_range, (req, exc), rule in itertools.product(((1, 255), (2, 40)), ((False, False), (True, False), (False, True), (True, True)),
                                                          (sref.BASE, sref.MIN, sref.SUM)):
        partners = ([(y, cy, (2, 255), R)] if req else []) + ([(z, cz, (1, 100), E)] if exc else [])
        want = ref.select(x, cx, base_range, partners, rule, gc=bounds)
        with dx.select(base_range[0], base_range[1], require=[(dy, 2, 255)] if req else [], exclude=[(dz, 1, 100)] if exc else [],
                       counter={sref.BASE: "base", sref.MIN: "min", sref.SUM: "sum"}[rule], gc=gc) as got:
            _same(got, want, dx, (gc, base_range, req, exc, rule))
        kept += want[0].size
        if not req and not exc and base_range == (1, 255):  # the extreme rows are not empty: the planted keys are kept
            assert want[0].size >= (2 if gc in ((0, 0), (21, 21)) else 500)
    assert kept
    assert np.array_equal(dx.entries()[0], x) and np.array_equal(dx.entries()[1], cx)  # the inputs are as they were


def test_matrix_of_a_gc_selection_is_the_rows_of_the_base(gpu, family):
    dx, x, cx = family["x"]
    k = family["k"]
    base = dx.gc_spectrum()
    for lo, hi in ((0, 0), (k, k), (0, k), (9, 12), (11, 32), (0, 9), (5, 5)):
        want = np.zeros_like(base)
        want[lo:hi + 1] = base[lo:hi + 1]
        with dx.select(gc=(lo, hi)) as picked:
            assert np.array_equal(picked.gc_spectrum(), want), (lo, hi)
            assert len(picked) == int(want.sum())


def test_defaults_an_old_struct_and_a_bound_above_k_change_nothing(gpu, family, tmp_path):
    """the file of a selection without `gc` is the reference's of before the bounds; so are those of the defaults, of bounds that
    cannot bind, and of a caller whose struct ends with `counter` (size 24), whatever lies behind it"""
    from trio_binning_amd import kmers

    dx, x, cx = family["x"]
    k = family["k"]
    want = sref.select(x, cx, (2, 200), (), sref.BASE)
    data = kf.file_bytes(k, *want, reads=0, bases=0, magic=FULL)
    paths = []
    for n, gc in enumerate((None, (0, 32), (0, k), (None, None), (0, None), (None, k + 3))):
        paths.append(str(tmp_path / "picked{}.tbkdb".format(n)))
        with (dx.select(2, 200) if gc is None else dx.select(2, 200, gc=gc)) as picked:
            picked.save(paths[-1])
    assert all(open(path, "rb").read() == data for path in paths)
    assert C.sizeof(gpu.SelectOptions) == 32
    for garbage in ((7, 3), (0xFFFFFFFF, 0), (40, 50), (12, 12)):  # crossed, too large, binding: not read from a struct of 24 bytes
        rc, h = _select_raw(gpu, dx, garbage, size=24, base_range=(2, 200))
        assert rc == 0 and h.value, (garbage, gpu.last_error())
        with kmers.KmerDatabase(h) as got:
            _same(got, want, dx, ("size 24", garbage))
    rc, h = _select_raw(gpu, dx, (12, 12), size=28, base_range=(2, 200))  # a size that reaches max_gc states the bounds
    assert rc == 0
    with kmers.KmerDatabase(h) as got:
        _same(got, ref.select(x, cx, (2, 200), (), sref.BASE, gc=(12, 12)), dx, "size 28")
    rc, h = _select_raw(gpu, dx, None, size=19)  # the lower bound on size has not moved
    assert rc == gpu.TBK_ERR_INVALID and not h.value and "tbk_select_options_init" in gpu.last_error()


def test_gc_bounds_that_are_none_are_refused(gpu, family):
    from trio_binning_amd import kmers

    dx, x, cx = family["x"]
    hist = dx.histogram()
    for bad in ((5, 4), (21, 0), (0, 33), (33, 33), (1, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)):
        rc, h = _select_raw(gpu, dx, bad)
        msg = gpu.last_error()
        assert rc == gpu.TBK_ERR_INVALID and not h.value and "GC range" in msg and "0 <= min <= max <= 32" in msg, (bad, rc, msg)
        with pytest.raises(ValueError, match="GC range"):
            dx.select(gc=bad)
    with pytest.raises(ValueError, match="GC range"):
        dx.select(gc=(-1, 5))
    # the inputs are still usable
    assert np.array_equal(dx.entries()[0], x) and np.array_equal(dx.entries()[1], cx) and np.array_equal(dx.histogram(), hist)
    rc, h = _select_raw(gpu, dx, (32, 32))  # legal, above k: nothing has 32 G-or-C bases among 21
    assert rc == 0
    with kmers.KmerDatabase(h) as got:
        assert len(got) == 0
    with dx.select(gc=(3, 18)) as got:
        _same(got, ref.select(x, cx, gc=(3, 18)), dx, "after the refusals")


# ---- 5: refusals of the matrix call ---------------------------------------------------------------------------------------------------
def test_matrix_refusals_leave_the_database(gpu, family):
    dx, x, cx = family["x"]
    hist = dx.histogram()
    rc, spec = _raw(gpu, None)
    assert rc == gpu.TBK_ERR_INVALID and "NULL" in gpu.last_error() and "tbk_kmerdb_gc_spectrum" in gpu.last_error() and not spec.any()
    assert gpu.lib.tbk_kmerdb_gc_spectrum(dx._h, None) == gpu.TBK_ERR_INVALID and "NULL" in gpu.last_error()
    assert gpu.lib.tbk_kmerdb_gc_spectrum(None, None) == gpu.TBK_ERR_INVALID
    assert np.array_equal(dx.histogram(), hist) and int(hist[1:].sum()) == x.size  # the database still answers
    _check(dx, x, cx, family["k"], "after the refusals")


# ---- 6: the commands on a toy library ---------------------------------------------------------------------------------------------------
def _dna_of_gc(rng, n, gc):
    return "".join(rng.choice(list("ACGT"), size=n, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]))


def test_the_commands_on_a_library_with_a_second_cloud(gpu, tmp_path, capsys):
    """reads of a genome of 40 % GC at 15x and of a short sequence of 70 % GC at 45x, counted into a kept database: the command's
    lines and matrix are the reference's of the database's own entries, and select_database --min-gc carves by them.  Whether
    the second cloud is "found" is nobody's to say here: no verdict is computed"""
    from trio_binning_amd import find_unique_kmers as fu, gc_spectrum as gs, kmers, select_database as sd

    k = 21
    rng = np.random.default_rng(90)
    genome, other = _dna_of_gc(rng, 8000, 0.4), _dna_of_gc(rng, 1500, 0.7)
    reads = _library(rng, genome, 800, 150) + _library(rng, other, 450, 150)
    fa, fb = _fastq(tmp_path / "a.fastq", reads), _fastq(tmp_path / "b.fastq", _library(rng, _random_dna(rng, 3000), 200, 150))
    out = tmp_path / "out"
    out.mkdir()
    fu.main(["-k", str(k), "-o", str(out), "-s", str(out), "--capacity", "400000", "--keep-databases", "--keep-singletons", "--min-count-a", "3",
             "--max-count-a", "200", "--min-count-b", "3", "--max-count-b", "200", fa, fb])
    path = str(out / "haplotypeA.tbkdb")
    with kmers.KmerDatabase.load(path) as db:
        keys, counts = db.entries()
        floor = db.floor
    assert floor == 1 and keys.size > 9000
    want = ref.gc_spectrum(keys, counts, k)
    matrix = str(tmp_path / "gc.tsv")
    capsys.readouterr()
    gs.main([path, "--matrix", matrix])
    said = capsys.readouterr()
    assert said.out == "\n".join(gs.summary(want, (1, 255))) + "\n"
    assert np.array_equal(gs.read_matrix(matrix), want) and not os.path.exists(matrix + ".tmp")
    head = [line for line in open(matrix) if line.startswith("#")]
    assert path in head[1] and "k = 21; floor = 1; space = plain" in head[2]
    assert "{} plain 21-mers, floor 1".format(keys.size) in said.err and said.err.rstrip().endswith("No verdict is computed")
    lines = said.out.splitlines()
    assert len(lines) == 1 + (k + 1) + 1 and lines[-1].split("\t")[:2] == ["#total", str(keys.size)]
    assert sum(int(line.split("\t")[1]) for line in lines[1:-1]) == keys.size
    gs.main([path, "--min-count", "5", "--max-count", "90"])
    assert capsys.readouterr().out == "\n".join(gs.summary(want, (5, 90))) + "\n"
    # the solid form of the same library starts at its floor
    solid = str(tmp_path / "solid.tbkdb")
    with kmers.load_solid_database(path) as db:
        db.save(solid)
    gs.main([solid])
    said = capsys.readouterr()
    keep = counts >= 2
    assert said.out == "\n".join(gs.summary(ref.gc_spectrum(keys[keep], counts[keep], k), (2, 255))) + "\n" and "floor 2; counters 2..255" in said.err
    # carve by GC and counter
    picked = str(tmp_path / "picked.tbkdb")
    sd.main(["-o", picked, "--min-gc", "13", "--min-count", "20", path])
    err = capsys.readouterr().err
    kept = ref.select(keys, counts, (20, 255), (), sref.BASE, gc=(13, 32))
    assert kept[0].size and open(picked, "rb").read() == kf.file_bytes(k, *kept, reads=0, bases=0, magic=FULL)
    assert "{} of the {} k-mers of {} kept with 13..21 G-or-C bases".format(kept[0].size, keys.size, path) in err
    rest = str(tmp_path / "rest.tbkdb")
    sd.main(["-o", rest, "--max-gc", "14", "--exclude", picked, path])
    kept = ref.select(keys, counts, (1, 255), [(kept[0], kept[1], (1, 255), E)], sref.BASE, gc=(0, 14))
    assert kept[0].size and open(rest, "rb").read() == kf.file_bytes(k, *kept, reads=0, bases=0, magic=FULL)
    assert "with 0..14 G-or-C bases" in capsys.readouterr().err
