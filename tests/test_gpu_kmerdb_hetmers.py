"""The het-mer pairs of a count database on the device (include/tbk.h: tbk_kmerdb_hetmers), kmers.KmerDatabase.hetmers and the
hetmers command on top.  Crafted databases are files this test writes itself (tests/kmerdb_files.py through the helpers of the
table and union tests); every expectation is the brute-force reference's (tests/db_hetmer_ref.py) and every number and every
pair record must equal it exactly.

The kernels look every candidate's three middle variants up through a directory, as a set; the tally strides over tiles of 1024
entries and keeps a low-counter corner of the pair spectrum in LDS; the pairs come through the tile compaction.  So the shapes
aim at: every canonical k-mer of k = 1, 3 and 5, where variants that are the k-mer itself and variants that merge are dense;
planted classes of 2, 3 and 4 members among random keys at k = 21 and 31 (62-bit ranks), at sizes around a tile; counter
ranges that cut classes apart; counters 1, 2, 254, 255 and cells on both sides of any corner edge; partners given or not, empty,
the database itself; the later trips of the strided tally (tbk_count_set_grid_caps_); and every refusal.

Not covered here: the refusal of 2^32 or more entries is tested on an object that only CLAIMS that size (the importer's
tbk_kmerdb_make_ over two 16-byte arrays, which the refused call never reads) - a real one would be 38 GB."""
import ctypes as C

import numpy as np
import pytest

import db_hetmer_ref as ref
from test_gpu_kmerdb_table import TILE, _write_db
from test_gpu_kmerdb_union import _write_full

pytestmark = pytest.mark.gpu

FULL_HPC = b"TBKKMFH1"
FIELDS = ("minor", "major", "c_minor", "c_major", "cls_minor", "cls_major")
# (minor, major) counters planted on pairs: 1, 2, 254, 255, and both sides of the edge of a corner of 2, 64, 128 or 256
SPECIAL = ((1, 1), (1, 2), (2, 2), (2, 63), (63, 63), (63, 64), (64, 64), (64, 65), (100, 200), (127, 128), (128, 128), (2, 254), (254, 255),
           (255, 255), (1, 255), (30, 30))
RANGES = ((1, 255), (2, 255), (2, 40), (64, 255), (30, 30), (255, 255))


def _write(path, k, keys, counts, floor, **kw):
    keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint8)
    assert counts.size == 0 or int(counts.min()) >= floor
    return _write_full(path, k, keys, counts, **kw) if floor == 1 else _write_db(path, k, keys, counts)


def _arrays(entries):
    """{rank: counter} -> (ascending ranks, counters)"""
    keys = np.array(sorted(entries), dtype=np.uint64)
    return keys, np.array([entries[int(key)] for key in keys], dtype=np.uint8)


def _records(rec):
    return [tuple(int(rec[f][i]) for f in FIELDS) for i in range(rec.size)]


def _check(db, keys, counts, k, lo, hi, y=None, z=None, y_range=(1, 255), z_range=(1, 255), what=None):
    """The device's answer with and without the pairs against the reference; y, z: None or (database, {rank: counter})."""
    want = ref.hetmers(keys, counts, k, lo, hi, y=None if y is None else y[1], y_range=y_range, z=None if z is None else z[1], z_range=z_range)
    kw = dict(y=None if y is None else y[0], z=None if z is None else z[0], y_range=y_range, z_range=z_range)
    plain, full = db.hetmers(lo, hi, **kw), db.hetmers(lo, hi, pairs=True, **kw)
    assert "records" not in plain
    for got in (plain, full):
        ref.check_invariants(got)
        assert (got["candidates"], got["pairs"]) == (want["candidates"], want["pairs"]), (what, lo, hi)
        for name in ("partners", "spec", "origin"):
            assert got[name].dtype == np.uint64 and np.array_equal(got[name], want[name]), (what, lo, hi, name)
    assert _records(full["records"]) == want["records"], (what, lo, hi)
    assert not full["records"]["reserved"].any()
    lower = np.minimum(full["records"]["minor"], full["records"]["major"])
    assert np.all(lower[1:] > lower[:-1])  # ascending by the rank of the lower-ranked member
    return want


# ---- k = 1, 3, 5: every canonical k-mer, exhaustive and random ---------------------------------------------------------------------
def _variant_kinds(keys, k):
    kinds = [ref.variant_kinds(int(key), k) for key in keys]
    return sum(a for a, _ in kinds), sum(b for _, b in kinds)


@pytest.mark.parametrize("floor", [1, 2])
def test_k1_and_every_canonical_3mer(gpu, tmp_path, floor):
    from trio_binning_amd import kmers

    with kmers.KmerDatabase.load(_write(tmp_path / "k1.tbkdb", 1, [0, 1], [7, 3], floor)) as db:
        want = _check(db, [0, 1], [7, 3], 1, 1, 255)
        assert want["records"] == [(1, 0, 3, 7, 0, 0)]
        assert _check(db, [0, 1], [7, 3], 1, 4, 255)["pairs"] == 0
    keys = np.array([ref.rank_of(s) for s in ref.all_canonical(3)], dtype=np.uint64)
    assert keys.size == 32 and _variant_kinds(keys, 3) == (8, 8)  # AAT-like k-mers: a variant that is the k-mer itself, two that merge
    rng = np.random.default_rng(31 + floor)
    met = set()
    for trial in range(6):
        counts = rng.integers(floor, 256, keys.size).astype(np.uint8) if trial else np.full(keys.size, 9, dtype=np.uint8)
        with kmers.KmerDatabase.load(_write(tmp_path / "k3.tbkdb", 3, keys, counts, floor)) as db:
            for lo, hi in ((1, 255), (floor, 128), (100, 255), (9, 9)):
                want = _check(db, keys, counts, 3, lo, hi, what=("k3", trial))
                met |= {j for j in range(4) if want["partners"][j]}
    assert met == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", range(10))
def test_random_subsets_of_the_canonical_5mers(gpu, tmp_path, seed):
    from trio_binning_amd import kmers

    every = np.array([ref.rank_of(s) for s in ref.all_canonical(5)], dtype=np.uint64)
    assert every.size == 512
    rng = np.random.default_rng(500 + seed)
    floor = 1 + seed % 2
    keys = every[rng.random(every.size) < (0.3, 0.6, 0.9, 1.0)[seed % 4]]
    selfs, merged = _variant_kinds(keys, 5)
    assert selfs > 0 and merged > 0  # both kinds of variant that a blind triple lookup would miscount
    counts = rng.integers(floor, 256, keys.size).astype(np.uint8)
    counts[rng.random(keys.size) < 0.3] = 30
    with kmers.KmerDatabase.load(_write(tmp_path / "k5.tbkdb", 5, keys, counts, floor)) as db:
        pairs = 0
        for lo, hi in RANGES + ((1, 29), (31, 255)):  # (ranges that cut classes apart)
            pairs += _check(db, keys, counts, 5, lo, hi, what=("k5", seed))["pairs"]
        assert pairs > 0


# ---- k = 21 and 31: planted classes among random keys -----------------------------------------------------------------------------
def _random_canonical(rng, k):
    return ref.canonical_rank(int(rng.integers(0, 1 << 62)) & ((1 << (2 * k)) - 1), k)


def _mirror_class(rng, k):
    """the two members of a class with mirrored flanks: L A rc(L) and L C rc(L)"""
    m = (k - 1) // 2
    left = int(rng.integers(0, 1 << (2 * m))) if m else 0
    flanks = (left << (2 * m + 2)) | ref.revcomp_rank(left, m)
    members = [flanks | (b << (2 * m)) for b in (0, 1)]
    assert all(ref.canonical_rank(x, k) == x for x in members) and [p for p, *_ in ref.partner_ranks(members[0], k)] == [members[1]]
    return members


def _planted(rng, k, n, floor, classes, only_pairs=False):
    """{rank: counter} of exactly n entries: `classes` planted classes - mirrored ones whole, classes of four with 2, 3 or all 4
    of their members - then random canonical ranks.  Pairs get the SPECIAL counters, in either order of rank."""
    entries, special = {}, [p for p in SPECIAL if p[0] >= floor]
    for i in range(classes):
        if len(entries) >= n:
            break
        if i % 4 == 0:
            members = _mirror_class(rng, k)
        else:
            x = _random_canonical(rng, k)
            members = [x] + [p for p, *_ in ref.partner_ranks(x, k)]
            if len(members) != 4:
                continue
            keep = 2 if only_pairs else (2, 3, 4)[i % 3]
            members = [members[j] for j in rng.permutation(4)[:keep]]
        if len(entries) + len(members) > n or any(x in entries for x in members):
            continue
        if len(members) == 2:
            a, b = special[i % len(special)]
            cs = [a, b] if rng.random() < 0.5 else [b, a]
        else:
            cs = [int(c) for c in rng.integers(max(floor, 2), 60, len(members))]
        entries.update(zip(members, cs))
    while len(entries) < n:
        assert not only_pairs
        x = _random_canonical(rng, k)
        if x not in entries:
            entries[x] = int(rng.integers(max(floor, 2), 60)) if rng.random() < 0.9 else int(rng.integers(floor, 256))
    assert len(entries) == n
    return entries


def _orientations(want, k):
    """(pairs whose partner is a variant as it stands, pairs reached through a variant's reverse complement) among the pairs found"""
    kept = flipped = 0
    for minor, major, *_ in want["records"]:
        x, p = min(minor, major), max(minor, major)
        flags = {q: (a, b) for q, a, b in ref.partner_ranks(x, k)}[p]
        kept += flags[0]
        flipped += flags[1]
    return kept, flipped


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 5000])
def test_planted_classes_at_every_size(gpu, tmp_path, k, n):
    from trio_binning_amd import kmers

    floor = 1 + (n + k // 10) % 2  # (both floors at both k)
    rng = np.random.default_rng(1000 * k + n)
    entries = _planted(rng, k, n, floor, classes=n // 6)
    keys, counts = _arrays(entries)
    if k == 31 and n >= TILE - 1:
        assert int(keys[-1]) >> 56  # 62-bit ranks
    with kmers.KmerDatabase.load(_write(tmp_path / "db.tbkdb", k, keys, counts, floor)) as db:
        assert db.floor == floor
        before = db.entries()
        kept = flipped = 0
        cells = set()
        for lo, hi in RANGES:
            want = _check(db, keys, counts, k, lo, hi, what=(k, n))
            a, b = _orientations(want, k)
            kept, flipped = kept + a, flipped + b
            cells |= {(r[2], r[3]) for r in want["records"]}
        after = db.entries()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])  # the input is as it was
        if n >= TILE - 1:
            assert kept > 0 and flipped > 0
            assert cells >= {p for p in SPECIAL if p[0] >= floor}  # 1 or 2, 254, 255; inside and outside any corner
        if n == 5000:  # the tally's later trips: one block walks all five tiles, then two blocks take them in turns
            try:
                for cap in (1, 2):
                    assert gpu.lib.tbk_count_set_grid_caps_(0, cap) == 0
                    _check(db, keys, counts, k, floor, 255, what=("cap", cap))
                    _check(db, keys, counts, k, 2, 40, y=(db, entries), y_range=(2, 30), what=("cap", cap, "y"))
            finally:
                gpu.lib.tbk_count_set_grid_caps_(0, 0)


@pytest.mark.parametrize("k", [21, 31])
def test_no_pair_at_all_and_every_entry_in_a_pair(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(77 + k)
    lone = _planted(rng, k, TILE + 1, 2, classes=0)
    keys, counts = _arrays(lone)
    with kmers.KmerDatabase.load(_write(tmp_path / "lone.tbkdb", k, keys, counts, 2)) as db:
        want = _check(db, keys, counts, k, 1, 255)
        assert want["pairs"] == 0 and int(want["partners"][0]) == TILE + 1
    paired = _planted(rng, k, 2 * TILE, 1, classes=40 * TILE, only_pairs=True)
    keys, counts = _arrays(paired)
    with kmers.KmerDatabase.load(_write(tmp_path / "paired.tbkdb", k, keys, counts, 1)) as db:
        want = _check(db, keys, counts, k, 1, 255)
        assert want["pairs"] == TILE and int(want["partners"][1]) == 2 * TILE
        assert min(_orientations(want, k)) > 0


# ---- partner databases ------------------------------------------------------------------------------------------------------------
def test_partners_given_or_not_empty_or_the_database_itself(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(2121)
    entries = _planted(rng, k, TILE + 1, 1, classes=300)
    keys, counts = _arrays(entries)

    def partner(name, share, floor):
        held = {int(key): int(rng.integers(floor, 256)) for key in keys[rng.random(keys.size) < share]}
        for _ in range(200):
            held.setdefault(_random_canonical(rng, k), int(rng.integers(floor, 256)))
        path = _write(tmp_path / (name + ".tbkdb"), k, *_arrays(held), floor)
        return kmers.KmerDatabase.load(path), held

    empty = kmers.KmerDatabase.load(_write(tmp_path / "empty.tbkdb", k, [], [], 2)), {}
    y, z = partner("y", 0.5, 2), partner("z", 0.5, 1)
    with kmers.KmerDatabase.load(_write(tmp_path / "db.tbkdb", k, keys, counts, 1)) as db, y[0], z[0], empty[0]:
        me = (db, entries)
        seen = np.zeros((4, 4), dtype=np.uint64)
        for lo, hi in ((1, 255), (2, 60)):
            for kw in (dict(y=y), dict(z=z), dict(y=y, z=z), dict(y=z, z=y), dict(y=me), dict(y=me, z=me, z_range=(100, 255)),
                       dict(y=empty), dict(y=empty, z=empty), dict(y=y, z=empty),
                       dict(y=y, z=z, y_range=(128, 255), z_range=(1, 127)), dict(y=y, z=z, y_range=(255, 255), z_range=(1, 1))):
                want = _check(db, keys, counts, k, lo, hi, what=sorted(kw), **kw)
                if set(kw) >= {"y", "z"} and kw["y"] is y:
                    seen += want["origin"]
        assert np.count_nonzero(seen) == 16  # every combination of classes was on some pair
        # the per-pair classes against numpy: membership of the record's ranks in the partners' arrays
        got = db.hetmers(1, 255, y=y[0], z=z[0], y_range=(2, 200), z_range=(3, 255), pairs=True)["records"]
        for dbp, held, (lo, hi), bit in ((y[0], y[1], (2, 200), 1), (z[0], z[1], (3, 255), 2)):
            pk, pc = dbp.entries()
            for side in ("minor", "major"):
                at = np.minimum(np.searchsorted(pk, got[side]), pk.size - 1)
                inside = (pk[at] == got[side]) & (pc[at] >= lo) & (pc[at] <= hi)
                assert np.array_equal((got["cls_" + side] & bit) != 0, inside)


def test_compressed_databases_are_accepted_in_one_space(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(9)
    entries = _planted(rng, k, 700, 1, classes=150)
    keys, counts = _arrays(entries)
    with kmers.KmerDatabase.load(_write(tmp_path / "h.tbkdb", k, keys, counts, 1, magic=FULL_HPC)) as db, \
            kmers.KmerDatabase.load(_write(tmp_path / "p.tbkdb", k, keys, counts, 1)) as plain:
        assert db.compressed and not plain.compressed
        _check(db, keys, counts, k, 1, 255, y=(db, entries))
        with pytest.raises(ValueError, match="compressed"):
            db.hetmers(1, 255, y=plain)
        with pytest.raises(ValueError, match="compressed"):
            plain.hetmers(1, 255, z=db)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_inputs_and_no_pairs(gpu, tmp_path):
    from trio_binning_amd import _lib, kmers

    rng = np.random.default_rng(4)
    e21, e31 = _planted(rng, 21, 300, 2, classes=60), _planted(rng, 31, 100, 2, classes=20)
    even = np.array(sorted({int(v) for v in rng.integers(0, 1 << 40, 50)}), dtype=np.uint64)
    with kmers.KmerDatabase.load(_write(tmp_path / "a.tbkdb", 21, *_arrays(e21), 2)) as db, \
            kmers.KmerDatabase.load(_write(tmp_path / "b.tbkdb", 31, *_arrays(e31), 2)) as other, \
            kmers.KmerDatabase.load(_write(tmp_path / "c.tbkdb", 20, even, np.full(even.size, 5, dtype=np.uint8), 2)) as even_db:
        before = db.entries()
        with pytest.raises(ValueError, match="even.*middle base must be its own mirror under reverse complement"):
            even_db.hetmers(1, 255)
        for lo, hi in ((0, 255), (1, 256), (9, 8), (0, 0), (300, 400)):
            with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
                db.hetmers(lo, hi)
            with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
                db.hetmers(1, 255, y=db, y_range=(lo, hi))
            with pytest.raises(ValueError, match="1 <= min <= max <= 255"):
                db.hetmers(1, 255, z_range=(lo, hi))
        with pytest.raises(ValueError, match="different k"):
            db.hetmers(1, 255, y=other)
        with pytest.raises(ValueError, match="different k"):
            db.hetmers(1, 255, z=other, pairs=True)
        # the C call itself: the pairs pointer is NULL after an error, NULL arguments and a bad size are refused
        o, res, ptr = _lib.HetmerOptions(), _lib.HetmerResult(), C.c_void_p(12345)
        spec = np.zeros(256 * 256, dtype=np.uint64)
        _lib.lib.tbk_hetmer_options_init(C.byref(o))
        _lib.lib.tbk_hetmer_result_init(C.byref(res))
        assert (o.size, o.min_count, o.max_count, o.y_min, o.y_max, o.z_min, o.z_max, o.want_pairs) == (C.sizeof(o), 1, 255, 1, 255, 1, 255, 0)
        assert res.size == C.sizeof(res)
        o.want_pairs, o.min_count = 1, 0
        assert _lib.lib.tbk_kmerdb_hetmers(db._h, C.byref(o), C.byref(res), spec.ctypes.data, C.byref(ptr)) == -1 and ptr.value is None
        o.min_count = 1
        assert _lib.lib.tbk_kmerdb_hetmers(db._h, C.byref(o), C.byref(res), spec.ctypes.data, None) == -1  # pairs wanted, nowhere to put them
        assert _lib.lib.tbk_kmerdb_hetmers(None, C.byref(o), C.byref(res), spec.ctypes.data, C.byref(ptr)) == -1
        assert _lib.lib.tbk_kmerdb_hetmers(db._h, C.byref(o), C.byref(res), None, C.byref(ptr)) == -1
        o.size = 8
        assert _lib.lib.tbk_kmerdb_hetmers(db._h, C.byref(o), C.byref(res), spec.ctypes.data, C.byref(ptr)) == -1
        assert "tbk_hetmer_options_init" in _lib.last_error()
        assert _lib.lib.tbk_abi_version() == 1
        # 2^32 entries: an object that claims them over two small arrays, which the refused call never reads
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        d_keys, d_counts, big = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_keys), 16) == 0 and hip.hipMalloc(C.byref(d_counts), 16) == 0
        make = _lib.lib.tbk_kmerdb_make_
        make.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
        make.restype = C.c_int
        hist = np.zeros(256, dtype=np.uint64)
        for n in (1 << 32,):
            assert make(d_keys, d_counts, n, 21, db.device, 2, 0, hist.ctypes.data, 0, 0, C.byref(big)) == 0
            try:
                o.size, o.want_pairs = C.sizeof(o), 1
                ptr = C.c_void_p(1)
                assert _lib.lib.tbk_kmerdb_hetmers(big, C.byref(o), C.byref(res), spec.ctypes.data, C.byref(ptr)) == -1 and ptr.value is None
                assert "32-bit offsets" in _lib.last_error() and str(1 << 32) in _lib.last_error()
            finally:
                _lib.lib.tbk_kmerdb_destroy(big)  # (frees the two arrays)
        after = db.entries()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        _check(db, *_arrays(e21), 21, 2, 255)  # and it still answers


# ---- the command, end to end ----------------------------------------------------------------------------------------------------------
def test_hetmers_command_on_a_crafted_trio(gpu, tmp_path, capsys):
    from trio_binning_amd import hetmers as hm

    k = 21
    rng = np.random.default_rng(808)
    child = _planted(rng, k, 1500, 2, classes=260)
    keys, counts = _arrays(child)
    base = ref.hetmers(keys, counts, k, 2, 255)
    assert base["pairs"] > 100
    a, b = {}, {}
    for i, (minor, major, *_rest) in enumerate(base["records"]):  # every combination of classes on some pair
        for member, cls in ((minor, i % 4), (major, (i // 4) % 4)):
            if cls & 1:
                a[member] = 2 + i % 50
            if cls & 2:
                b[member] = 2 + i % 70
    for held in (a, b):
        for _ in range(300):
            held.setdefault(_random_canonical(rng, k), int(rng.integers(2, 90)))
    paths = {name: _write(tmp_path / (name + ".tbkdb"), k, *_arrays(entries), 2) for name, entries in (("child", child), ("A", a), ("B", b))}
    range_a, range_b = (2, 40), (3, 60)
    want = ref.hetmers(keys, counts, k, 2, 255, y=a, y_range=range_a, z=b, z_range=range_b)
    assert np.count_nonzero(want["origin"]) == 16
    matrix, pairs = tmp_path / "het.tsv", tmp_path / "pairs.tsv"
    hm.main([paths["child"], "--min-count", "2", "--max-count", "255", "--matrix", str(matrix), "--pairs", str(pairs), "--parent-a", paths["A"],
             "--parent-b", paths["B"], "--min-count-a", "2", "--max-count-a", "40", "--min-count-b", "3", "--max-count-b", "60"])
    out = dict(line.split("\t") for line in capsys.readouterr().out.splitlines())
    n_pairs, cand = want["pairs"], want["candidates"]
    assert out["k"] == "21" and out["space"] == "plain" and out["range"] == "2,255" and out["range_a"] == "2,40" and out["range_b"] == "3,60"
    assert int(out["candidates"]) == cand and int(out["pairs"]) == n_pairs
    assert [int(out["candidates_with_{}_partners".format(j)]) for j in range(4)] == [int(v) for v in want["partners"]]
    assert out["candidates_in_pairs_share"] == "{:.6f}".format(2 * n_pairs / cand)
    for i in range(4):
        for j in range(4):
            assert int(out["pairs_minor_{}_major_{}".format(hm.CLASSES[i], hm.CLASSES[j])]) == int(want["origin"][i, j])
    split = int(want["origin"][1, 2] + want["origin"][2, 1])
    inside = int(want["origin"][1, 1] + want["origin"][2, 2])
    orphan = sum(1 for r in want["records"] if r[4] == 0 or r[5] == 0)
    assert (int(out["pairs_split_between_parents"]), int(out["pairs_inside_one_parent"]), int(out["pairs_with_a_member_in_neither"])) == (split, inside, orphan)
    assert out["pairs_split_between_parents_share"] == "{:.6f}".format(split / n_pairs)
    assert out["pairs_inside_one_parent_share"] == "{:.6f}".format(inside / n_pairs)
    assert out["pairs_with_a_member_in_neither_share"] == "{:.6f}".format(orphan / n_pairs)
    assert np.array_equal(hm.read_matrix(str(matrix)), want["spec"])
    assert open(matrix).readline().startswith("#") and "k = 21" in open(matrix).readline() and "2,255" in open(matrix).readline()
    lines = [line.rstrip("\n").split("\t") for line in open(pairs)]
    assert lines == [[ref.kmer_of(r[0], k), str(r[2]), ref.kmer_of(r[1], k), str(r[3]), hm.CLASSES[r[4]], hm.CLASSES[r[5]]] for r in want["records"]]
    assert not (tmp_path / "het.tsv.tmp").exists() and not (tmp_path / "pairs.tsv.tmp").exists()
    # without parents: four columns, no origin lines
    hm.main([paths["child"], "--min-count", "10", "--max-count", "50", "--pairs", str(pairs)])
    out = dict(line.split("\t") for line in capsys.readouterr().out.splitlines())
    alone = ref.hetmers(keys, counts, k, 10, 50)
    assert int(out["pairs"]) == alone["pairs"] and not any(name.startswith("pairs_minor_") for name in out)
    assert hm.read_pairs(str(pairs)) == [(ref.kmer_of(r[0], k), r[2], ref.kmer_of(r[1], k), r[3]) for r in alone["records"]]
