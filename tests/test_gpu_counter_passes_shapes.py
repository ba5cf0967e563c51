"""The k-mer counter in passes and the count databases at the shapes tests/test_gpu_counter_passes.py and tests/test_gpu_kmerdb.py do
not reach: every class-selecting instantiation of the counting kernel, a retained store of several segments, grids that go round
their grid-stride loop twice, a database saved and loaded in two pieces, the store limit to the word, batches that lie on the device.
The yardstick is oracle/unique_oracle.py's numpy counter and the files tests/kmerdb_files.py writes; every comparison is exact.

  test_every_pass_kernel_against_the_oracle     B1  one (k, W, m) per instantiation, tables rebuilt in class 0 AND in a replayed class
  test_boundaries_on_the_64_bit_path            B2  the boundary reads of test_batch_and_chunk_boundaries under W = 4 / 3, m = 17
  test_library_past_every_size_edge_in_passes   B3  > 4,194,304 kept k-mers: store segments, element grids, table grids, file pieces
  test_library_past_every_size_edge_in_one_pass B3  the same reads through one-pass counters: export and unique kernels past their grids
  test_store_limit_to_the_word                  B4  N batches that pack to exactly the limit; 8 bytes less refuses the last
  test_add_device_in_passes                     B5  tbk_counter_add_device with passes = 3
  (B6, several pieces in passes, is test_multi_piece_add_in_passes beside test_multi_piece_add in tests/test_gpu_counter_shapes.py)

The edges, and what puts an input past them (each test asserts its own):
  2^17 words       the first segment of the retained store (store_append): 2,097,152 positions of the separated stream
  1,048,576 slots  one round of the distil and export grids (4096 x 256)
  2,097,152        one round of the db_unique / db_rank / kmerdb_unique grids, and of tbk_count_unique_kernel's (8192 x 256)
  4,194,304 k-mers one piece of tbk_kmerdb_save / _load (keys, then counters)

Libraries with one error each (variant libraries chosen with TBK_LIBRARY, never committed), and the test that is there for each.
NOT RUN YET: neither this file nor the variants have been on an MI355X (profiles/r08/README.md); the table is what each test was
built to notice, from reading tbk_count.cpp and tbk_count_kernels.hip, and what the two older files cannot notice by their shapes.
  1 tbk_launch_count_class launches the 32-bit instantiation when m > 16      the 64-bit cases of test_every_pass_kernel (a key the
      rehash placed by tbk_bucket_of is counted again in another bucket), test_boundaries_on_the_64_bit_path,
      test_multi_piece_add_in_passes; the older files never run a table with m > 16
  2 counter_finish replays every piece from segment 0 (where the piece fits its capacity; a variant that read past segment 0
      is not built)      test_library_past_every_size_edge_in_passes (the read of 300 bases in segment 2), test_store_limit_to_the_word
      (the second batch opens segment 1); the older files keep every store in one segment
  3 tbk_count_distil_kernel's loop body runs once (`if` for `for`)      every table of more than 1,048,576 slots with k-mers to
      keep: both tests of B3's passes half, test_store_limit_to_the_word, test_multi_piece_add_in_passes.  Slots past the grid
      also stay occupied for the next class, so test_table_of_a_class_is_smaller of the older file may notice it as well
  4 the same in tbk_db_unique_kernel      test_library_past_every_size_edge_in_passes alone (a class of more than 2,097,152 k-mers)
  5 tbk_kmerdb_save writes the counters of every piece from d_counts + 0      test_library_past_every_size_edge_in_passes and
      _in_one_pass: the file differs from kmerdb_files.file_bytes where a counter of the second piece is not that of the first
      piece at the same offset (285 k-mers of A have a counter other than 2)
  6 store_append compares >= for > against the limit      test_store_limit_to_the_word[exact]: the third batch is refused
  7 word() in the pass kernel returns 0 past the store instead of sixteen not-ACGT positions      EQUIVALENT: a window counts only
      if start + k <= total, and total is 16 x the store's words, so no counted window reads a position past the store - as the
      header of test_gpu_counter_shapes.py found for load_chunk in the one-pass kernel.  No test can notice it.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kmerdb_files as kf
from oracle import unique_oracle as uo
from test_gpu_counter_passes import _boundary_reads
from test_gpu_counter_shapes import _M32, _M64, _PARTNERS, _Pinned, _compare, _expect, _rc, _stress_reads, _two_parent_reads

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NONE = (np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64))
_SEGMENT = 1 << 17  # words of the store's first segment


def _pack(arrays):
    """(bases, offsets) of reads given as uint8 arrays."""
    offsets = np.zeros(len(arrays) + 1, dtype=np.uint64)
    np.cumsum([a.size for a in arrays], out=offsets[1:])
    return (np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.uint8)), offsets


def _words(arrays):
    """64-bit words a batch takes in the retained store: 16 positions of the separated stream (every read and its 'N') each."""
    return (sum(a.size for a in arrays) + len(arrays) + 15) // 16


def _segment_caps(batch_words, limit_bytes=0):
    """Capacities (words) of the store's segments after batches of these sizes, by store_append's rule: a batch lies in one segment;
    a new segment holds the batch, 2^17 words or half of what is kept, whichever is most - but, under a limit, no more than the
    limit leaves (and still the batch)."""
    caps, free, kept = [], 0, 0
    for w in batch_words:
        if not caps or free < w:
            cap = max(w, _SEGMENT, kept // 2)
            if limit_bytes:
                cap = max(w, min(cap, limit_bytes // 8 - kept))
            caps.append(cap)
            free = cap
        free -= w
        kept += w
    return caps


def _read_keys(counter, other, lo, hi, path, k):
    n = counter.unique(other, lo, hi, str(path))
    got = uo.read_list_np(str(path), k)
    os.unlink(path)
    assert n == got.size
    return got


# ---- B1. every class-selecting instantiation --------------------------------------------------------------------------------
_U32 = np.uint64(0xFFFFFFFF)


def _class_of(key, n_classes):
    """tbk_class_of (tbk_common.h) of an array of keys in the table's form (base 0 in the low bits, the smaller strand)."""
    key = key.astype(np.uint64)
    lo, hi = key & _U32, key >> np.uint64(32)
    h = ((lo ^ np.uint64(0x2545F491)) * np.uint64(0xCC9E2D51) + (hi ^ np.uint64(0x68E31DA4)) * np.uint64(0x1B873593)) & _U32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & _U32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & _U32
    h ^= h >> np.uint64(16)
    return (h * np.uint64(n_classes)) >> np.uint64(32)


@functools.lru_cache(maxsize=None)
def _reads_outside_class_0(k, passes, n_reads=2048, length=200):
    """Random reads grown base by base, each base chosen (where one of the four allows it) so that the window it completes is a
    k-mer of another class than 0: class 0 gets next to none of their 350,000-odd distinct k-mers, the other classes share them.
    With these among A's reads a later class holds several times the k-mers of class 0, so the table that sufficed for class 0
    has to be rebuilt while that class is replayed."""
    rng = np.random.default_rng(70_000 + 64 * k + passes)
    mask = np.uint64((1 << (2 * k)) - 1)
    top = np.uint64(2 * (k - 1))
    codes = np.zeros((n_reads, length), dtype=np.uint8)
    fwd = np.zeros(n_reads, dtype=np.uint64)
    rc = np.zeros(n_reads, dtype=np.uint64)
    for j in range(length):
        start = rng.integers(0, 4, n_reads).astype(np.uint64)
        todo = np.ones(n_reads, dtype=bool)
        nf, nr = fwd.copy(), rc.copy()
        for step in range(4):
            c = (start + np.uint64(step)) & np.uint64(3)
            f = (fwd >> np.uint64(2)) | (c << top)
            r = ((rc << np.uint64(2)) | (np.uint64(3) - c)) & mask
            take = todo & ((_class_of(np.minimum(f, r), passes) != 0) | (j < k - 1) | (step == 3))
            nf[take], nr[take], codes[take, j] = f[take], r[take], c[take]
            todo &= ~take
        fwd, rc = nf, nr
    return tuple(row.tobytes().decode() for row in _ACGT[codes])


# one (k, W, m) per instantiation, from the matrix of test_every_kernel_against_the_oracle: W = 1 .. 8 with 32-bit m-mers, W = 1 .. 8
# with 64-bit m-mers - m = 16 beside m = 17 at k = 21, 22 and 32 -, plain mode, and m = 4, where keys leave their home bucket
_PASS32 = [(15, 1, 15), (19, 2, 12), (19, 3, 15), (21, 4, 16), (22, 5, 16), (32, 6, 15), (32, 7, 16), (27, 8, 12)]
_PASS64 = [(32, 1, 32), (27, 2, 20), (21, 3, 17), (22, 4, 17), (31, 5, 25), (32, 6, 17), (31, 7, 17), (31, 8, 24)]
_PASS_MATRIX = [(k, w, m, _expect(k, w, m)) for k, w, m in _PASS32 + _PASS64 + [(21, 6, 4)]] + [(21, 0, None, (0, 0, 0))]
assert set(_PASS32) <= set(_M32) and set(_PASS64) <= set(_M64) and (21, 6, 4) in _M32
assert [w for _, w, _ in _PASS32] == list(range(1, 9)) == [w for _, w, _ in _PASS64]
assert {(k, m) for k, _, m in _PASS32 + _PASS64} >= {(k, m) for k in (21, 22, 32) for m in (16, 17)}


@pytest.mark.parametrize("i,k,w,m,expect", [(i,) + c for i, c in enumerate(_PASS_MATRIX)], ids=[f"k{k}-W{w}-m{m or 0}" for k, w, m, _ in _PASS_MATRIX])
def test_every_pass_kernel_against_the_oracle(gpu, tmp_path, monkeypatch, i, k, w, m, expect):
    """tbk_count_kernel<W, M64, TbkClassSel> at every W and either m-mer width, in 2, 3 or 7 passes: the library and the stress
    reads of test_every_kernel_against_the_oracle plus _reads_outside_class_0, A in batches of 50 reads from a table of a few
    hundred slots, B pinned like A in every fourth case and otherwise to plain mode, a 32-bit or a 64-bit selection.

    The counting kernel places a key by its rolled minimizer, tbk_count_rehash_kernel by tbk_bucket_of: only a rebuild shows a
    disagreement (a k-mer's count split over two slots).  So A's table must be rebuilt while class 0 is counted from the arriving
    batches and again while a later class is replayed from the store; the table's size before finish() against the first
    table's, and the largest table ever held against that, show both.  (Why the second holds: after class 0 the table's 0.85 is
    below twice the most class 0 ever needed, slots taken plus the window starts of a batch - some 20,000 to 50,000 with batches
    of 50 reads; class 1 ends with 60,000 to 360,000 k-mers.  The growth rule of count_stream, walked through on the CPU with the
    oracle's k-mers of every batch, rebuilds the table one to three times in class 0 and two or three times in class 1 in all
    18 cases.)"""
    passes = (2, 3, 7)[i % 3]
    rng = np.random.default_rng(9500 + i)
    tiny = m is not None and m <= 8
    reads_a, reads_b = _two_parent_reads(rng, 8000, 900, 700)
    stress = _stress_reads(rng, k)
    reads_a += stress + ["", "ACGT", "N" * 40, stress[6], stress[6].lower(), _rc(stress[6])] + list(_reads_outside_class_0(k, passes))
    reads_b += ["A" * 100, "AAT" * 30, stress[6], _rc(stress[7]), stress[8], stress[8]]
    reads_a = [reads_a[j] for j in rng.permutation(len(reads_a))]
    bw, bm = (w, m) if i % 4 == 0 else _PARTNERS[k][i % 3]
    cap_a, load = (16, 0.9) if tiny else ((1000, 16)[i % 2] * passes, None)
    with _Pinned(monkeypatch, k, cap_a, w, m, load, expect, passes=passes) as ca, \
            _Pinned(monkeypatch, k, 200_000, bw, bm, None, expect if i % 4 == 0 else _expect(k, bw, bm), passes=passes) as cb:
        first = ca.stats()["table_bytes"]
        for j in range(0, len(reads_a), 50):
            ca.add(reads_a[j:j + 50])
        cb.add(reads_b)
        arrived = ca.stats()
        assert first < arrived["table_bytes"] == arrived["peak_table_bytes"], "the table was not rebuilt while class 0 was counted"
        assert ca.finish()["peak_table_bytes"] > arrived["table_bytes"], "the table was not rebuilt while a later class was replayed"
        oa, ob = uo.count_kmers_np(*uo.pack(reads_a), k), uo.count_kmers_np(*uo.pack(reads_b), k)
        assert oa[1].max() >= 200 and (oa[1] == 1).sum() > 1000
        _compare(ca, cb, oa, ob, k, tmp_path, ((2, 255), (3, 9), (1, 4), (200, 255)))
        _compare(cb, ca, ob, oa, k, tmp_path, ((2, 255), (4, 6)))


# ---- B2. boundaries on the 64-bit path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w,m", [(32, 4, 17), (21, 3, 17)], ids=["k32-W4-m17", "k21-W3-m17"])
def test_boundaries_on_the_64_bit_path(gpu, tmp_path, monkeypatch, k, w, m):
    """The reads of test_batch_and_chunk_boundaries - one read per batch, the stream ending on, before and after a 16-base word of
    the store and a 2048-window pass - through the 64-bit class-selecting kernels."""
    reads = _boundary_reads()
    oa = uo.count_kmers_np(*uo.pack(reads), k)
    assert oa[1].max() < 255 and (uo.histogram_np(oa[1])[2:255] > 0).sum() > 3  # the counts are told apart, none saturates
    expect = _expect(k, w, m)
    with _Pinned(monkeypatch, k, 4000, w, m, None, expect, passes=2) as c, _Pinned(monkeypatch, k, 16, w, m, None, expect, passes=2) as empty:
        for r in reads:
            c.add([r])
        _compare(c, empty, oa, _NONE, k, tmp_path, ((2, 255), (int(oa[1].max()), 255), (2, int(np.median(oa[1])))))


# ---- B3. one library past every size edge -------------------------------------------------------------------------------------
_CUTS = ((0, 100), (100, 200), (200, 450), (450, 451), (451, 881))  # A's batches, as ranges of its reads


@functools.lru_cache(maxsize=None)
def _big():
    """A: a random genome of 4.4 Mbases at k = 21 in 440 pieces of 10 kb that overlap by k - 1, every piece twice, and one read of
    300 bases (read 450) that is a batch of its own; B: the first half of A's pieces, twice.  Every 21-mer of the genome is seen
    at least twice, so A keeps more than 4,194,304 k-mers - asserted here, from the oracle alone."""
    k = 21
    g = _ACGT[np.random.default_rng(4400).integers(0, 4, 4_400_000)]
    pieces = [g[at:at + 10_000 + k - 1] for at in range(0, g.size, 10_000)]
    reads_a = pieces * 2
    reads_a.insert(450, g[5:305])
    reads_b = pieces[:220] * 2
    a, b = _pack(reads_a), _pack(reads_b)
    oa, ob = uo.count_kmers_np(*a, k), uo.count_kmers_np(*b, k)
    keys, counts, hist = kf.database_of(*oa)
    assert keys.size > 4_194_304
    file_a = kf.file_bytes(k, keys, counts, hist, reads=len(reads_a), bases=int(a[1][-1]))
    return {"k": k, "reads_a": reads_a, "b": b, "oa": oa, "ob": ob, "db_a": (keys, counts, hist), "file_a": file_a}


@functools.lru_cache(maxsize=None)
def _big_unique(a_minus_b, lo, hi):
    big = _big()
    return uo.unique_np(big["oa"], big["ob"], lo, hi) if a_minus_b else uo.unique_np(big["ob"], big["oa"], lo, hi)


def _add_big(ca, cb):
    big = _big()
    for lo, hi in _CUTS:
        ca.add(*_pack(big["reads_a"][lo:hi]))
    cb.add(*big["b"])


def test_library_past_every_size_edge_in_passes(gpu, tmp_path):
    """A in 2 passes from a capacity of 100,000 k-mers, in five batches of 1.0, 1.0, 2.5, 0.0003 and 4.3 M positions.

    2^17 words: the third batch (more than 2,097,152 positions) does not fit what the first segment has left and is larger than a
    default segment, so its segment is made to measure (cap = words); the read of 300 bases after it finds that segment full and
    opens a third, the last batch a fourth: pieces of segments 1, 2 and 3 are replayed for class 1.  store_bytes is what
    store_append's rule gives for these batches.
    2,097,152 elements: A keeps more than 4,194,304 k-mers (asserted in _big), so one of its two classes holds more than 2,097,152
    and tbk_db_unique_kernel and tbk_db_rank_kernel go round their grids twice, whatever the class hash does.
    1,048,576 slots: the table holds more than 2 M k-mers of a class, so distil goes round its grid several times with k-mers to keep.
    4,194,304 k-mers: the database is saved, loaded and saved again in two pieces; tbk_kmerdb_unique_kernel goes round twice."""
    from trio_binning_amd import kmers

    big = _big()
    k = big["k"]
    want_keys, want_counts, want_hist = big["db_a"]
    pa, pb, pa2 = tmp_path / "a.tbkdb", tmp_path / "b.tbkdb", tmp_path / "a2.tbkdb"
    with kmers.KmerCounter(k, 100_000, passes=2) as ca, kmers.KmerCounter(k, 100_000, passes=2) as cb:
        _add_big(ca, cb)
        words = [_words(big["reads_a"][lo:hi]) for lo, hi in _CUTS]
        caps = _segment_caps(words)
        assert words[2] * 16 > 2_097_152 and words[2] > _SEGMENT and len(caps) == 4 and caps[1] == words[2]
        st = ca.stats()
        assert st["store_used_bytes"] == 8 * sum(words) and st["store_bytes"] == 8 * sum(caps)
        assert st["n_slots"] > 1_048_576 and st["reads_added"] == 881
        assert ca.histogram().tolist() == uo.histogram_np(big["oa"][1]).tolist()
        for lo, hi in ((2, 255), (3, 255)):
            assert np.array_equal(_read_keys(ca, cb, lo, hi, tmp_path / "ab.txt", k), _big_unique(True, lo, hi))
            assert np.array_equal(_read_keys(cb, ca, lo, hi, tmp_path / "ba.txt", k), _big_unique(False, lo, hi))
        assert _big_unique(True, 2, 255).size > 2_097_152 and 0 < _big_unique(True, 3, 255).size < 1000
        with ca.database() as da, cb.database() as db:
            assert len(da) == want_keys.size
            keys, counts = da.entries()
            assert np.array_equal(keys, want_keys) and np.array_equal(counts, want_counts) and da.histogram().tolist() == want_hist.tolist()
            da.save(str(pa))
            db.save(str(pb))
    assert pa.read_bytes() == big["file_a"]
    with kmers.KmerDatabase.load(str(pa)) as da, kmers.KmerDatabase.load(str(pb)) as db:
        da.save(str(pa2))
        assert pa2.read_bytes() == big["file_a"]
        for a_minus_b, x, y in ((True, da, db), (False, db, da)):
            assert np.array_equal(_read_keys(x, y, 2, 255, tmp_path / "u.txt", k), _big_unique(a_minus_b, 2, 255))
        assert np.array_equal(_read_keys(da, db, 3, 255, tmp_path / "u.txt", k), _big_unique(True, 3, 255))


def test_library_past_every_size_edge_in_one_pass(gpu, tmp_path):
    """The same reads through one-pass counters: the same file and the same lists.  The table of 4.4 M k-mers has more than
    2,097,152 slots, so tbk_count_export_kernel (4096 x 256) and tbk_count_unique_kernel (8192 x 256) go round their grids."""
    from trio_binning_amd import kmers

    big = _big()
    k = big["k"]
    with kmers.KmerCounter(k, 100_000) as ca, kmers.KmerCounter(k, 100_000) as cb:
        _add_big(ca, cb)
        assert ca.stats()["n_slots"] > 2_097_152
        assert ca.histogram().tolist() == uo.histogram_np(big["oa"][1]).tolist()
        assert np.array_equal(_read_keys(ca, cb, 2, 255, tmp_path / "ab.txt", k), _big_unique(True, 2, 255))
        assert np.array_equal(_read_keys(ca, cb, 3, 255, tmp_path / "ab.txt", k), _big_unique(True, 3, 255))
        assert np.array_equal(_read_keys(cb, ca, 2, 255, tmp_path / "ba.txt", k), _big_unique(False, 2, 255))
        with ca.database() as da:
            da.save(str(tmp_path / "a.tbkdb"))
    assert (tmp_path / "a.tbkdb").read_bytes() == big["file_a"]


# ---- B4. the store limit to the word ------------------------------------------------------------------------------------------
_LIMIT_WORDS = (100_000, 40_000, 30_000)


@functools.lru_cache(maxsize=None)
def _limit_batches():
    """Three batches of three reads that pack to 100,000, 40,000 and 30,000 words (each ends 5 positions short of its last word).
    The second and the third repeat sequence of the first, so every batch changes the counts of k-mers the others hold."""
    seq = _ACGT[np.random.default_rng(44).integers(0, 4, 16 * _LIMIT_WORDS[0])]
    batches = []
    for i, words in enumerate(_LIMIT_WORDS):
        total = 16 * words - 5 - 3  # bases: the separated stream has one more position per read
        at = 1000 * i
        cut = (at, at + total // 3, at + total // 2, at + total)
        batches.append([seq[cut[j]:cut[j + 1]] for j in range(3)])
        assert _words(batches[-1]) == words
    return batches


@pytest.mark.parametrize("short", [0, 8], ids=["exact", "8-bytes-less"])
def test_store_limit_to_the_word(gpu, tmp_path, short):
    """store_limit of exactly the 1,360,000 bytes three batches pack to: all three are accepted.  8 bytes less: the third is
    refused with TBK_ERR_NOMEM, and finish(), the histogram and a dump are the oracle's for the first two.  The second batch does
    not fit what the first left of the first segment (2^17 words), so it opens a second one, which the limit trims (70,000 words
    for 131,072): the third batch fills it to the last word."""
    from trio_binning_amd import kmers

    k = 21
    batches = _limit_batches()
    limit = 8 * sum(_LIMIT_WORDS) - short
    caps = _segment_caps(_LIMIT_WORDS[:3 - bool(short)], limit)
    assert len(caps) == 2 and caps[0] == _SEGMENT and _LIMIT_WORDS[1] <= caps[1] == limit // 8 - _LIMIT_WORDS[0] < _SEGMENT
    with kmers.KmerCounter(k, 100_000, passes=2, store_limit=limit) as c, kmers.KmerCounter(k, 16, passes=2) as empty:
        c.add(*_pack(batches[0]))
        c.add(*_pack(batches[1]))
        accepted = batches[0] + batches[1]
        bases, offsets = _pack(batches[2])
        if short:
            for _ in range(2):
                rc = gpu.lib.tbk_counter_add_batch(c._h, bases.ctypes.data, offsets.ctypes.data, 3)
                assert rc == gpu.TBK_ERR_NOMEM and "{} bases are retained".format(sum(a.size for a in accepted)) in gpu.last_error()
            with pytest.raises(MemoryError, match="bases are retained"):
                c.add(bases, offsets)
        else:
            c.add(bases, offsets)
            accepted = accepted + batches[2]
        st = c.stats()
        assert st["store_used_bytes"] == 8 * sum(_LIMIT_WORDS[:3 - bool(short)]) <= limit and st["store_bytes"] == 8 * sum(caps)
        assert st["bases_added"] == sum(a.size for a in accepted) and st["reads_added"] == len(accepted)
        c.finish()
        oa = uo.count_kmers_np(*_pack(accepted), k)
        assert (oa[1] >= 2).sum() > 500_000 and c.stats()["distinct"] == oa[0].size
        assert c.histogram().tolist() == uo.histogram_np(oa[1]).tolist()
        for lo, hi in ((2, 255), (3, 3)):
            assert np.array_equal(_read_keys(c, empty, lo, hi, tmp_path / "u.txt", k), uo.unique_np(oa, _NONE, lo, hi))


# ---- B5. batches that lie on the device ---------------------------------------------------------------------------------------
def test_add_device_in_passes(gpu, tmp_path):
    """tbk_counter_add_device with passes = 3: two batches copied to the device by the caller are retained and counted like
    batches that come from the host - equal to the oracle, and to add() of the same bytes."""
    from trio_binning_amd import kmers

    k, dev = 21, kmers.default_device()
    rng = np.random.default_rng(55)
    reads_a, reads_b = _two_parent_reads(rng, 8000, 600, 300)
    reads_a += _stress_reads(rng, k)
    halves = [uo.pack(reads_a[:333]), uo.pack(reads_a[333:])]
    held = []
    with kmers.KmerCounter(k, 3000, passes=3) as cd, kmers.KmerCounter(k, 3000, passes=3) as ch, kmers.KmerCounter(k, 100_000, passes=3) as cb:
        try:
            for bases, offsets in halves:
                ptrs = []
                for arr in (bases, offsets):
                    p = C.c_void_p()
                    gpu.check(gpu.lib.tbk_device_alloc(dev, max(16, arr.nbytes), C.byref(p)))
                    held.append(p)
                    gpu.check(gpu.lib.tbk_memcpy_h2d(dev, p, arr.ctypes.data, arr.nbytes))
                    ptrs.append(p.value)
                cd.add_device(ptrs[0], ptrs[1], offsets.size - 1, int(offsets[-1]))
                ch.add(bases, offsets)
        finally:
            for p in held:
                gpu.check(gpu.lib.tbk_device_free(dev, p))
        cb.add_reads(reads_b)
        sd, sh = cd.stats(), ch.stats()
        assert sd["store_used_bytes"] == sh["store_used_bytes"] > 0 and sd["bases_added"] == sh["bases_added"] == sum(map(len, reads_a))
        oa, ob = uo.count_kmers_np(*uo.pack(reads_a), k), uo.count_kmers_np(*uo.pack(reads_b), k)
        want_hist = uo.histogram_np(oa[1]).tolist()
        assert cd.histogram().tolist() == want_hist and ch.histogram().tolist() == want_hist and cd.stats()["distinct"] == oa[0].size
        for lo, hi in ((2, 255), (3, 9), (1, 4)):
            want = uo.unique_np(oa, ob, lo, hi)
            assert np.array_equal(_read_keys(cd, cb, lo, hi, tmp_path / "d.txt", k), want)
            assert np.array_equal(_read_keys(ch, cb, lo, hi, tmp_path / "h.txt", k), want)
        assert np.array_equal(_read_keys(cb, cd, 2, 255, tmp_path / "b.txt", k), uo.unique_np(ob, oa, 2, 255))
        assert uo.unique_np(oa, ob, 2, 255).size > 100
