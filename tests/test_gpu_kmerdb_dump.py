"""Counted k-mer dumps on the device (include/tbk.h): tbk_kmerdb_import_text and tbk_kmerdb_dump_text against tests/dump_ref.py,
which tests/test_host_dump_ref.py holds to the oracle's counter.

The shapes are the smallest at which each piece can go wrong: every k whose rank fills another part of the 64 bits (1, 2, 15,
21, 31, 32 with bit 63 set), line starts on every offset of a 16-byte vector, a wave and a 4096-byte tile (counters of 1 to 4
digits at random), windows of 4096, 4097 and 65536 bytes and the default, damage in one tile, in two tiles and in two windows,
keys in order (no sort may run), shuffled, on either strand and on both, runs of equal keys that saturate."""
import os

import numpy as np
import pytest

import dump_ref as ref
import hpc_ref
import kmerdb_files as kf
from oracle import unique_oracle as uo
from test_host_dump_ref import _reads

pytestmark = pytest.mark.gpu


def _write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return str(path)


def _saved(db, tmp_path, name="got.tbkdb"):
    path = str(tmp_path / name)
    db.save(path)
    with open(path, "rb") as fh:
        return fh.read()


def _imported(gpu, tmp_path, texts, **kw):
    """the *.tbkdb bytes of the database the texts (one per file) make"""
    from trio_binning_amd import kmers

    paths = [_write(tmp_path, "in{}.txt".format(i), t) for i, t in enumerate(texts)]
    with kmers.KmerDatabase.from_dump(paths, **kw) as db:
        return _saved(db, tmp_path)


def _refused(gpu, tmp_path, text, k, line_no, reason, **kw):
    from trio_binning_amd import kmers

    with pytest.raises(ref.DumpError) as want:
        ref.parse(text, k, kw.get("compressed", False))
    assert (want.value.line_no, want.value.reason) == (line_no, reason), "the test's own expectation"
    path = _write(tmp_path, "bad.txt", text)
    with pytest.raises(ValueError) as exc:
        kmers.KmerDatabase.from_dump(path, k=k, **kw)
    assert "{}: line {}: ".format(path, line_no) in str(exc.value) and reason in str(exc.value), str(exc.value)


def _random_kmers(rng, n, k):
    """n distinct canonical k-mers as ascending ranks"""
    top = 1 << (2 * k)
    keys = set()
    while len(keys) < n:
        for s in uo.kmer_strings(np.array([int(x) for x in rng.integers(0, min(top, 1 << 63), n, dtype=np.uint64)], dtype=np.uint64), k):
            keys.add(ref.rank(uo.canonical(s)))
    return np.array(sorted(keys)[:n], dtype=np.uint64)


def _text(keys, counts, k, sep="\t"):
    return "".join("{}{}{}\n".format(s, sep, c) for s, c in zip(uo.kmer_strings(keys, k), counts)).encode()


# ---- 1. round trip against the counter -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 15, 21, 31, 32])
def test_round_trip_against_the_counter(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(700 + k)
    reads = _reads(rng) + ["T" * 70, "TA" * 40, "GC" * 40, "TGCA" * 20]
    keys, counts = uo.count_kmers_np(*uo.pack(reads), k)
    capped = np.minimum(counts, 255)
    assert capped.max() == 255 and keys[0] == 0  # (A...A, which T...T is too)
    if k == 32:
        assert (keys >> np.uint64(63)).any(), "a rank with bit 63 set"
    with kmers.KmerCounter(k, 1 << 16, keep_singletons=True) as counter:
        counter.add_reads(reads)
        with counter.database() as full:
            st = full.stats()
            full_bytes = _saved(full, tmp_path, "full.tbkdb")
            dump = str(tmp_path / "full.txt")
            assert full.dump(dump, min_count=1) == keys.size
    with open(dump, "rb") as fh:
        text = fh.read()
    assert text == ref.format(keys, capped, k)
    with kmers.KmerDatabase.from_dump(dump, floor=1, reads=st["reads_added"], bases=st["bases_added"]) as back:
        assert (back.k, back.floor, len(back)) == (k, 1, keys.size)
        assert _saved(back, tmp_path) == full_bytes
    with kmers.KmerCounter(k, 1 << 16) as counter:
        counter.add_reads(reads)
        with counter.database() as solid:
            solid_bytes = _saved(solid, tmp_path, "solid.tbkdb")
    with kmers.KmerDatabase.from_dump([dump], k=k, floor=2, reads=st["reads_added"], bases=st["bases_added"]) as back:
        assert back.floor == 2
        assert _saved(back, tmp_path) == solid_bytes


# ---- 2. order and strands ----------------------------------------------------------------------------------------------------
def test_order_and_strands(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 22
    rng = np.random.default_rng(2)
    palindromes = [ref.rank(s) for s in ("ACGTACGTACGTACGTACGTAC"[:11] + ref.revcomp("ACGTACGTACGTACGTACGTAC"[:11]), "TTTTTTTTTTTAAAAAAAAAAA", "A" * 11 + "T" * 11)]
    keys = np.unique(np.concatenate((_random_kmers(rng, 3000, k), np.array(palindromes, dtype=np.uint64))))
    strings = uo.kmer_strings(keys, k)
    assert sum(s == ref.revcomp(s) for s in strings) >= 3
    counts = rng.integers(2, 600, keys.size)
    want = ref.database_bytes([_text(keys, counts, k)], k)
    pairs = list(zip(strings, counts.tolist()))
    before = kmers.dump_import_stats()
    assert _imported(gpu, tmp_path, [_text(keys, counts, k)]) == want
    after = kmers.dump_import_stats()
    assert after["imports"] == before["imports"] + 1 and after["sorts"] == before["sorts"], "ascending canonical keys: nothing to sort"
    assert after["lines"] == before["lines"] + keys.size
    order = rng.permutation(len(pairs))
    shuffled = "".join("{}\t{}\n".format(*pairs[i]) for i in order).encode()
    assert _imported(gpu, tmp_path, [shuffled]) == want
    assert kmers.dump_import_stats()["sorts"] == after["sorts"] + 1
    other = "".join("{}\t{}\n".format(ref.revcomp(s) if i % 2 else s, c) for i, (s, c) in enumerate(pairs)).encode()
    assert _imported(gpu, tmp_path, [other]) == want
    # both strands, the counter split between them (per line saturated first, as the rule says); a palindrome listed once
    both = []
    for s, c in pairs:
        c = min(c, 255)
        both += [(s, c)] if s == ref.revcomp(s) else [(s, c // 2), (ref.revcomp(s), c - c // 2)]
    split = "".join("{} {}\n".format(*both[i]) for i in rng.permutation(len(both))).encode()
    assert ref.database_bytes([split], k) == want, "the test's own expectation"
    assert _imported(gpu, tmp_path, [split]) == want


# ---- 3. several files ----------------------------------------------------------------------------------------------------------
def test_several_files(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(3)
    lane_a, lane_b = _reads(rng, 40), _reads(rng, 40)
    lane_b = lane_b + lane_a[:10]  # (overlapping reads; the random reads of either lane are its own)
    texts = []
    for lane in (lane_a, lane_b):
        keys, counts = uo.count_kmers_np(*uo.pack(lane), k)
        texts.append(ref.format(keys, np.minimum(counts, 255), k))
    pa, pb = _write(tmp_path, "a.txt", texts[0]), _write(tmp_path, "b.txt", texts[1])
    want = ref.database_bytes(texts, k, floor=1)
    with kmers.KmerDatabase.from_dump([pa, pb], floor=1) as both:
        assert _saved(both, tmp_path) == want
    with kmers.KmerDatabase.from_dump(pa, floor=1) as a, kmers.KmerDatabase.from_dump(pb, floor=1) as b, a.union(b) as united:
        assert _saved(united, tmp_path) == want
    # without saturated lanes that is the database of both lanes' reads counted together
    unit = "".join("ACGT"[c] for c in rng.integers(0, 4, 30)) * 160  # (each of its k-mers about 160 times a lane)
    small_a, small_b = lane_a[:5] + [unit], lane_b[:5] + lane_a[:2] + [unit]
    small = [uo.count_kmers_np(*uo.pack(lane), k) for lane in (small_a, small_b, small_a + small_b)]
    assert max(c.max() for _k, c in small[:2]) < 255 and small[2][1].max() > 255, "the sum saturates, the lanes do not"
    together = ref.database(small[2][0], np.minimum(small[2][1], 255), 1)
    assert _imported(gpu, tmp_path, [ref.format(kk, cc, k) for kk, cc in small[:2]], floor=1) == kf.file_bytes(k, *together[:3], magic=ref.magic(1))
    # the same file twice: every counter doubled, saturating
    pk, pc = ref.parse(texts[0], k)
    with kmers.KmerDatabase.from_dump([pa, pa]) as db:
        assert db.floor == 2  # (auto: no folded counter is 1)
        assert np.array_equal(db.entries()[0], pk) and np.array_equal(db.entries()[1], np.minimum(2 * pc.astype(np.int64), 255))
        assert _saved(db, tmp_path) == ref.database_bytes([texts[0], texts[0]], k)
    # an empty file among them changes nothing
    assert _imported(gpu, tmp_path, [texts[0], b"", texts[1]], floor=1, k=k) == want


# ---- 4. counters -----------------------------------------------------------------------------------------------------------------
ACCEPTED = ["1", "9", "10", "99", "100", "254", "255", "256", "4294967296", "9" * 32, "007", "18446744073709551616", "0255", "00000000000000000000000000000001"]


def test_counters_accepted_and_folded(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 15
    rng = np.random.default_rng(4)
    keys = _random_kmers(rng, len(ACCEPTED) + 2, k)
    strings = uo.kmer_strings(keys, k)
    lines = ["{}\t{}\n".format(s, d) for s, d in zip(strings, ACCEPTED)]
    lines += ["{}\t{}\n".format(strings[-2], c) for c in (200, 100, 1)]  # a run of three: 255
    lines += ["{} 1\n".format(strings[-1])] * 300                        # 300 ones: 255, at most 255 steps of the head's lane
    want_counts = [min(int(d), 255) for d in ACCEPTED] + [255, 255]
    for name, order in (("as written", np.arange(len(lines))), ("shuffled", rng.permutation(len(lines)))):
        text = "".join(lines[i] for i in order).encode()
        path = _write(tmp_path, "c.txt", text)
        with kmers.KmerDatabase.from_dump(path, floor=1) as db:
            got_keys, got_counts = db.entries()
            assert np.array_equal(got_keys, keys) and got_counts.tolist() == want_counts, name
            assert _saved(db, tmp_path) == ref.database_bytes([text], k, floor=1), name


# runs of equal keys as (first, last) entry of the sorted pairs: across a flag word's edge, across a tile's edge (1024
# entries), 300 ones up to a tile's last entry, from a tile's first entry on, the last two entries (of a partial tile)
FOLD_RUNS = [(62, 65), (1022, 1025), (1748, 2047), (2048, 2050), (2506, 2507)]
FOLD_COUNTERS = [(1, 2, 3, 4), (200, 100, 1, 1), (1,) * 300, (1, 1, 1), (1, 1)]


def test_fold_at_word_and_tile_edges(gpu, tmp_path):
    """The fold's heads and runs where the compaction's layout has its edges (FOLD_RUNS); every other key stands once."""
    k = 21
    rng = np.random.default_rng(41)
    total = FOLD_RUNS[-1][1] + 1
    times = []  # how often each distinct key is written, in the keys' order
    for first, last in FOLD_RUNS:
        times += [1] * (first - sum(times)) + [last - first + 1]
    assert sum(times) == total
    keys = _random_kmers(rng, len(times), k)
    assert keys.size == 2200
    counts = []
    runs = iter(FOLD_COUNTERS)
    for t in times:
        counts += list(next(runs)) if t > 1 else [int(rng.integers(1, 300))]
    order = rng.permutation(total)
    text = _text(np.repeat(keys, times)[order], np.array(counts)[order], k)
    # the positions are what this test is about: found again from the text alone
    parsed = np.sort(ref.parse(text, k)[0])
    heads = np.flatnonzero(np.concatenate(([True], parsed[1:] != parsed[:-1], [True])))
    assert [(int(a), int(b) - 1) for a, b in zip(heads[:-1], heads[1:]) if b - a > 1] == FOLD_RUNS and parsed.size == total
    for floor in (1, 2):
        want = ref.database_bytes([text], k, floor=floor)
        assert _imported(gpu, tmp_path, [text], floor=floor) == want, floor
    folded = ref.fold(*ref.parse(text, k))[1]
    assert folded[np.array(times) > 1].tolist() == [10, 255, 255, 3, 2], "the test's own expectation"


@pytest.mark.parametrize("digits,reason", [("0", ref.ZERO), ("000", ref.ZERO), ("-1", ref.NOT_DIGITS), ("+1", ref.NOT_DIGITS), ("1.0", ref.NOT_DIGITS),
                                           ("1e3", ref.NOT_DIGITS), ("", ref.EMPTY_COUNTER), ("1" * 33, ref.TOO_MANY_DIGITS), ("1" * 34, ref.TOO_MANY_DIGITS),
                                           ("1" * 35, ref.TOO_LONG), ("1" * 5000, ref.TOO_LONG)])
def test_counters_refused(gpu, tmp_path, digits, reason):
    k = 15
    keys = _random_kmers(np.random.default_rng(41), 9, k)
    lines = _text(keys, [3] * 9, k).split(b"\n")[:-1]
    lines[6] = lines[6][:k + 1] + digits.encode()
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, 7, reason)


def test_a_line_longer_than_a_window(gpu, tmp_path):
    """no newline within a window's bytes: the host's cut finds it, after the windows before it have been parsed"""
    k = 15
    keys = _random_kmers(np.random.default_rng(42), 400, k)
    lines = _text(keys, [3] * 400, k).split(b"\n")[:-1]
    lines[300] = lines[300] + b"1" * 5000
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, 301, ref.TOO_LONG, window_bytes=4096)
    lines[100] = lines[100] + b"x"
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, 101, ref.NOT_DIGITS, window_bytes=4096)


# ---- 5. lines --------------------------------------------------------------------------------------------------------------------
def _sound_lines(k, n, seed=5):
    rng = np.random.default_rng(seed)
    keys = _random_kmers(rng, n, k)
    counts = rng.integers(1, 3000, n)
    return keys, counts, _text(keys, counts, k).split(b"\n")[:-1]


def test_separators_and_the_last_line(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    keys, _c, lines = _sound_lines(k, 50)
    lines = [l.replace(b"\t", b" ") if i % 2 else l for i, l in enumerate(lines)]
    text = b"\n".join(lines) + b"\n"
    want = ref.database_bytes([text], k)
    assert _imported(gpu, tmp_path, [text]) == want
    assert _imported(gpu, tmp_path, [text[:-1]]) == want, "a last line without its newline"
    assert _imported(gpu, tmp_path, [text[:-1], text[:-1]], floor=2) == ref.database_bytes([text[:-1], text[:-1]], k, floor=2), "each file's own last line"
    with kmers.KmerDatabase.from_dump(_write(tmp_path, "empty.txt", b""), k=k) as db:
        assert (len(db), db.k, db.floor) == (0, k, 2) and int(db.histogram().sum()) == 0
        assert _saved(db, tmp_path) == ref.database_bytes([b""], k)
    with pytest.raises(ValueError, match="empty"):
        kmers.KmerDatabase.from_dump(_write(tmp_path, "empty.txt", b""))  # (no k given and no line to take it from)
    with pytest.raises(IOError):
        kmers.KmerDatabase.from_dump(str(tmp_path / "missing.txt"), k=k)


DAMAGE = [
    ("two separators", lambda l, k: l[:k] + b"\t" + l[k:], ref.NOT_DIGITS),
    ("no separator", lambda l, k: l[:k] + l[k + 1:], ref.NO_SEPARATOR),
    ("no counter", lambda l, k: l[:k], ref.NO_COUNTER),
    ("k - 1 bases", lambda l, k: l[1:], ref.SHORT_KMER),
    ("k + 1 bases", lambda l, k: b"A" + l, ref.LONG_KMER),
    ("N", lambda l, k: l[:3] + b"N" + l[4:], ref.NOT_ACGT),
    ("lower case", lambda l, k: l[:k - 1] + l[k - 1:k].lower() + l[k:], ref.NOT_ACGT),
    ("carriage return", lambda l, k: l + b"\r", ref.NOT_DIGITS),
    ("empty line", lambda l, k: b"", ref.EMPTY),
]


@pytest.mark.parametrize("name,damage,reason", DAMAGE, ids=[d[0].replace(" ", "_") for d in DAMAGE])
def test_lines_refused(gpu, tmp_path, name, damage, reason):
    k = 21
    _keys, _c, lines = _sound_lines(k, 40)
    lines[16] = damage(lines[16], k)
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, 17, reason)


def test_empty_last_line_refused(gpu, tmp_path):
    k = 21
    _keys, _c, lines = _sound_lines(k, 40)
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n\n", k, 41, ref.EMPTY)
    _refused(gpu, tmp_path, b"\n", k, 1, ref.EMPTY)
    _refused(gpu, tmp_path, b"\n" + b"\n".join(lines) + b"\n", k, 1, ref.EMPTY)


@pytest.mark.parametrize("first,second,window", [(3, 5, 0), (10, 400, 65536), (10, 400, 0), (10, 900, 4096), (700, 701, 4096), (150, 156, 4096)],
                         ids=["one_tile", "two_tiles", "two_tiles_default_window", "two_windows", "late_window", "around_the_first_window_edge"])
def test_the_first_of_two_damaged_lines_is_named(gpu, tmp_path, first, second, window):
    k = 21
    _keys, _c, lines = _sound_lines(k, 1000)
    assert sum(len(l) + 1 for l in lines[:400]) > 2 * 4096 and sum(len(l) + 1 for l in lines[:10]) < 4096
    lines[first - 1] = lines[first - 1] + b"x"              # NOT_DIGITS
    lines[second - 1] = lines[second - 1][:2] + b"n" + lines[second - 1][3:]  # NOT_ACGT
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, first, ref.NOT_DIGITS, window_bytes=window)
    # the other way round: the reason follows the line, not the kind of damage
    lines[first - 1], lines[second - 1] = lines[second - 1], lines[first - 1]
    _refused(gpu, tmp_path, b"\n".join(lines) + b"\n", k, first, ref.NOT_ACGT, window_bytes=window)


def test_second_file_refusal_names_its_own_line(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    _keys, _c, lines = _sound_lines(k, 300)
    good = b"\n".join(lines) + b"\n"
    lines[200] = lines[200] + b" "
    pa, pb = _write(tmp_path, "a.txt", good[:-1]), _write(tmp_path, "b.txt", b"\n".join(lines) + b"\n")
    for window in (0, 4096):
        with pytest.raises(ValueError) as exc:
            kmers.KmerDatabase.from_dump([pa, pb], window_bytes=window)
        assert "{}: line 201: ".format(pb) in str(exc.value) and ref.NOT_DIGITS in str(exc.value)
    with pytest.raises(ValueError, match="window_bytes"):
        kmers.KmerDatabase.from_dump(pa, window_bytes=4095)


# ---- 6. tiles and windows -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """about 20 000 lines whose counters have 1 to 4 digits at random, some keys twice and on either strand, not in order"""
    k = 21
    rng = np.random.default_rng(6)
    keys = _random_kmers(rng, 19000, k)
    keys = np.concatenate((keys, keys[rng.integers(0, keys.size, 1000)]))
    rng.shuffle(keys)
    digits = rng.integers(1, 5, keys.size)
    counts = [int(rng.integers(10 ** (d - 1), 10 ** d)) for d in digits]
    strings = [ref.revcomp(s) if i % 3 == 0 else s for i, s in enumerate(uo.kmer_strings(keys, k))]
    text = "".join("{}\t{}\n".format(s, c) for s, c in zip(strings, counts)).encode()
    starts = np.cumsum([0] + [k + 2 + d for d in digits[:-1]])
    assert len(set((starts % 16).tolist())) == 16 and len(set((starts % 4096).tolist())) > 3500
    return k, text, {floor: ref.database_bytes([text], k, floor=floor) for floor in (1, 2)}


@pytest.mark.parametrize("window", [4096, 4097, 65536, 0])
def test_tiles_and_windows(gpu, tmp_path, big, window):
    k, text, want = big
    assert _imported(gpu, tmp_path, [text], floor=1, window_bytes=window) == want[1]
    assert _imported(gpu, tmp_path, [text[:-1]], floor=2, window_bytes=window) == want[2], "the last newline removed"


def test_windows_of_a_sorted_dump_need_no_sort(gpu, tmp_path, big):
    from trio_binning_amd import kmers

    k, text, want = big
    pk, pc = ref.parse(text, k)
    keys, counters = ref.fold(pk, pc)
    ordered = ref.format(keys, counters, k)
    before = kmers.dump_import_stats()
    assert _imported(gpu, tmp_path, [ordered], floor=1, window_bytes=4096) == want[1]
    after = kmers.dump_import_stats()
    assert after["sorts"] == before["sorts"] and after["windows"] - before["windows"] >= len(ordered) // 4096


# ---- 7. floor ------------------------------------------------------------------------------------------------------------------------
def test_floor(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 17
    rng = np.random.default_rng(7)
    keys = _random_kmers(rng, 2100, k)
    with_ones = np.where(rng.random(keys.size) < 0.4, 1, rng.integers(2, 300, keys.size))
    without = np.maximum(with_ones, 2)
    for counts, auto in ((with_ones, 1), (without, 2)):
        text = _text(keys, counts, k)
        path = _write(tmp_path, "f.txt", text)
        for floor in ("auto", 1, 2):
            with kmers.KmerDatabase.from_dump(path, floor=floor) as db:
                want_floor = auto if floor == "auto" else floor
                assert db.floor == want_floor
                hist = db.histogram()
                ones = int((counts == 1).sum())
                assert int(hist[0]) == keys.size and int(hist[1]) == ones
                assert len(db) == keys.size - (ones if want_floor == 2 else 0)
                data = _saved(db, tmp_path, "f{}.tbkdb".format(floor))
                assert data == ref.database_bytes([text], k, floor=floor)
                assert data[:8] == ref.magic(want_floor)
            with kmers.KmerDatabase.load(str(tmp_path / "f{}.tbkdb".format(floor))) as again:
                assert (again.floor, len(again)) == (want_floor, keys.size - (ones if want_floor == 2 else 0))
                assert np.array_equal(again.histogram(), hist)
    # every folded counter 1 and floor 2: a database without entries that still states what it saw
    text = _text(keys, [1] * keys.size, k)
    with kmers.KmerDatabase.from_dump(_write(tmp_path, "ones.txt", text), floor=2) as db:
        assert len(db) == 0 and int(db.histogram()[1]) == keys.size
        assert _saved(db, tmp_path) == ref.database_bytes([text], k, floor=2)


# ---- 8. compressed ---------------------------------------------------------------------------------------------------------------------
def test_compressed(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 15
    rng = np.random.default_rng(8)
    reads = _reads(rng)
    squeezed = hpc_ref.compress_reads(reads, True)
    keys, counts = uo.count_kmers_np(*uo.pack(squeezed), k)
    text = ref.format(keys, np.minimum(counts, 255), k)
    path = _write(tmp_path, "hpc.txt", text)
    for keep, magic in ((True, b"TBKKMFH1"), (False, b"TBKKMDH1")):
        with kmers.KmerCounter(k, 1 << 16, compress=True, keep_singletons=keep) as counter:
            counter.add_reads(reads)
            with counter.database() as db:
                st = db.stats()
                want = _saved(db, tmp_path, "want.tbkdb")
        with kmers.KmerDatabase.from_dump(path, compressed=True, floor=1 if keep else 2, reads=st["reads_added"], bases=st["bases_added"]) as db:
            assert db.compressed and db.floor == (1 if keep else 2)
            got = _saved(db, tmp_path)
        assert got[:8] == magic and got == want
    # one line with two equal adjacent bases: refused with the flag, accepted without
    lines = text.split(b"\n")[:-1]
    lines[30] = lines[30][:5] + lines[30][4:5] + lines[30][6:]
    assert lines[30][4] == lines[30][5]
    damaged = b"\n".join(lines) + b"\n"
    _refused(gpu, tmp_path, damaged, k, 31, ref.NOT_COMPRESSED, compressed=True)
    assert _imported(gpu, tmp_path, [damaged], floor=1) == ref.database_bytes([damaged], k, floor=1)


# ---- 9. export ranges ------------------------------------------------------------------------------------------------------------------
RANGES = [(1, 255), (2, 255), (3, 7), (255, 255), (7, 3), (0, 1000), (256, 300)]


@pytest.mark.parametrize("floor", [1, 2])
@pytest.mark.parametrize("k", [21, 32])
def test_export_ranges(gpu, tmp_path, floor, k):
    from trio_binning_amd import kmers

    rng = np.random.default_rng(90 + floor + k)
    keys = _random_kmers(rng, 2500, k)
    if k == 32:
        keys = np.unique(np.concatenate((keys, np.array([0, (1 << 63) + 5, (1 << 64) - 1 - 3], dtype=np.uint64))))  # (not all canonical: an export takes the keys as they are)
    counts = np.where(rng.random(keys.size) < 0.3, rng.integers(1, 9, keys.size), rng.integers(1, 256, keys.size)).astype(np.uint8)
    counts[:3] = (255, 1, 7)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[0] = keys.size
    if floor == 2:
        keep = counts >= 2
        keys, counts = keys[keep], counts[keep]
    path = _write(tmp_path, "db.tbkdb", kf.file_bytes(k, keys, counts, hist, reads=3, bases=99, magic=ref.magic(floor)))
    with kmers.KmerDatabase.load(path) as db:
        for lo, hi in RANGES:
            out = str(tmp_path / "out.txt")
            n = db.dump(out, lo, hi)
            want = ref.format(keys, counts, k, max(lo, floor), min(hi, 255))
            with open(out, "rb") as fh:
                assert fh.read() == want, (lo, hi)
            assert n == want.count(b"\n")
            assert not os.path.exists(out + ".tmp")
            if (lo, hi) in ((7, 3), (256, 300)):
                assert n == 0 and want == b""
        # the default range, read back: the same database
        out = str(tmp_path / "all.txt")
        assert db.dump(out) == keys.size
        if k != 32 and floor == 1:  # (the k = 32 keys above are not all canonical; a solid dump does not say what was seen once)
            with kmers.KmerDatabase.from_dump(out, floor=1, reads=3, bases=99) as back, open(path, "rb") as fh:
                assert _saved(back, tmp_path) == fh.read()
        # a failed write: IOError, and no .tmp file left
        target = tmp_path / "a_directory"
        target.mkdir()
        (target / "inside").write_text("x")
        with pytest.raises(IOError):
            db.dump(str(target))
        assert not os.path.exists(str(target) + ".tmp") and os.path.isdir(str(target))
        with pytest.raises(IOError):
            db.dump(str(tmp_path / "no_such_directory" / "out.txt"))


def test_export_of_an_empty_database(gpu, tmp_path):
    from trio_binning_amd import kmers

    hist = np.zeros(256, dtype=np.uint64)
    path = _write(tmp_path, "empty.tbkdb", kf.file_bytes(21, [], [], hist))
    with kmers.KmerDatabase.load(path) as db:
        out = str(tmp_path / "out.txt")
        assert db.dump(out) == 0 and os.path.getsize(out) == 0


# ---- 10. after a refusal or TBK_ERR_NOMEM --------------------------------------------------------------------------------------------
def test_the_device_stays_usable(gpu, tmp_path, big):
    from trio_binning_amd import _lib, kmers

    k, text, want = big
    path = _write(tmp_path, "big.txt", text)
    lines = text.split(b"\n")
    lines[15000] = lines[15000] + b"?"
    _refused(gpu, tmp_path, b"\n".join(lines), k, 15001, ref.NOT_DIGITS, window_bytes=65536)
    with kmers.KmerDatabase.from_dump(path, floor=1, window_bytes=65536) as db:
        assert _saved(db, tmp_path) == want[1]
    # no memory at the first allocation, at the pairs, at the sort's second set of pairs: each time nothing is left behind
    free0 = kmers.device_mem_info()[0]
    try:
        for limit in (1000, 100_000, 300_000):
            _lib.lib.tbk_dump_set_alloc_limit_(limit)
            with pytest.raises(MemoryError):
                kmers.KmerDatabase.from_dump(path, floor=1, window_bytes=4096)
    finally:
        _lib.lib.tbk_dump_set_alloc_limit_(0)
    with kmers.KmerDatabase.from_dump(path, floor=2, window_bytes=4096) as db:
        assert _saved(db, tmp_path) == want[2]
    assert kmers.device_mem_info()[0] >= free0 - (8 << 20), "device memory of the failed imports was not given back"
