"""Counting in homopolymer-compressed space (kmers.KmerCounter(compress=True), tbk_counter_options.compress) and the databases
it leaves (magic TBKKMDH1).  Everything after the compression is the existing counter on the compressed batch, so the
yardstick is the existing oracle, oracle.unique_oracle.count_kmers_np, run on tests/hpc_ref.compress_np(..., fold_case=True)
of the same reads; files are crafted with tests/kmerdb_files.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import hpc_ref
import kmerdb_files as kf

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGT", "TGCA")
KS = (5, 21, 32)
MAGIC_HPC = b"TBKKMDH1"


def _jitter(rng, s):
    """Every homopolymer run of s made one base longer, one shorter (never empty) or left alone, a third each."""
    out = []
    for ch, run in itertools.groupby(s):
        n = len(list(run)) + int(rng.integers(-1, 2))
        out.append(ch * max(n, 1))
    return "".join(out)


def _library(rng, genome, n_reads):
    reads = []
    for _ in range(n_reads):
        length = int(rng.integers(150, 3001))
        p = int(rng.integers(0, len(genome) - length))
        r = _jitter(rng, genome[p:p + length])
        if rng.random() < 0.5:
            r = r.translate(COMP)[::-1]
        if rng.random() < 0.15:
            r = r.lower()
        elif rng.random() < 0.15:  # mixed case inside runs: folded together by the counter
            r = "".join(c.lower() if i % 3 == 0 else c for i, c in enumerate(r))
        if rng.random() < 0.3:
            q = int(rng.integers(0, len(r)))
            r = r[:q] + "NN" + r[q:]
        reads.append(r)
    return reads + ["", "A", "AAAA", "acgt" * 10]


@functools.lru_cache(maxsize=None)
def _parents():
    """Two libraries of about 200 reads of 150 to 3000 bases from two haplotypes of a random genome, their compressed batches."""
    from oracle import unique_oracle as uo

    rng = np.random.default_rng(77)
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, 20_000))
    other = list(base)
    for i in np.flatnonzero(rng.random(len(base)) < 1 / 150):
        other[int(i)] = "ACGT"[("ACGT".index(other[int(i)]) + int(rng.integers(1, 4))) % 4]
    out = {}
    for name, genome, n in (("a", base, 200), ("b", "".join(other), 160)):
        reads = _library(rng, genome, n)
        bases, offsets = uo.pack(reads)
        cb, co = hpc_ref.compress_np(bases, offsets, True)
        out[name] = {"reads": reads, "bases": bases, "offsets": offsets, "cb": cb, "co": co}
    return out


@functools.lru_cache(maxsize=None)
def _counts(name, k):
    from oracle import unique_oracle as uo

    p = _parents()[name]
    return uo.count_kmers_np(p["cb"], p["co"], k)


def _count(name, k, mode="host", compress=True):
    """A counter fed the library in several batches: from host memory, in three passes, or from batches already in HBM."""
    from trio_binning_amd import kmers
    from trio_binning_amd._lib import check, lib

    p = _parents()[name]
    reads = p["reads"]
    counter = kmers.KmerCounter(k, 300_000, passes=3 if mode == "passes" else 1, compress=compress)
    for lo in range(0, len(reads), 70):
        part = reads[lo:lo + 70]
        if mode != "device":
            counter.add_reads(part)
            continue
        from oracle import unique_oracle as uo

        bases, offsets = uo.pack(part)
        d_bases, d_offsets = C.c_void_p(), C.c_void_p()
        check(lib.tbk_device_alloc(counter.device, bases.size + 64, C.byref(d_bases)))
        check(lib.tbk_device_alloc(counter.device, offsets.nbytes, C.byref(d_offsets)))
        try:
            check(lib.tbk_memcpy_h2d(counter.device, d_bases, bases.ctypes.data, bases.size))
            check(lib.tbk_memcpy_h2d(counter.device, d_offsets, offsets.ctypes.data, offsets.nbytes))
            counter.add_device(d_bases.value, d_offsets.value, len(part), int(offsets[-1]))
        finally:
            lib.tbk_device_free(counter.device, d_bases)
            lib.tbk_device_free(counter.device, d_offsets)
    return counter


def _has_equal_neighbours(keys, k):
    """per key: two equal adjacent bases somewhere in the k-mer"""
    keys = np.asarray(keys, dtype=np.uint64)
    if k < 2:
        return np.zeros(keys.size, dtype=bool)
    same = ~(keys ^ (keys >> np.uint64(2)))  # both bits of a base equal to the next one's: 11 at the pair's place
    pairs = same & (same >> np.uint64(1)) & np.uint64(0x5555555555555555)
    mask = np.uint64((1 << (2 * (k - 1))) - 1)
    return (pairs & mask) != 0


def packed_keys(ranks, k):
    """rank (base 0 in the top bits of the 2k) -> a list's key (base i at bits 2i..2i+1), base by base"""
    ranks = np.asarray(ranks, dtype=np.uint64)
    out = np.zeros_like(ranks)
    for i in range(k):
        out |= ((ranks >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)) << np.uint64(2 * i)
    return out


@pytest.mark.parametrize("mode", ["host", "passes", "device"])
@pytest.mark.parametrize("k", KS)
def test_a_compressing_counter_counts_the_compressed_reads(gpu, k, mode):
    from oracle import unique_oracle as uo

    p = _parents()["a"]
    keys, counts = _counts("a", k)
    assert keys.size and not _has_equal_neighbours(keys, k).any()  # (the oracle's own k-mers are compressed ones)
    with _count("a", k, mode) as counter:
        assert counter.compress
        st = counter.stats()
        assert st["reads_added"] == len(p["reads"]) and st["bases_added"] == p["cb"].size
        assert np.array_equal(counter.histogram().astype(np.int64), uo.histogram_np(counts))
        with counter.database() as db:
            assert db.compressed and db.k == k
            want_keys, want_counts, want_hist = kf.database_of(keys, counts)
            got_keys, got_counts = db.entries()
            assert np.array_equal(got_keys, want_keys) and np.array_equal(got_counts, want_counts)
            assert np.array_equal(db.histogram(), want_hist)
            assert db.stats()["reads_added"] == len(p["reads"]) and db.stats()["bases_added"] == p["cb"].size


def test_a_plain_counter_is_what_it_was(gpu):
    from oracle import unique_oracle as uo

    p = _parents()["a"]
    with _count("a", 21, compress=False) as counter:
        assert not counter.compress and counter.stats()["bases_added"] == p["bases"].size
        assert np.array_equal(counter.histogram().astype(np.int64), uo.histogram_np(uo.count_kmers_np(p["bases"], p["offsets"], 21)[1]))
        with counter.database() as db:
            assert not db.compressed


@pytest.mark.parametrize("k", KS)
def test_a_compressed_database_is_a_file_of_its_own_kind(gpu, tmp_path, k):
    from trio_binning_amd import kmers

    p = _parents()["a"]
    keys, cnt, hist = kf.database_of(*_counts("a", k))
    want = kf.file_bytes(k, keys, cnt, hist, reads=len(p["reads"]), bases=p["cb"].size, magic=MAGIC_HPC)
    path = str(tmp_path / "a.tbkdb")
    with _count("a", k) as counter, counter.database() as db:
        db.save(path)
    data = open(path, "rb").read()
    assert data[:8] == MAGIC_HPC and data == want
    info = kmers.database_file_info(path)
    assert info["compressed"] and info["k"] == k and info["n"] == keys.size
    with kmers.KmerDatabase.load(path) as back:
        assert back.compressed
        got_keys, got_counts = back.entries()
        assert np.array_equal(got_keys, keys) and np.array_equal(got_counts, cnt) and np.array_equal(back.histogram(), hist)
        again = str(tmp_path / "again.tbkdb")
        back.save(again)
        assert open(again, "rb").read() == want
    plain = str(tmp_path / "plain.tbkdb")
    with open(plain, "wb") as fh:
        fh.write(kf.file_bytes(k, keys, cnt, hist, reads=len(p["reads"]), bases=p["cb"].size))
    assert not kmers.database_file_info(plain)["compressed"]
    with kmers.KmerDatabase.load(plain) as db:
        assert not db.compressed


def test_a_damaged_compressed_file_is_still_refused(gpu, tmp_path):
    from trio_binning_amd import kmers

    sound, keys, counts, hist = kf.sound(k=21, n=5, seed=4)
    data = MAGIC_HPC + sound[8:]
    data = kf.with_crc(data)
    path = str(tmp_path / "sound.tbkdb")
    with open(path, "wb") as fh:
        fh.write(data)
    assert data == kf.file_bytes(21, keys, counts, hist, reads=11, bases=1234, magic=MAGIC_HPC)
    assert kmers.database_file_info(path)["compressed"]
    with kmers.KmerDatabase.load(path) as db:
        assert db.compressed and np.array_equal(db.entries()[0], keys)
    for name, damaged in kf.header_refusals(data):
        bad = str(tmp_path / (name + ".tbkdb"))
        with open(bad, "wb") as fh:
            fh.write(damaged)
        with pytest.raises(ValueError):
            kmers.database_file_info(bad)
        with pytest.raises(ValueError):
            kmers.KmerDatabase.load(bad)


@pytest.mark.parametrize("k", KS)
def test_compressed_and_plain_do_not_mix_and_two_compressed_subtract(gpu, tmp_path, k):
    from oracle import unique_oracle as uo
    na, nb = _counts("a", k), _counts("b", k)
    out = str(tmp_path / "list.txt")
    with _count("a", k) as ca, _count("b", k) as cb, _count("b", k, compress=False) as plain_counter:
        with pytest.raises(ValueError, match="compressed"):
            ca.unique(plain_counter, 2, 255, out)
        with pytest.raises(ValueError, match="compressed"):
            plain_counter.unique(ca, 2, 255, out)
        for lo, hi in ((2, 255), (3, 20)):
            want = uo.unique_np(na, nb, lo, hi)
            assert ca.unique(cb, lo, hi, out) == want.size
            assert np.array_equal(uo.read_list_np(out, k), want) and not _has_equal_neighbours(want, k).any()
        with ca.database() as da, cb.database() as db, plain_counter.database() as plain:
            assert da.compressed and db.compressed and not plain.compressed
            for first, second, child in ((da, plain, None), (plain, da, None), (da, db, plain), (da, plain, db), (plain, da, db)):
                third = {} if child is None else {"child": child}
                with pytest.raises(ValueError, match="compressed"):
                    first.unique(second, 2, 255, out, **third)
                with pytest.raises(ValueError, match="compressed"):
                    first.unique_set(second, 2, 255, **third)
            for lo, hi in ((2, 255), (3, 20)):
                want = uo.unique_np(na, nb, lo, hi)
                assert da.unique(db, lo, hi, out) == want.size and np.array_equal(uo.read_list_np(out, k), want)
                if want.size == 0:  # (k = 5: both parents hold every compressed 5-mer) an empty selection is no list, as ever
                    for third in ({}, {"child": da}):
                        with pytest.raises(ValueError, match="empty k-mer list"):
                            da.unique_set(db, lo, hi, **third)
                    assert da.unique(db, lo, hi, out, child=da) == 0 and open(out).read() == ""
                    continue
                with da.unique_set(db, lo, hi) as hs:
                    assert np.array_equal(hs.keys(), packed_keys(want, k))
                # the inherited forms, with B's own library standing in for a child: what A alone holds, B's child cannot hold
                held = want[np.isin(want, nb[0][nb[1] >= 2])]
                assert held.size == 0 and da.unique(db, lo, hi, out, child=db) == 0
                # ... and with A's own database as the child: everything A alone holds, it holds
                assert da.unique(db, lo, hi, out, child=da) == want.size and np.array_equal(uo.read_list_np(out, k), want)
                with da.unique_set(db, lo, hi, child=da) as hs:
                    assert np.array_equal(hs.keys(), packed_keys(want, k))
                text = open(out).read().split()
                assert all(x != y for line in text for x, y in zip(line, line[1:]))
