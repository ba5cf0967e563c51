"""The k-mer counter working in passes (tbk_counter_create_opts, KmerCounter(passes=P)): the reads are kept on the
device, one class of k-mers at a time goes through the table, and histogram, subtraction and dump come from the
classes' databases.  Everything must equal the oracle's restatement of the KMC steps (oracle/unique_oracle.py) and
what the single-pass counter writes; the table must really be smaller."""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGT", "TGCA")
RANGES = ((2, 255), (3, 20), (5, 5), (1, 4), (200, 255))


def _rc(s):
    return s.translate(COMP)[::-1]


# ---- libraries, made as tests/test_gpu_unique.py makes them ---------------------------------------------
def _library(rng, genome, n_reads, read_len, err=0.01, lower=0.0, n_rate=0.001):
    reads = []
    for _ in range(n_reads):
        p = int(rng.integers(0, len(genome) - read_len))
        s = list(genome[p:p + read_len])
        for i in np.nonzero(rng.random(read_len) < err)[0]:
            s[int(i)] = "ACGT"[int(rng.integers(0, 4))]
        for i in np.nonzero(rng.random(read_len) < n_rate)[0]:
            s[int(i)] = "N"
        r = "".join(s)
        if rng.random() < 0.5:
            r = _rc(r)
        if rng.random() < lower:
            r = r.lower()
        reads.append(r)
    return reads


def _two_parents(rng, glen=30_000, snp=1 / 200):
    base = "".join("ACGT"[c] for c in rng.integers(0, 4, glen))
    def mutate():
        s = list(base)
        for i in np.nonzero(rng.random(glen) < snp)[0]:
            s[int(i)] = "ACGT"[(("ACGT".index(s[int(i)])) + int(rng.integers(1, 4))) % 4]
        return "".join(s)
    return mutate(), mutate()


def _random_dna(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _add_in_batches(counter, reads, cuts):
    """`cuts`: batch sizes, repeated until the reads are used up."""
    i = j = 0
    while i < len(reads):
        step = cuts[j % len(cuts)]
        counter.add_reads(reads[i:i + step])
        i, j = i + step, j + 1


def _dump(counter, other, lo, hi, path):
    n = counter.unique(other, lo, hi, str(path))
    text = open(path).read()
    lines = text.split("\n")
    assert lines[-1] == "" and n == len(lines) - 1
    return text


def _check_histogram(hist, counts, db):
    from oracle import unique_oracle as uo

    assert int(hist[0]) == len(counts)
    assert int(hist[1]) == sum(1 for n in counts.values() if n == 1)
    assert [int(hist[c]) for c in range(2, 256)] == [n for c, n in uo.histogram_rows(db) if c >= 2]


# ---- 1. equal to the oracle and to the single pass --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(k):
    """The two libraries of a k, the oracle's view of them and (filled in by the first test that needs them) the
    single-pass counter's dumps."""
    from oracle import unique_oracle as uo

    rng = np.random.default_rng(100 + k)
    ga, gb = _two_parents(rng, glen=8_000 if k > 5 else 600)
    reads_a = _library(rng, ga, 900, 150, lower=0.1) + ["", "ACGT", "N" * 40, ga[:k - 1], ga[:k], ga[:k]]
    reads_b = _library(rng, gb, 700, 150)
    oa, ob = uo.count_kmers(reads_a, k), uo.count_kmers(reads_b, k)
    return {"a": reads_a, "b": reads_b, "oa": oa, "dba": uo.database(oa), "dbb": uo.database(ob), "single": {}}


def _single_pass_dumps(case, k, tmp_path):
    from trio_binning_amd import kmers

    if not case["single"]:
        with kmers.KmerCounter(k, 400_000) as ca, kmers.KmerCounter(k, 400_000) as cb:
            _add_in_batches(ca, case["a"], (250,))
            cb.add_reads(case["b"])
            case["single"]["hist"] = ca.histogram().tolist()
            for lo, hi in RANGES:
                case["single"][(lo, hi)] = _dump(ca, cb, lo, hi, tmp_path / f"single_{lo}_{hi}.txt")
    return case["single"]


@pytest.mark.parametrize("passes", [2, 3, 7])
@pytest.mark.parametrize("k", [5, 16, 21, 31, 32])
def test_passes_match_oracle_and_single_pass(gpu, tmp_path, k, passes):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    case = _case(k)
    single = _single_pass_dumps(case, k, tmp_path)
    with kmers.KmerCounter(k, 400_000, passes=passes) as ca, kmers.KmerCounter(k, 400_000, passes=passes) as cb:
        _add_in_batches(ca, case["a"], (250, 1, 333, 97, 225))  # five batches of unequal size
        _add_in_batches(cb, case["b"], (300, 123))
        st = ca.stats()
        assert st["passes"] == passes and not st["finished"] and st["store_bytes"] >= st["store_used_bytes"] > 0
        assert st["reads_added"] == len(case["a"]) and st["bases_added"] == sum(map(len, case["a"]))
        hist = ca.histogram()
        _check_histogram(hist, case["oa"], case["dba"])
        assert hist.tolist() == single["hist"]
        for lo, hi in RANGES:
            text = _dump(ca, cb, lo, hi, tmp_path / f"u_{lo}_{hi}.txt")
            assert text.split("\n")[:-1] == uo.unique_kmers(case["dba"], case["dbb"], lo, hi)
            assert text == single[(lo, hi)]  # byte for byte the single pass's file
        st = ca.stats()
        assert st["finished"] and st["store_bytes"] == 0 and st["distinct"] == len(case["oa"])
        assert st["database_bytes"] == 9 * len(case["dba"])


# ---- 2. empty and tiny classes ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_most_classes_empty(gpu, tmp_path, k):
    """4^k / 2 or so canonical k-mers in 16 classes: most classes hold nothing, some a k-mer or two."""
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    rng = np.random.default_rng(7 + k)
    reads_a = [_random_dna(rng, int(n)) for n in rng.integers(0, 12, 40)] + ["ACGTN" * 3, "acgtacgt"]
    reads_b = ["AC" * 4, "GGG", "TTTTT", ""]
    oa, ob = uo.count_kmers(reads_a, k), uo.count_kmers(reads_b, k)
    dba, dbb = uo.database(oa), uo.database(ob)
    with kmers.KmerCounter(k, 16, passes=16) as ca, kmers.KmerCounter(k, 16, passes=16) as cb:
        _add_in_batches(ca, reads_a, (7, 20))
        cb.add_reads(reads_b)
        _check_histogram(ca.histogram(), oa, dba)
        for lo, hi in ((2, 255), (1, 3), (4, 255)):
            text = _dump(ca, cb, lo, hi, tmp_path / f"u_{lo}_{hi}.txt")
            assert text.split("\n")[:-1] == uo.unique_kmers(dba, dbb, lo, hi)
        text = _dump(cb, ca, 2, 255, tmp_path / "b.txt")
        assert text.split("\n")[:-1] == uo.unique_kmers(dbb, dba, 2, 255)


def test_every_read_shorter_than_k(gpu, tmp_path):
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(3)
    reads = [_random_dna(rng, int(n)) for n in rng.integers(0, k, 200)] + ["", "N" * 20]
    with kmers.KmerCounter(k, 1000, passes=16) as ca, kmers.KmerCounter(k, 1000, passes=16) as cb:
        _add_in_batches(ca, reads, (64,))
        ca.finish()
        assert not ca.histogram().any() and ca.stats()["distinct"] == 0 and ca.stats()["database_bytes"] == 0
        assert _dump(ca, cb, 1, 255, tmp_path / "a.txt") == "" and _dump(cb, ca, 1, 255, tmp_path / "b.txt") == ""


# ---- 3. batch and chunk boundaries ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary_reads():
    """One read per batch, one batch per length of the separated stream (the read and the byte that closes it) from
    2032 to 2080 and from 4080 to 4112: the stream ends on, before and after a 16-base word of the store and a
    2048-window pass of the kernel.  Every read is a prefix of one sequence of period 2500, so a window that ran
    from the end of a batch into the start of the next would be a k-mer no read holds."""
    rng = np.random.default_rng(11)
    unit = _random_dna(rng, 2500)
    periodic = unit * 2
    return [periodic[:length - 1] for length in list(range(2032, 2081)) + list(range(4080, 4113))]


@pytest.mark.parametrize("k", [21, 32])
def test_batch_and_chunk_boundaries(gpu, tmp_path, k):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    reads = _boundary_reads()
    bases, offsets = uo.pack(reads)
    keys, counts = uo.count_kmers_np(bases, offsets, k)
    want = uo.histogram_np(counts)
    assert counts.max() < 255 and (want[2:255] > 0).sum() > 3  # the counts are told apart, none saturates
    with kmers.KmerCounter(k, 4000, passes=2) as c, kmers.KmerCounter(k, 16, passes=2) as empty:
        for r in reads:
            c.add_reads([r])
        assert c.histogram().tolist() == want.tolist()
        for lo, hi in ((2, 255), (int(counts.max()), 255), (2, int(np.median(counts)))):
            text = _dump(c, empty, lo, hi, tmp_path / f"u_{lo}_{hi}.txt")
            assert text.split("\n")[:-1] == uo.kmer_strings(uo.unique_np((keys, counts), (keys[:0], counts[:0]), lo, hi), k)


# ---- 4. saturation across passes --------------------------------------------------------------------------------
def test_saturation_across_passes(gpu, tmp_path):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    k = 21
    rng = np.random.default_rng(21)
    ga, gb = _two_parents(rng, glen=4000)
    sixty = _random_dna(rng, 60)
    reads_a = _library(rng, ga, 300, 150)
    reads_a = reads_a[:100] + ["A" * 400] + reads_a[100:200] + [sixty] * 300 + reads_a[200:]
    reads_b = _library(rng, gb, 300, 150) + [sixty[:30]] * 2
    oa, ob = uo.count_kmers(reads_a, k), uo.count_kmers(reads_b, k)
    dba, dbb = uo.database(oa), uo.database(ob)
    assert oa["A" * k] == 380 and sum(1 for n in dba.values() if n == 255) >= 41
    with kmers.KmerCounter(k, 50_000, passes=3) as ca, kmers.KmerCounter(k, 50_000, passes=3) as cb:
        _add_in_batches(ca, reads_a, (150, 77, 301))
        cb.add_reads(reads_b)
        hist = ca.histogram()
        _check_histogram(hist, oa, dba)
        assert int(hist[255]) == sum(1 for n in dba.values() if n == 255)
        for lo, hi in ((2, 255), (2, 254), (255, 255)):
            text = _dump(ca, cb, lo, hi, tmp_path / f"u_{lo}_{hi}.txt")
            assert text.split("\n")[:-1] == uo.unique_kmers(dba, dbb, lo, hi)


# ---- 5. the point of it: memory -----------------------------------------------------------------------------------
def test_table_of_a_class_is_smaller(gpu):
    """2 M random bases, practically every 21-mer distinct, into counters told to expect 65 536 k-mers: the table
    doubles as the batches arrive.  In 8 passes it holds an eighth of the k-mers, so by the growth rule of
    tbk_count.cpp (grow before a piece that could fill the table; a piece is a batch here) its largest size should be
    about an eighth of the single pass's; half is required, which leaves a factor for the granularity of doubling
    and for classes of unequal size.  The database is 9 bytes per k-mer seen at least twice; the slack of 4096 bytes
    allowed on top is not expected to be used."""
    from trio_binning_amd import kmers

    rng = np.random.default_rng(5)
    batches = []
    for _ in range(32):
        codes = rng.integers(0, 4, (64, 1000), dtype=np.uint8)
        bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].reshape(-1)
        batches.append((bases, np.arange(65, dtype=np.uint64) * 1000))
    out = {}
    for passes in (1, 8):
        with kmers.KmerCounter(21, 65_536, passes=passes) as c:
            for bases, offsets in batches:
                c.add(bases, offsets)
            c.finish()
            out[passes] = (c.histogram(), c.stats())
    (h1, s1), (h8, s8) = out[1], out[8]
    print("peak_table_bytes: 1 pass", s1["peak_table_bytes"], "8 passes", s8["peak_table_bytes"], "database_bytes", s8["database_bytes"])
    assert h1.tolist() == h8.tolist() and int(h1[0]) > 1_900_000
    assert s8["peak_table_bytes"] * 2 <= s1["peak_table_bytes"]
    assert s8["store_bytes"] == 0 and s8["finished"] and s8["distinct"] == int(h8[0])
    assert s8["database_bytes"] <= 9 * int(h8[2:].sum()) + 4096
    assert s1["store_bytes"] == 0 and s1["database_bytes"] == 0 and s1["passes"] == 1


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def _raw_counter(lib_mod, k, capacity, passes, store_limit=0, size=None):
    opts = lib_mod.CounterOptions()
    lib_mod.lib.tbk_counter_options_init(C.byref(opts))
    opts.passes, opts.store_limit_bytes = passes, store_limit
    if size is not None:
        opts.size = size
    h = C.c_void_p()
    from trio_binning_amd import kmers

    return lib_mod.lib.tbk_counter_create_opts(k, capacity, C.byref(opts), kmers.default_device(), C.byref(h)), h


def _still_works(tmp_path):
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    reads = ["ACGTACGTAC", "ACGTA", "GGGTTACCA"]
    want = uo.count_kmers(reads, 5)
    with kmers.KmerCounter(5, 100, passes=2) as c, kmers.KmerCounter(5, 100, passes=2) as d:
        c.add_reads(reads)
        assert int(c.histogram()[0]) == len(want)
        assert _dump(c, d, 2, 255, tmp_path / "ok.txt").split("\n")[:-1] == uo.unique_kmers(uo.database(want), {}, 2, 255)


def test_refusals(gpu, tmp_path):
    from trio_binning_amd import kmers

    _lib = gpu
    lib = _lib.lib
    reads = ["ACGTTGCAAGGCTTAACCGGATCGATCGGATT"] * 3
    off = str(tmp_path / "never.txt")
    n = C.c_uint64()
    for passes in (1, 2):  # adding to a finished counter
        with kmers.KmerCounter(21, 1000, passes=passes) as c:
            c.add_reads(reads)
            c.finish()
            c.finish()  # (finishing twice is fine)
            bases, offsets = kmers.pack_reads(reads)
            assert lib.tbk_counter_add_batch(c._h, bases.ctypes.data, offsets.ctypes.data, 3) == _lib.TBK_ERR_INVALID
            assert "finished" in _lib.last_error()
            with pytest.raises(ValueError, match="finished"):
                c.add_reads(reads)
            assert int(c.histogram()[3]) == 12
    with kmers.KmerCounter(21, 1000, passes=2) as c2, kmers.KmerCounter(21, 1000, passes=3) as c3, kmers.KmerCounter(21, 1000) as c1:
        for c in (c1, c2, c3):
            c.add_reads(reads)
        for a, b, names in ((c2, c3, ("2", "3")), (c3, c2, ("3", "2")), (c2, c1, ("2", "1")), (c1, c2, ("1", "2"))):
            assert lib.tbk_counter_unique(a._h, b._h, 2, 255, os.fsencode(off), C.byref(n)) == _lib.TBK_ERR_INVALID
            msg = _lib.last_error()
            assert "passes" in msg and "({} and {})".format(*names) in msg
            with pytest.raises(ValueError, match="passes"):
                a.unique(b, 2, 255, off)
        assert not os.path.exists(off)
    # the options struct through the C-ABI
    for passes in (0, -1, 1025):
        rc, h = _raw_counter(_lib, 21, 1000, passes)
        assert rc == _lib.TBK_ERR_INVALID and not h.value and "passes" in _lib.last_error()
    rc, h = _raw_counter(_lib, 21, 1000, 2, size=4)
    assert rc == _lib.TBK_ERR_INVALID and not h.value
    with pytest.raises(ValueError, match="passes"):
        kmers.KmerCounter(21, 1000, passes=0)
    # a store limited to 1 MB, 4 MB of reads (2 MB packed)
    rng = np.random.default_rng(1)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1 << 20, dtype=np.uint8)]
    offsets = np.arange(1025, dtype=np.uint64) * 1024
    with kmers.KmerCounter(21, 100_000, passes=2, store_limit=1 << 20) as c:
        c.add(bases, offsets)  # the first MB of reads: half a MB packed
        for _ in range(3):     # the second would pass the limit, and so would every later one
            assert lib.tbk_counter_add_batch(c._h, bases.ctypes.data, offsets.ctypes.data, 1024) == _lib.TBK_ERR_NOMEM
            assert "{} bases are retained".format(1 << 20) in _lib.last_error()
        with pytest.raises(MemoryError, match="bases are retained"):
            c.add(bases, offsets)
        st = c.stats()
        assert st["store_used_bytes"] <= 1 << 20 and st["bases_added"] == 1 << 20
    _still_works(tmp_path)


# ---- 7. the command line -------------------------------------------------------------------------------------------------
def test_cli_passes(gpu, tmp_path, capsys):
    """The fixture of test_find_unique_kmers_cli (two parents of a 60 kb genome at 25x), parent A gzip'ed in two
    files: --passes 3 writes the lists and histograms --passes 1 writes."""
    from trio_binning_amd import find_unique_kmers as fu

    k = 21
    rng = np.random.default_rng(77)
    ga, gb = _two_parents(rng, glen=60_000)
    reads_a, reads_b = _library(rng, ga, 10_000, 150), _library(rng, gb, 10_000, 150)

    def fastq(path, reads, gz=False):
        text = "".join(f"@r{i} x\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads))
        with (gzip.open if gz else open)(path, "wt") as fh:
            fh.write(text)
        return str(path)

    fa = fastq(tmp_path / "a1.fastq.gz", reads_a[:6000], gz=True) + "," + fastq(tmp_path / "a2.fastq.gz", reads_a[6000:], gz=True)
    fb = fastq(tmp_path / "b.fastq", reads_b)
    got = {}
    for passes in (1, 3):
        out = tmp_path / f"out{passes}"
        out.mkdir()
        fu.main(["-k", str(k), "-o", str(out), "-s", str(out), "--capacity", "3000000", "--passes", str(passes), fa, fb])
        err = capsys.readouterr().err
        assert "Using counts in range [" in err and "# of unique k-mers in haplotype A:" in err
        got[passes] = [open(out / name, "rb").read() for name in
                       ("hapA_only_kmers.txt", "hapB_only_kmers.txt", "haplotypeA.histogram", "haplotypeB.histogram")]
    assert got[3] == got[1] and all(len(x) > 1000 for x in got[1])


# ---- 8. seeded fuzz ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(int(os.environ.get("TBK_FUZZ_SEEDS", "8"))))
def test_passes_seeded_fuzz(gpu, tmp_path, seed):
    """test_counter_seeded_fuzz with a random number of passes and both counters cut into random batches."""
    from oracle import unique_oracle as uo
    from trio_binning_amd import kmers

    rng = np.random.default_rng(9000 + seed)
    k = int(rng.choice([1, 3, 8, 15, 16, 17, 21, 25, 31, 32]))
    passes = int(rng.integers(1, 10))
    ga, gb = _two_parents(rng, glen=int(rng.choice([300, 3000, 12000])), snp=1 / 100)
    def lib(g):
        n, L = int(rng.integers(1, 400)), int(rng.choice([20, 75, 150, 400]))
        L = min(L, len(g) - 1)
        reads = _library(rng, g, n, L, err=float(rng.choice([0.0, 0.01, 0.05])), lower=0.2, n_rate=0.003)
        return reads + ["", "N" * 30, g[:max(k - 1, 0)], g[:k], g[:k].lower()]
    reads_a, reads_b = lib(ga), lib(gb)
    cap_a, cap_b = int(rng.choice([16, 200_000])), int(rng.choice([16, 200_000]))
    with kmers.KmerCounter(k, cap_a, passes=passes) as ca, kmers.KmerCounter(k, cap_b, passes=passes) as cb:
        for counter, reads in ((ca, reads_a), (cb, reads_b)):
            i = 0
            while i < len(reads):
                step = int(rng.integers(1, 200))
                counter.add_reads(reads[i:i + step])
                i += step
        oa, ob = uo.count_kmers(reads_a, k), uo.count_kmers(reads_b, k)
        dba, dbb = uo.database(oa), uo.database(ob)
        hist = ca.histogram()
        assert int(hist[0]) == len(oa) == ca.stats()["distinct"], (k, passes)
        assert [int(hist[c]) for c in range(2, 256)] == [n for c, n in uo.histogram_rows(dba) if c >= 2]
        for lo, hi in ((2, 255), (3, 9), (int(rng.integers(1, 6)), int(rng.integers(6, 300)))):
            text = _dump(ca, cb, lo, hi, tmp_path / f"u_{lo}_{hi}.txt")
            assert text.split("\n")[:-1] == uo.unique_kmers(dba, dbb, lo, min(hi, 255)), (k, passes, lo, hi)
