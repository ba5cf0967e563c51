"""The GC x count matrix without a GPU: the reference's GC of a key (tests/db_gc_ref.py) against counting letters, the summary
lines of the gc_spectrum command from hand-made matrices, its matrix file there and back, and every refusal of gc_spectrum and
of select_database's --min-gc / --max-gc - from the arguments and crafted headers (tests/kmerdb_files.py) alone, with the
device's entry points patched to fail the test if they are reached."""
import contextlib
import os
from unittest.mock import patch

import numpy as np
import pytest

import db_gc_ref as ref
import db_select_ref
import kmerdb_files as kf
from test_host_kmerdb_full import FULL_HPC, full_file

DEVICE_ENTRIES = ("tbk_kmerdb_load", "tbk_kmerdb_select", "tbk_kmerdb_save", "tbk_kmerdb_gc_spectrum")


@contextlib.contextmanager
def no_device():
    from trio_binning_amd import _lib, kmers

    def reached(*args, **kw):
        raise AssertionError("the device was touched: KmerDatabase.load")

    with contextlib.ExitStack() as stack:
        stack.enter_context(patch.object(kmers.KmerDatabase, "load", reached))
        for name in DEVICE_ENTRIES:
            stack.enter_context(patch.object(_lib.lib, name, side_effect=AssertionError("the device was touched: " + name)))
        yield


# ---- the GC of a key ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 21, 31, 32])
def test_gc_of_a_key_is_the_g_and_c_letters_of_its_kmer(k):
    rng = np.random.default_rng(k)
    kmers = ["A" * k, "C" * k, "G" * k, "T" * k, ("CG" * k)[:k], ("GC" * k)[:k], ("AT" * k)[:k], "T" + "A" * (k - 1), "G" + "A" * (k - 1),
             "C" + "T" * (k - 1), "A" * (k - 1) + "G"]
    kmers += ["".join("ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(300)]
    keys = np.array([ref.rank_of(s) for s in kmers], dtype=np.uint64)
    assert [ref.kmer_of(key, k) for key in keys] == kmers
    if k == 32:
        assert int(keys[3]) == 2**64 - 1 and sum(int(key) >> 63 for key in keys) > 100  # the top bit is in use
    else:
        assert int(keys.max()) < 4**k
    want = [s.count("G") + s.count("C") for s in kmers]
    assert ref.gc_of(keys).tolist() == want
    assert want[:6] == [0, k, k, 0, k, k] and want[6] == 0
    # the identity the library uses: a base is G or C exactly when its two bits differ
    xor = [bin((int(key) ^ (int(key) >> 1)) & 0x5555555555555555).count("1") for key in keys]
    assert xor == want
    # a k-mer and its reverse complement have one GC
    rc = ["".join("TGCA"["ACGT".index(b)] for b in reversed(s)) for s in kmers]
    assert ref.gc_of(np.array([ref.rank_of(s) for s in rc], dtype=np.uint64)).tolist() == want


def test_reference_matrix_and_gc_bounded_selection():
    k = 5
    kmers = ["AAAAA", "AAAAC", "ACGTA", "CCGGC", "CGCGC", "GGGGG", "TTTTT"]
    keys = np.array(sorted(ref.rank_of(s) for s in kmers), dtype=np.uint64)
    counts = np.array([1, 2, 2, 255, 9, 9, 1], dtype=np.uint8)
    gcs = ref.gc_of(keys).tolist()
    assert sorted(gcs) == [0, 0, 1, 2, 5, 5, 5]
    spec = ref.gc_spectrum(keys, counts, k)
    assert spec.shape == (6, 256) and int(spec.sum()) == 7 and not spec[:, 0].any()
    assert np.array_equal(spec.sum(axis=0), np.bincount(counts, minlength=256))
    for g, c in zip(gcs, counts):
        assert spec[g, c] >= 1
    assert ref.gc_spectrum(keys[:0], counts[:0], k).shape == (6, 256) and not ref.gc_spectrum(keys[:0], counts[:0], k).any()
    got = ref.select(keys, counts, (1, 255), (), db_select_ref.BASE, gc=(1, 4))
    inside = np.array([1 <= g <= 4 for g in gcs])
    assert np.array_equal(got[0], keys[inside]) and np.array_equal(got[1], counts[inside]) and int(got[2][0]) == int(inside.sum())
    whole = ref.select(keys, counts, (2, 255), [(keys[::2], counts[::2], (1, 255), db_select_ref.REQUIRE)], db_select_ref.SUM)
    plain = db_select_ref.select(keys, counts, (2, 255), [(keys[::2], counts[::2], (1, 255), db_select_ref.REQUIRE)], db_select_ref.SUM)
    assert all(np.array_equal(a, b) for a, b in zip(whole, plain))  # the default range is no bound


# ---- the summary lines ------------------------------------------------------------------------------------------------------------------
def test_summary_lines_of_a_hand_made_matrix(built):
    from trio_binning_amd import gc_spectrum as gs

    spec = np.zeros((4, 256), dtype=np.uint64)  # k = 3
    spec[0, 2], spec[0, 7], spec[0, 9] = 5, 5, 1          # a tie of the mode: the lowest counter
    spec[2, 1], spec[2, 30], spec[2, 255] = 100, 3, 2     # counter 1 lies below a range from 2 on; 255 is in it
    spec[3, 40] = 4                                       # row 1 stays empty
    lines = gs.summary(spec, (2, 255))
    assert lines[0] == "gc\tkmers\tshare\toccurrences\tmode\tmean"
    assert lines[1] == "0\t11\t{:.6f}\t54\t2\t{:.6f}".format(11 / 20, 54 / 11)
    assert lines[2] == "1\t0\t0.000000\t0\t-\t-"
    assert lines[3] == "2\t5\t0.250000\t600\t30\t120.000000"
    assert lines[4] == "3\t4\t0.200000\t160\t40\t40.000000"
    assert lines[5] == "#total\t20\t1.000000\t814\t2\t40.700000" and len(lines) == 6
    # the range moves what is counted: from 1 on row 2 has its once-seen k-mers and the total's mode is 1
    lines = gs.summary(spec, (1, 255))
    assert lines[3] == "2\t105\t{:.6f}\t700\t1\t{:.6f}".format(105 / 120, 700 / 105)
    assert lines[5] == "#total\t120\t1.000000\t914\t1\t{:.6f}".format(914 / 120)
    # a range of one counter, and one that holds nothing: every row empty, the shares of nothing
    assert gs.summary(spec, (7, 7))[1] == "0\t5\t1.000000\t35\t7\t7.000000"
    empty = gs.summary(spec, (100, 200))
    assert empty[1:] == ["{}\t0\tnan\t0\t-\t-".format(name) for name in (0, 1, 2, 3, "#total")]
    # sums that do not fit 64 bits stay exact
    big = np.zeros((2, 256), dtype=np.uint64)
    big[1, 255] = 2**60
    assert gs.summary(big, (1, 255))[2] == "1\t{}\t1.000000\t{}\t255\t255.000000".format(2**60, 255 * 2**60)


def test_matrix_file_there_and_back(built, tmp_path):
    from trio_binning_amd import gc_spectrum as gs

    rng = np.random.default_rng(3)
    for k, floor, compressed in ((21, 2, False), (32, 1, True), (1, 1, False)):
        spec = rng.integers(0, 2**40, (k + 1, 256)).astype(np.uint64)
        spec[:, 0] = 0
        spec[k, 255] = 2**64 - 1
        path = str(tmp_path / "gc{}.tsv".format(k))
        gs.write_matrix(path, spec, "lib.tbkdb", k, floor, compressed)
        assert not os.path.exists(path + ".tmp")
        head = [line for line in open(path) if line.startswith("#")]
        assert "lib.tbkdb" in head[1] and "k = {};".format(k) in head[2] and "floor = {}".format(floor) in head[2]
        assert ("homopolymer-compressed" if compressed else "plain") in head[2]
        assert sum(1 for line in open(path)) == len(head) + k + 1
        back = gs.read_matrix(path)
        assert back.dtype == np.uint64 and np.array_equal(back, spec)
    # a writer that fails leaves no half file and the one that was there
    with pytest.raises(ValueError):
        gs.write_matrix(path, np.zeros((5, 256), dtype=np.uint64), "lib.tbkdb", 1, 1, False)
    assert not os.path.exists(path + ".tmp") and np.array_equal(gs.read_matrix(path), spec)
    open(path, "w").write("# nothing\n1\t2\t3\n")
    with pytest.raises(ValueError, match="256"):
        gs.read_matrix(path)


# ---- refusals before a device is touched ----------------------------------------------------------------------------------------------
@pytest.fixture()
def dbs(tmp_path):
    files = {
        "full": full_file(k=21, seed=2)[0],
        "fullh": full_file(k=21, seed=2, magic=FULL_HPC)[0],
        "solid": kf.sound(k=21, n=40, seed=3)[0],
        "solid16": kf.sound(k=16, n=30, seed=4)[0],
        "damaged": kf.sound(k=21, n=40, seed=3)[0][:-3],
    }
    out = {"dir": str(tmp_path)}
    for name, data in files.items():
        out[name] = str(tmp_path / (name + ".tbkdb"))
        open(out[name], "wb").write(data)
    out["list"] = str(tmp_path / "hapA.txt")
    open(out["list"], "w").write("ACGTACGTACGTACGTACGTA\n")
    out["out"] = str(tmp_path / "picked.tbkdb")
    return out


def _refused(main, cases, capsys):
    with no_device():
        for argv, code, words in cases:
            with pytest.raises(SystemExit) as ei:
                main(argv)
            err = capsys.readouterr().err
            text = err if code == 2 else str(ei.value.code)
            assert (ei.value.code == 2) == (code == 2) and all(w in text for w in words), (argv, ei.value.code, err)
    assert capsys.readouterr().out == ""


def test_gc_spectrum_settles_a_sound_command_line_from_the_header(built, dbs):
    from trio_binning_amd import gc_spectrum as gs

    with no_device():
        a = gs.parse_args([dbs["solid"]])
        assert (a.range, a.matrix, a.info["k"], a.info["floor"]) == ((2, 255), None, 21, 2)  # a floor-2 file starts at 2
        a = gs.parse_args([dbs["full"]])
        assert (a.range, a.info["floor"]) == ((1, 255), 1)
        assert gs.parse_args([dbs["fullh"], "--max-count", "90"]).range == (1, 90)
        assert gs.parse_args([dbs["solid"], "--min-count", "1"]).range == (1, 255)
        assert gs.parse_args([dbs["solid16"], "--min-count", "255", "--max-count", "255", "--matrix", dbs["dir"] + "/m.tsv"]).range == (255, 255)
        with pytest.raises(AssertionError, match="the device was touched: KmerDatabase.load"):
            gs.main([dbs["solid"], "--matrix", dbs["dir"] + "/m.tsv"])
    assert not os.path.exists(dbs["dir"] + "/m.tsv")


def test_gc_spectrum_refuses_from_the_command_line_and_the_header(built, dbs, capsys):
    from trio_binning_amd import gc_spectrum as gs

    cases = (
        ([], 2, ["lib.tbkdb"]),
        ([dbs["list"]], 2, [dbs["list"], "not a count database", ".tbkdb"]),
        ([dbs["solid"] + "," + dbs["full"]], 2, ["not a count database"]),
        ([dbs["solid"], "--min-count", "0"], 2, ["--min-count 0", "1..255"]),
        ([dbs["solid"], "--max-count", "256"], 2, ["--max-count 256", "1..255"]),
        ([dbs["solid"], "--min-count", "-1"], 2, ["--min-count -1"]),
        ([dbs["solid"], "--min-count", "9", "--max-count", "8"], 2, ["--min-count 9 --max-count 8", "1 <= min <= max <= 255"]),
        ([dbs["solid"], "--max-count", "1"], 2, ["--min-count 2 --max-count 1"]),  # crossed against the floor the range starts at
        ([dbs["solid"], "--min-count", "x"], 2, ["--min-count"]),
        ([dbs["solid"], "--matrix", dbs["solid"]], 2, ["names the input"]),
        ([dbs["damaged"]], None, [dbs["damaged"], "gc_spectrum"]),
        ([dbs["solid"] + ".absent.tbkdb"], None, [".absent.tbkdb", "does not exist"]),
    )
    _refused(gs.main, cases, capsys)


def test_select_database_settles_and_refuses_gc_bounds(built, dbs, capsys):
    from trio_binning_amd import select_database as sd

    o = ["-o", dbs["out"]]
    with no_device():
        assert sd.parse_args(o + [dbs["full"]]).gc is None
        assert sd.parse_args(o + ["--min-gc", "8", dbs["full"]]).gc == (8, None)
        assert sd.parse_args(o + ["--max-gc", "0", dbs["full"]]).gc == (None, 0)
        assert sd.parse_args(o + ["--min-gc", "21", "--max-gc", "21", dbs["full"]]).gc == (21, 21)
        assert sd.parse_args(o + ["--min-gc", "0", "--max-gc", "16", dbs["solid16"]]).gc == (0, 16)
    assert (sd.gc_words(None, 21), sd.gc_words((8, None), 21), sd.gc_words((None, 9), 21)) == ("", " with 8..21 G-or-C bases", " with 0..9 G-or-C bases")
    cases = (
        (o + ["--min-gc", "-1", dbs["full"]], 2, ["--min-gc -1", "0..k"]),
        (o + ["--max-gc", "33", dbs["full"]], 2, ["--max-gc 33", "0..k"]),
        (o + ["--min-gc", "9", "--max-gc", "8", dbs["full"]], 2, ["--min-gc 9 --max-gc 8", "min <= max"]),
        (o + ["--min-gc", "22", dbs["full"]], 2, ["--min-gc 22", "21-mers", "0..21"]),           # in 0..32, above this file's k
        (o + ["--max-gc", "17", dbs["solid16"]], 2, ["--max-gc 17", "16-mers", "0..16"]),
        (o + ["--min-gc", "3", "--max-gc", "32", dbs["full"]], 2, ["--max-gc 32", "0..21"]),
        (o + ["--min-gc", "40%", dbs["full"]], 2, ["--min-gc"]),                                  # bases, not per cent
        (o + ["--min-gc", "3", dbs["damaged"]], None, [dbs["damaged"], "select_database"]),
    )
    _refused(sd.main, cases, capsys)
    assert not os.path.exists(dbs["out"])
