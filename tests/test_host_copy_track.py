"""What of the copy-number track needs no device: the two references of tests/copy_track_ref.py held to each other and to a
case worked by hand, the refusals python -m trio_binning_amd.copy_track makes from its arguments and the database's header
alone, its default peak, and the new symbol's signature."""
import ctypes as C
import os

import numpy as np
import pytest

import copy_track_ref as ctr
import db_query_ref as ref
import kmerdb_files as kf
from conftest import DATA


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _pack(sequences):
    """(bases, offsets) as kmers.pack_reads gives them, without the library"""
    bases = np.frombuffer("".join(sequences).encode(), dtype=np.uint8)
    offsets = np.zeros(len(sequences) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in sequences], out=offsets[1:])
    return bases, offsets


def _both(db, k):
    ranks = np.array(sorted(ref.lex_rank(km) for km in db), dtype=np.uint64)
    by_rank = {ref.lex_rank(km): c for km, c in db.items()}
    return ref.Tally(db), ref.TallyNp(ranks, np.array([by_rank[int(r)] for r in ranks], dtype=np.uint8))


# ---- the two references ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_the_two_references_agree(seed):
    rng = np.random.default_rng(4100 + seed)
    k = int(rng.choice((4, 5, 6, 21, 32)))
    genome = _seq(rng, int(rng.integers(80, 400)))
    held = [km for km in ref.window_kmers(genome, k) if km is not None and rng.integers(0, 5)]
    db = {km: int(rng.choice((2, 5, 10, 15, 20, 30, 254, 255))) for km in held}
    contigs = []
    for _ in range(int(rng.integers(1, 7))):
        n = int(rng.integers(0, len(genome)))
        p = int(rng.integers(0, len(genome) - n + 1))
        c = list(genome[p:p + n])
        if c and rng.integers(0, 2):
            c[int(rng.integers(0, len(c)))] = "N"
        if c and rng.integers(0, 2):
            at = int(rng.integers(0, len(c)))
            c[at:at + 9] = [x.lower() for x in c[at:at + 9]]
        contigs.append(ref.revcomp("".join(c).upper()) if rng.integers(0, 3) == 0 else "".join(c))
    contigs += ["", genome[:k - 1], genome[:k]]
    loop, fast = _both(db, k)
    bases, offsets = _pack(contigs)
    for added in range(3):  # never added (a = 0), once, twice
        before = (loop.hist.copy(), dict(loop.copies), fast.hist.copy(), fast.copies.copy())
        for window in (1, 2, 7, 64, 1 << 31):
            for peak in (1, 10, 254):
                want, want_prefix = ctr.as_array(ctr.track(loop, contigs, k, window, peak))
                got, prefix = ctr.track_np(fast, bases, offsets, k, window, peak)
                assert np.array_equal(prefix, want_prefix)
                assert ctr.equal(got, want), (k, window, peak, added, ctr.first_difference(got, want))
        assert np.array_equal(loop.hist, before[0]) and loop.copies == before[1]  # a track only reads
        assert np.array_equal(fast.hist, before[2]) and np.array_equal(fast.copies, before[3])
        loop.add(contigs, k)
        fast.add(bases, offsets, k)


# ---- a case worked by hand ---------------------------------------------------------------------------------------------------------
# k = 5, peak = 10, W = 8.  S has 32 windows, all of different canonical 5-mers.  The reads' counter by window of S:
#   0..5    10    a unique stretch at the one-copy depth
#   6..9    20    held once, read twice as deep: collapsed (40 > 3 x 10)
#   10      15    a tie: 30 > 30 is false, not collapsed
#   11       5    a tie: 10 < 10 is false, not expanded
#   12     255    saturated: no verdict
#   13..16  10    the stretch S[13:21], which the second contig holds again: a = 2, expanded (20 < 3 x 10)
#   17       -    not in the database: absent
#   18..31  10
# The second contig is S[13:21], an N and four bases: nine window starts, of which 0..3 are clean (the stretch's four
# k-mers) and 4..8 hold the N.
HAND_S = "CGGCTCGCCTAGCGTCGGCAGATTTATTGTTTAACA"
HAND_C = [10] * 6 + [20] * 4 + [15, 5, 255] + [10] * 4 + [0] + [10] * 14
HAND_SECOND = HAND_S[13:21] + "N" + "ACGT"
HAND_WANT = [
    # clean absent saturated collapsed expanded depth copies
    [(8, 0, 0, 2, 0, 10, 1),   # windows 0..7: 10 x 6, 20 x 2
     (8, 0, 1, 2, 3, 10, 1),   # 8..15: c = 20 20 15 5 255 10 10 10, a = 1 1 1 1 1 2 2 2: sorted c[3] = 10, sorted a[3] = 1
     (8, 1, 0, 0, 1, 10, 1),   # 16..23: one expanded, one absent, six plain: seven present, sorted a = 1 x 6, 2
     (8, 0, 0, 0, 0, 10, 1)],  # 24..31
    [(4, 0, 0, 0, 4, 10, 2),   # the stretch again: four present windows, a = 2
     (0, 0, 0, 0, 0, 0, 0)],   # window 8 alone, over the N: a last bin of one window, nothing clean
]


def _hand():
    windows = ref.window_kmers(HAND_S, 5)
    assert len(windows) == 32 == len(HAND_C) and len(set(windows)) == 32 and None not in windows
    return {km: c for km, c in zip(windows, HAND_C) if c}


def test_the_hand_worked_case():
    db = _hand()
    contigs = [HAND_S, HAND_SECOND]
    assert [km is not None for km in ref.window_kmers(HAND_SECOND, 5)] == [True] * 4 + [False] * 5
    loop, fast = _both(db, 5)
    loop.add(contigs, 5)
    fast.add(*_pack(contigs), 5)
    got = ctr.track(loop, contigs, 5, 8, 10)
    assert [[tuple(b[f] for f in ctr.FIELDS) for b in bins] for bins in got] == HAND_WANT
    arr, prefix = ctr.track_np(fast, *_pack(contigs), 5, 8, 10)
    assert prefix.tolist() == [0, 4, 6] and ctr.equal(arr, ctr.as_array(got)[0])
    # the ties by themselves, and one step to either side of them
    assert ctr.verdicts(15, 1, 10) == (False, False) and ctr.verdicts(5, 1, 10) == (False, False)
    assert ctr.verdicts(16, 1, 10) == (True, False) and ctr.verdicts(4, 1, 10) == (False, True)
    assert ctr.verdicts(255, 1, 10) == (False, False) and ctr.verdicts(254, 1, 10) == (True, False)
    assert ctr.verdicts(1, 0, 10) == (False, False) and ctr.verdicts(6, 0, 10) == (True, False)  # a = 0: never expanded
    # what the command writes of it
    out, track = ctr.command_tables(["S", "second"], [36, 13], got, 8, 10)
    assert out == "S\t36\t32\t1\t1\t4\t4\nsecond\t13\t4\t0\t0\t0\t4\n#total\t49\t36\t1\t1\t4\t8\t10\t8\n"
    assert track.splitlines()[3] == "S\t24\t36\t8\t0\t0\t10\t1\t0\t0" and track.splitlines()[5] == "second\t8\t13\t0\t0\t0\t0\t0\t0\t0"


def test_lower_median():
    assert ctr.lower_median([]) == 0 and ctr.lower_median([7]) == 7 and ctr.lower_median([9, 3]) == 3
    assert ctr.lower_median([5, 1, 9]) == 5 and ctr.lower_median([4, 1, 9, 6]) == 4


# ---- the command line's refusals ------------------------------------------------------------------------------------------------------
def _database_with(hist_rows, k=21):
    """the bytes of a sound database whose header holds these rows 2..255 ({counter: k-mers}); row 1 is made up"""
    hist = np.zeros(256, dtype=np.uint64)
    for c, n in hist_rows.items():
        hist[c] = n
    counts = np.repeat(np.arange(256), hist.astype(np.int64)).astype(np.uint8)
    keys = np.arange(counts.size, dtype=np.uint64) * np.uint64(977)
    hist[1] = 10 ** 6
    hist[0] = counts.size + 10 ** 6
    return kf.file_bytes(k, keys, counts, hist, reads=3, bases=99), hist


PEAKED = {2: 100, 3: 50, 4: 30, 5: 40, 6: 60, 7: 70, 8: 80, 9: 85, 10: 90, 11: 90, 12: 70, 13: 50, 14: 35, 15: 20, 16: 95}
FALLING = {c: 300 - c for c in range(2, 256)}


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "reads.tbkdb"), "falling": str(tmp_path / "falling.tbkdb"), "hpc": str(tmp_path / "hpc.tbkdb"),
             "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"), "track": str(tmp_path / "track.tsv")}
    with open(paths["db"], "wb") as fh:
        fh.write(_database_with(PEAKED)[0])
    with open(paths["falling"], "wb") as fh:
        fh.write(_database_with(FALLING)[0])
    _, keys, counts, hist = kf.sound(k=21, n=5, seed=1)
    with open(paths["hpc"], "wb") as fh:
        fh.write(kf.file_bytes(21, keys, counts, hist, reads=11, bases=1234, magic=b"TBKKMDH1"))

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.DatabaseQuery, "__init__", touched)
    return paths


def _exit(files, argv):
    from trio_binning_amd import copy_track

    with pytest.raises(SystemExit) as ei:
        copy_track.main(argv + ["--track", files["track"]])
    assert not os.path.exists(files["track"]) and not os.path.exists(files["track"] + ".tmp")
    return ei.value.code


@pytest.mark.parametrize("missing", ["assembly", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "assembly" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("copy_track: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("copy_track: ") and files["list"] in code
    assert "is not a count database" in code and "k-mer list holds no counts" in code and "--keep-databases" in code
    assert capsys.readouterr().out == ""


def test_a_compressed_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["hpc"], "--peak", "10"])
    assert isinstance(code, str) and code.startswith("copy_track: ") and files["hpc"] in code
    assert "holds homopolymer-compressed k-mers (find-unique-kmers --compress)" in code and "Give a plain database." in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("value", ["0", "-1"])
def test_a_window_below_1_is_refused(files, capsys, value):
    code = _exit(files, [files["fa"], files["db"], "--window", value])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--window" in err and "1 <= W" in err


@pytest.mark.parametrize("value", ["0", "255", "-3", "1000"])
def test_a_peak_outside_1_to_254_is_refused(files, capsys, value):
    code = _exit(files, [files["fa"], files["db"], "--peak", value])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--peak" in err and "1 <= N <= 254" in err


def test_sound_arguments_reach_the_database(files, capsys):
    """the fixture's tripwire is what a sound command line meets first: nothing above was refused for another reason"""
    from trio_binning_amd import copy_track

    args = copy_track.parse_args([files["fa"], files["db"], "--window", "1", "--peak", "254"])
    assert args.info["k"] == 21 and (args.window, args.peak, args.track) == (1, 254, None)
    assert copy_track.parse_args([files["fa"], files["db"], "--peak", "1"]).window == 10000
    assert capsys.readouterr().err == ""  # a given peak is not announced
    with pytest.raises(AssertionError, match="the device was touched"):
        copy_track.main([files["fa"], files["db"], "--track", files["track"]])
    assert not os.path.exists(files["track"] + ".tmp")


# ---- the default peak --------------------------------------------------------------------------------------------------------------------
def test_the_default_peak_of_a_made_up_histogram(files, capsys):
    """PEAKED falls to row 4 (30 k-mers) and rises from row 5: lo = 4.  Row 15 (20) is the first behind it below 30: hi = 15.
    In [4, 15] rows 10 and 11 tie at 90: the lower counter wins.  Row 16 (95) lies outside, and so does row 1, however full."""
    from trio_binning_amd import copy_track, find_unique_kmers as fu

    hist = _database_with(PEAKED)[1]
    rows = [(c, 0 if c == 1 else int(hist[c])) for c in range(1, 256)]
    assert fu.analyze_histogram(rows, "made up") == (4, 15)
    assert copy_track.default_peak({"histogram": hist}, "made up") == 10
    lone = hist.copy()
    lone[11] = 91
    assert copy_track.default_peak({"histogram": lone}, "made up") == 11
    capsys.readouterr()
    args = copy_track.parse_args([files["fa"], files["db"]])
    assert args.peak == 10 and "Using 10 as the one-copy read depth" in capsys.readouterr().err


def test_a_histogram_without_a_peak_asks_for_the_option(files, capsys):
    code = _exit(files, [files["fa"], files["falling"]])
    assert isinstance(code, str) and code.startswith("copy_track: ") and files["falling"] in code and "--peak" in code
    from trio_binning_amd import copy_track

    assert copy_track.parse_args([files["fa"], files["falling"], "--peak", "30"]).peak == 30  # given by hand, the histogram is not asked


def test_help_says_that_no_verdict_is_computed(built, capsys):
    from trio_binning_amd import copy_track

    with pytest.raises(SystemExit) as ei:
        copy_track.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "No verdict on the assembly is computed" in text and "heterozygous (one-copy) peak" in text


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_its_signature_and_its_struct(built):
    from trio_binning_amd import _lib, kmers

    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    fn = _lib.lib.tbk_kmerdb_query_track
    assert _lib.HAS_DB_TRACK and fn.restype == C.c_int and list(fn.argtypes) == [vp, vp, vp, u64, u32, u32, vp, u64]
    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    assert "tbk_kmerdb_query_track(" in header and "typedef struct tbk_depth_bin" in header
    assert fn(None, None, None, 0, 1, 1, None, 0) == _lib.TBK_ERR_INVALID  # a NULL handle is refused without a device
    assert kmers.DEPTH_BIN == ctr.BIN and kmers.DEPTH_BIN.itemsize == 24
    assert [kmers.DEPTH_BIN.fields[f][1] for f in ctr.FIELDS] == [0, 4, 8, 12, 16, 20, 21]
