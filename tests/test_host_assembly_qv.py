"""What of the database query needs no device: kmers.qv, the refusals python -m trio_binning_amd.assembly_qv makes from its
arguments and the database's header alone (the entry points that would touch a device are replaced by ones that fail the test),
the absent-stretch helper on hand-built arrays, the new symbols of the built library, and tests/db_query_ref.py - the reference
of the GPU tests - held to the oracle on the repository's own test data."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import db_query_ref as ref
import kmerdb_files as kf
from conftest import DATA


# ---- kmers.qv ---------------------------------------------------------------------------------------------------------------------
def test_qv(built):
    from trio_binning_amd import kmers

    assert kmers.qv(0, 100, 21) == 0.0  # nothing found: an error rate of 1
    assert kmers.qv(100, 100, 21) == math.inf
    assert math.isnan(kmers.qv(0, 0, 21)) and math.isnan(kmers.qv(5, 0, 21))
    # by hand: found / clean = 2^-2 and k = 2 give 1 - 1/2: -10 log10(1/2) = 3.0103
    assert abs(kmers.qv(25, 100, 2) - 10 * math.log10(2)) < 1e-12
    # by hand: (999/1000)^(1/1) leaves 1e-3: QV 30
    assert abs(kmers.qv(999, 1000, 1) - 30.0) < 1e-9
    assert kmers.qv(990, 1000, 21) < kmers.qv(999, 1000, 21) < kmers.qv(999, 1000, 31)


def test_the_fixed_float_formats(built):
    from trio_binning_amd import assembly_qv as aq

    assert aq.format_qv(10, 10, 21) == "inf" and aq.format_qv(0, 0, 21) == "nan" and aq.format_qv(0, 10, 21) == "0.0000"
    assert aq.format_qv(999, 1000, 1) == "30.0000"
    assert aq.format_error_rate(999, 1000, 1) == "1.00000e-03" and aq.format_error_rate(5, 5, 21) == "0.00000e+00"
    assert aq.format_error_rate(0, 0, 21) == "nan"
    assert aq.format_completeness(1, 3) == "0.333333" and aq.format_completeness(0, 0) == "nan" and aq.format_completeness(4, 4) == "1.000000"


# ---- the absent-stretch helper -------------------------------------------------------------------------------------------------------
def _stretches(counts, clean):
    from trio_binning_amd import assembly_qv as aq

    first, last = aq.absent_stretches(np.array(counts, dtype=np.uint8), np.array(clean, dtype=bool))
    got = list(zip(first.tolist(), last.tolist()))
    assert got == ref.absent_stretches(counts, clean)
    return got


def test_absent_stretches(built):
    assert _stretches([], []) == []
    assert _stretches([3, 3, 3], [1, 1, 1]) == []
    assert _stretches([0, 0, 0], [1, 1, 1]) == [(0, 2)]
    assert _stretches([0, 5, 0, 0, 9, 0], [1, 1, 1, 1, 1, 1]) == [(0, 0), (2, 3), (5, 5)]
    # a window that is not clean is not absent, and it ends a stretch
    assert _stretches([0, 0, 0, 0, 0], [1, 1, 0, 1, 1]) == [(0, 1), (3, 4)]
    assert _stretches([0, 0, 0], [0, 0, 0]) == []
    # counts runs to the sequence's end (k - 1 bytes more than there are windows)
    assert _stretches([7, 0, 0, 0, 0], [1, 1, 1]) == [(1, 2)]


def test_clean_windows(built):
    from trio_binning_amd import assembly_qv as aq

    s = b"ACGTNacgtACXT"
    got = aq.clean_windows(np.frombuffer(s, dtype=np.uint8), 3)
    want = [km is not None for km in ref.window_kmers(s.decode(), 3)]
    assert got.tolist() == want and sum(want) == 6  # ACG CGT, acg cgt gtA tAC
    assert aq.clean_windows(np.frombuffer(b"AC", dtype=np.uint8), 3).size == 0


# ---- the command line's refusals ----------------------------------------------------------------------------------------------------
@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "reads.tbkdb"), "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"),
             "bed": str(tmp_path / "absent.bed"), "spectrum": str(tmp_path / "spectrum.tsv")}
    with open(paths["db"], "wb") as fh:
        fh.write(kf.sound(k=21, n=5, seed=1)[0])

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.DatabaseQuery, "__init__", touched)
    return paths


def _exit(files, argv):
    from trio_binning_amd import assembly_qv

    with pytest.raises(SystemExit) as ei:
        assembly_qv.main(argv + ["--absent-bed", files["bed"], "--spectrum", files["spectrum"]])
    for out in (files["bed"], files["spectrum"]):
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    return ei.value.code


@pytest.mark.parametrize("missing", ["assembly", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "assembly" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("assembly_qv: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("assembly_qv: ") and files["list"] in code
    assert "is not a count database" in code and "k-mer list holds no counts" in code and "--keep-databases" in code
    assert capsys.readouterr().out == ""


def test_a_damaged_database_is_refused_by_its_header(files, capsys, tmp_path):
    bad = tmp_path / "bad.tbkdb"
    bad.write_bytes(kf.patched(kf.sound(k=21, n=5, seed=1)[0], 0, b"TBKKMDB2"))
    code = _exit(files, [files["fa"], str(bad)])
    assert isinstance(code, str) and code.startswith("assembly_qv: ") and str(bad) in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("option", ["--min-count", "--max-count"])
@pytest.mark.parametrize("value", ["1", "0", "256", "-4"])
def test_a_count_outside_2_to_255_is_refused(files, capsys, option, value):
    code = _exit(files, [files["fa"], files["db"], option, value])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and option in err and "2 <= N <= 255" in err


def test_min_above_max_is_refused(files, capsys):
    code = _exit(files, [files["fa"], files["db"], "--min-count", "10", "--max-count", "9"])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count 10 is larger than --max-count 9" in err


def test_sound_arguments_reach_the_database(files):
    """the fixture's tripwire is what a sound command line meets first: nothing above was refused for another reason"""
    from trio_binning_amd import assembly_qv

    args = assembly_qv.parse_args([files["fa"], files["db"], "--min-count", "3", "--max-count", "200"])
    assert args.info["k"] == 21 and args.info["n"] == 5 and (args.min_count, args.max_count) == (3, 200)
    with pytest.raises(AssertionError, match="the device was touched"):
        assembly_qv.main([files["fa"], files["db"]])


def test_help_states_the_deviation_from_merqury(built, capsys):
    from trio_binning_amd import assembly_qv

    with pytest.raises(SystemExit) as ei:
        assembly_qv.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "lower bound of Merqury's" in text and "four decimals" in text


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_and_their_signatures(built):
    from trio_binning_amd import _lib

    assert _lib.HAS_DB_QUERY and _lib.lib.tbk_abi_version() == 1
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    want = {
        "tbk_kmerdb_query_create": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
        "tbk_kmerdb_query_destroy": (None, [vp]),
        "tbk_kmerdb_query_add": (C.c_int, [vp, vp, vp, u64, u32, vp, vp]),
        "tbk_kmerdb_query_histogram": (C.c_int, [vp, vp]),
        "tbk_kmerdb_query_completeness": (C.c_int, [vp, u32, u32, C.POINTER(u64), C.POINTER(u64)]),
        "tbk_kmerdb_query_copy_spectrum": (C.c_int, [vp, vp]),
        "tbk_kmerdb_query_reset": (C.c_int, [vp]),
    }
    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    for name, (restype, argtypes) in want.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
        assert name + "(" in header
    # NULL handles are refused without a device
    out = vp()
    assert _lib.lib.tbk_kmerdb_query_create(None, 0, C.byref(out)) == -1 and not out.value
    assert _lib.lib.tbk_kmerdb_query_add(None, None, None, 0, 2, None, None) == -1
    assert _lib.lib.tbk_kmerdb_query_reset(None) == -1
    _lib.lib.tbk_kmerdb_query_destroy(None)
    import trio_binning.assembly_qv as alias
    import trio_binning_amd.assembly_qv as impl

    assert alias is impl or alias.main is impl.main


def test_the_grid_hooks_are_no_part_of_the_header_and_refuse_null(built):
    from trio_binning_amd import _lib

    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    for name in ("tbk_kmerdb_query_set_wave_slots_", "tbk_hit_tracker_set_wave_slots_"):
        fn = getattr(_lib.lib, name)
        assert fn.restype == C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_uint64] and name not in header
        assert fn(None, 3) == _lib.TBK_ERR_INVALID and fn(None, 0) == _lib.TBK_ERR_INVALID


# ---- the reference of the GPU tests against the oracle -------------------------------------------------------------------------------
def _fastq_reads(path):
    return [line.strip() for i, line in enumerate(open(path)) if i % 4 == 1]


@pytest.mark.parametrize("k", [5, 21, 32])
def test_db_query_ref_agrees_with_the_oracle(k):
    from oracle import unique_oracle as uo

    reads = _fastq_reads(os.path.join(DATA, "hapA.fastq"))[:40] + ["acgtnACGT" * 9, "N" * 50, "", "A" * 300]
    assert sum(len(r) for r in reads) > 5000
    occurrences = uo.count_kmers(reads, k)
    db = uo.database(occurrences)
    tally = ref.Tally(db)
    per_read, counts = tally.add(reads, k)
    # every window's k-mer is the oracle's canonical one, and its counter the database's
    at = 0
    for r, s in enumerate(reads):
        windows = ref.window_kmers(s, k)
        assert len(windows) == max(len(s) - k + 1, 0)
        for w, km in enumerate(windows):
            text = s[w:w + k].upper()
            if km is None:
                assert any(c not in "ACGT" for c in text) and counts[at + w] == 0
            else:
                assert km == uo.canonical(text) and int(counts[at + w]) == db.get(km, 0)
        assert int(per_read[r, 0]) == sum(km is not None for km in windows)
        at += len(s)
    # the tally is the oracle's count, seen from the windows' side
    assert int(tally.hist.sum()) == sum(occurrences.values()) == int(per_read[:, 0].sum())
    assert int(tally.hist[0]) == sum(1 for n in occurrences.values() if n == 1)
    for c in range(2, 256):
        assert int(tally.hist[c]) == sum(n for n in occurrences.values() if min(n, 255) == c and n >= 2)
    assert tally.copies == {km: occurrences[km] for km in db}
    assert tally.completeness() == (len(db), len(db)) and int(per_read[:, 1].sum()) == int(tally.hist[2:].sum())
    spec = tally.spectrum()
    assert int(spec.sum()) == len(db) and int(spec[0].sum()) == int(spec[1].sum()) == 0
    # ranks order as the k-mers do, and a crafted file is a sound database holding them
    kmers_sorted = sorted(db)
    assert [ref.lex_rank(km) for km in kmers_sorted] == sorted(ref.lex_rank(km) for km in db)
    data = ref.database_bytes(db, k)
    assert len(data) == kf.HEADER + 9 * len(db)
    keys_np, counts_np = uo.count_kmers_np(*uo.pack(reads), k)
    held = kf.database_of(keys_np, counts_np)
    assert np.array_equal(np.frombuffer(data[kf.HEADER:kf.HEADER + 8 * len(db)], dtype="<u8"), held[0])
    assert np.array_equal(np.frombuffer(data[kf.HEADER + 8 * len(db):], dtype=np.uint8), held[1])
