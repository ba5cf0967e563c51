"""What of python -m trio_binning_amd.repair_candidates needs no device: the refusals it makes from its arguments and the
database's header alone, its defaults, the --edits lines, the application of the edits with its conflict rule, and the new
symbol's signature."""
import ctypes as C
import os

import numpy as np
import pytest

import kmerdb_files as kf
import repair_ref as rr
from conftest import DATA


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    from trio_binning_amd import kmers

    paths = {"db": str(tmp_path / "reads.tbkdb"), "full": str(tmp_path / "full.tbkdb"), "hpc": str(tmp_path / "hpc.tbkdb"),
             "list": os.path.join(DATA, "hapA.txt"), "fa": os.path.join(DATA, "test.fa"), "edits": str(tmp_path / "edits.tsv"),
             "apply": str(tmp_path / "mended.fa")}
    _, keys, counts, hist = kf.sound(k=21, n=5, seed=1)
    full_hist = np.bincount(counts, minlength=256).astype(np.uint64)  # (a full database's row 1 counts entries, row 0 all of them)
    full_hist[0] = counts.size
    for name, magic, rows in (("db", kf.MAGIC, hist), ("hpc", b"TBKKMDH1", hist), ("full", b"TBKKMFB1", full_hist)):
        with open(paths[name], "wb") as fh:
            fh.write(kf.file_bytes(21, keys, counts, rows, reads=11, bases=1234, magic=magic))

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.DatabaseQuery, "__init__", touched)
    return paths


def _exit(files, argv):
    from trio_binning_amd import repair_candidates

    with pytest.raises(SystemExit) as ei:
        repair_candidates.main(argv + ["--edits", files["edits"], "--apply", files["apply"]])
    for out in (files["edits"], files["apply"]):
        assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    return ei.value.code


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", ["assembly", "database"])
def test_a_missing_file_is_refused(files, capsys, tmp_path, missing):
    gone = str(tmp_path / ("nothing.tbkdb" if missing == "database" else "nothing.fa"))
    code = _exit(files, [gone, files["db"]] if missing == "assembly" else [files["fa"], gone])
    assert isinstance(code, str) and code.startswith("repair_candidates: ") and gone in code and "does not exist" in code
    assert capsys.readouterr().out == ""


def test_a_list_in_place_of_the_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["list"]])
    assert isinstance(code, str) and code.startswith("repair_candidates: ") and files["list"] in code
    assert "is not a count database" in code and "k-mer list holds no counts" in code and "--keep-databases" in code
    assert capsys.readouterr().out == ""


def test_a_compressed_database_is_refused_in_words(files, capsys):
    code = _exit(files, [files["fa"], files["hpc"]])
    assert isinstance(code, str) and code.startswith("repair_candidates: ") and files["hpc"] in code
    assert "holds homopolymer-compressed k-mers (find-unique-kmers --compress)" in code and "Give a plain database." in code
    assert capsys.readouterr().out == ""


def test_presence_needs_a_full_database(files, capsys):
    from trio_binning_amd import repair_candidates

    code = _exit(files, [files["fa"], files["db"], "--min-count", "1"])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and "--min-count 1" in err and "--keep-singletons" in err
    assert repair_candidates.parse_args([files["fa"], files["full"], "--min-count", "1"]).min_count == 1


@pytest.mark.parametrize("option, value", [("--min-count", "0"), ("--min-count", "256"), ("--min-count", "-2"), ("--min-support", "0"),
                                           ("--min-support", "33"), ("--min-support", "-1")])
def test_values_out_of_range_are_refused(files, capsys, option, value):
    code = _exit(files, [files["fa"], files["db"], option, value])
    out, err = capsys.readouterr()
    assert code == 2 and out == "" and option in err and "<= N <=" in err


def test_sound_arguments_reach_the_database(files, capsys):
    """the fixture's tripwire is what a sound command line meets first: nothing above was refused for another reason"""
    from trio_binning_amd import repair_candidates

    args = repair_candidates.parse_args([files["fa"], files["db"]])
    assert args.info["k"] == 21 and (args.min_count, args.min_support, args.edits, args.apply) == (2, 11, None, None)  # (k + 1) // 2
    args = repair_candidates.parse_args([files["fa"], files["db"], "--min-count", "255", "--min-support", "32"])
    assert (args.min_count, args.min_support) == (255, 32)
    with pytest.raises(AssertionError, match="the device was touched"):
        repair_candidates.main([files["fa"], files["db"], "--edits", files["edits"], "--apply", files["apply"]])
    assert not os.path.exists(files["edits"] + ".tmp") and not os.path.exists(files["apply"] + ".tmp")


def test_help_says_that_no_verdict_is_computed(built, capsys):
    from trio_binning_amd import repair_candidates

    with pytest.raises(SystemExit) as ei:
        repair_candidates.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert ei.value.code == 0 and "No verdict on the assembly is computed" in text and "(k + 1) // 2" in text


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def _records(*tuples):
    return rr.as_array(list(tuples))


def test_the_edit_lines(built):
    from trio_binning_amd import repair_candidates as rc

    sequence = np.frombuffer(b"ACgtNACGT", dtype=np.uint8)
    records = _records((0, 0, 2, 3, 1, rr.SUB, ord("T"), 3, 9), (0, 1, 3, 2, 2, rr.DEL, 0, 2, 255), (0, 2, 5, 1, 1, rr.INS, ord("C"), 1, 2),
                       (0, 3, 0, 4, 0, rr.NONE, 0, 0, 0), (0, 4, 0, 40, 0, rr.LONG, 0, 0, 0))
    assert [rc.verdict(r) for r in records] == ["mended", "ambiguous", "mended", "unmended", "long"]
    assert [rc.edit_line("ctg 1", sequence, r) for r in records] == [
        "ctg 1\t0\t3\tmended\tsub\t2\tG\tT\t1\t3\t9\n",  # ref is the sequence's base, folded to upper case
        "ctg 1\t1\t2\tambiguous\tdel\t3\tT\t.\t2\t2\t255\n",
        "ctg 1\t2\t1\tmended\tins\t5\t.\tC\t1\t1\t2\n",
        "ctg 1\t3\t4\tunmended\t.\t.\t.\t.\t0\t0\t0\n",
        "ctg 1\t4\t40\tlong\t.\t.\t.\t.\t0\t0\t0\n"]
    assert len(rc.EDIT_COLUMNS) == 11 and len(rc.TSV_COLUMNS) == 7


# ---- the application -----------------------------------------------------------------------------------------------------------------
def test_apply_an_insertion_and_a_deletion_and_keep_the_case(built):
    from trio_binning_amd import repair_candidates as rc

    #             0123456789012345678901234
    sequence = b"acgtACGTnnACGTacgtACGTacg"
    records = _records((0, 0, 2, 3, 1, rr.SUB, ord("T"), 3, 9),    # g -> T: the new base is upper case
                       (0, 7, 9, 2, 1, rr.DEL, 0, 2, 9),           # the second n goes
                       (0, 14, 16, 1, 1, rr.INS, ord("A"), 1, 9),  # an A in front of base 16
                       (0, 20, 23, 1, 3, rr.SUB, ord("A"), 1, 9),  # ambiguous: never applied
                       (0, 21, 0, 1, 0, rr.NONE, 0, 0, 0), (0, 22, 0, 50, 0, rr.LONG, 0, 0, 0))
    fixed, applied, conflicting = rc.apply_edits(sequence, records, 5)
    assert (fixed, applied, conflicting) == (b"acTtACGTnACGTacAgtACGTacg", 3, 0)
    want = rr.apply_edits(sequence.decode(), [(rr.SUB, 2, "T"), (rr.DEL, 9, ""), (rr.INS, 16, "A")])
    assert fixed.decode() == want and len(fixed) == len(sequence)
    assert rc.apply_edits(sequence, records[:0], 5) == (sequence, 0, 0) and rc.apply_edits(b"", records[:0], 5) == (b"", 0, 0)


def test_the_conflict_rule(built):
    from trio_binning_amd import repair_candidates as rc

    sequence = b"A" * 60
    sub = lambda pos, accepted=1: (0, pos, pos, 1, accepted, rr.SUB, ord("C"), 1, 9)  # noqa: E731
    # 10 and 14 are fewer than 5 apart: neither is applied; 20 and 25 are exactly k apart: both are
    fixed, applied, conflicting = rc.apply_edits(sequence, _records(sub(10), sub(14), sub(20), sub(25)), 5)
    assert (applied, conflicting) == (2, 2) and fixed == b"A" * 20 + b"CAAAAC" + b"A" * 34
    # a chain: 30, 33, 36 - the middle one conflicts with both, and all three stay out; an ambiguous neighbour does not count
    fixed, applied, conflicting = rc.apply_edits(sequence, _records(sub(30), sub(33), sub(36), sub(50), sub(52, accepted=2)), 5)
    assert (applied, conflicting) == (1, 3) and fixed == b"A" * 50 + b"C" + b"A" * 9
    # kinds mix: an insertion in front of base 12 and a deletion of base 15
    mixed = _records((0, 8, 12, 1, 1, rr.INS, ord("G"), 1, 9), (0, 11, 15, 1, 1, rr.DEL, 0, 1, 9))
    assert rc.apply_edits(sequence, mixed, 5) == (sequence, 0, 2) and rc.apply_edits(sequence, mixed, 3)[1:] == (2, 0)


# ---- the library ------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_its_signature_and_its_struct(built):
    from trio_binning_amd import _lib, kmers

    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    fn = _lib.lib.tbk_kmerdb_query_repairs
    assert _lib.HAS_DB_REPAIRS and fn.restype == C.c_int
    assert list(fn.argtypes) == [vp, vp, vp, u64, u32, u32, C.POINTER(vp), C.POINTER(u64)]
    header = open(os.path.join(os.path.dirname(DATA), "..", "include", "tbk.h")).read()
    assert "tbk_kmerdb_query_repairs(" in header and "typedef struct tbk_repair" in header and "repair candidates" in header
    ptr, count = vp(), u64()
    assert fn(None, None, None, 0, 2, 1, C.byref(ptr), C.byref(count)) == _lib.TBK_ERR_INVALID  # a NULL handle is refused without a device
    assert kmers.REPAIR == rr.REPAIR and kmers.REPAIR.itemsize == 40
    assert [kmers.REPAIR.fields[f][1] for f in rr.FIELDS] == [0, 8, 16, 24, 28, 30, 31, 32, 33]
    assert (kmers.REPAIR_NONE, kmers.REPAIR_SUB, kmers.REPAIR_DEL, kmers.REPAIR_INS, kmers.REPAIR_LONG) == (rr.NONE, rr.SUB, rr.DEL, rr.INS, rr.LONG)
