"""select_database and hapmers without a GPU: every refusal of the two command lines comes from the arguments and from crafted
headers (tests/kmerdb_files.py) alone, before a database is loaded - ``kmers.KmerDatabase.load`` and the library's device
entry points are patched to fail the test if they are reached - and a sound command line is settled and goes on to the device."""
import contextlib
import os
from unittest.mock import patch

import pytest

import kmerdb_files as kf
from test_host_kmerdb_full import FULL_HPC, full_file

DEVICE_ENTRIES = ("tbk_kmerdb_load", "tbk_kmerdb_solid", "tbk_kmerdb_select", "tbk_kmerdb_save", "tbk_kmerdb_origin_spectrum")


@contextlib.contextmanager
def no_device():
    """loading a database, and every device entry point either command could reach, raises"""
    from trio_binning_amd import _lib, kmers

    def reached(*args, **kw):
        raise AssertionError("the device was touched: KmerDatabase.load")

    with contextlib.ExitStack() as stack:
        stack.enter_context(patch.object(kmers.KmerDatabase, "load", reached))
        for name in DEVICE_ENTRIES:
            stack.enter_context(patch.object(_lib.lib, name, side_effect=AssertionError("the device was touched: " + name)))
        yield


@pytest.fixture()
def dbs(tmp_path):
    files = {
        "full": full_file(k=21, seed=2)[0],
        "full16": full_file(k=16, seed=2)[0],
        "fullh": full_file(k=21, seed=2, magic=FULL_HPC)[0],
        "solid": kf.sound(k=21, n=40, seed=3)[0],
        "solid2": kf.sound(k=21, n=30, seed=4)[0],
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


# ---- select_database ------------------------------------------------------------------------------------------------------------
def test_partner_specs():
    from trio_binning_amd.select_database import partner_spec

    assert partner_spec("a.tbkdb") == ("a.tbkdb", 1, 255)
    assert partner_spec("a.tbkdb:2") == ("a.tbkdb", 2, 255)
    assert partner_spec("a.tbkdb:5:35") == ("a.tbkdb", 5, 35)
    assert partner_spec("dir:1/a.tbkdb:5:35") == ("dir:1/a.tbkdb", 5, 35)
    assert partner_spec("x:1:2:3") == ("x:1", 2, 3)
    assert partner_spec("a.tbkdb:0:256") == ("a.tbkdb", 0, 256)  # (refused later, as a range)
    assert partner_spec("a.tbkdb:-1") == ("a.tbkdb:-1", 1, 255)   # (no file of that name)
    assert partner_spec("7") == ("7", 1, 255)


def test_a_sound_selection_is_settled_from_the_headers(built, dbs):
    from trio_binning_amd import select_database as sd

    with no_device():
        a = sd.parse_args(["-o", dbs["out"], dbs["full"]])
        assert (a.min_count, a.max_count, a.counter, a.partners, a.info["k"], a.info["floor"]) == (1, 255, "base", [], 21, 1)
        a = sd.parse_args(["-o", dbs["out"], "--min-count", "3", "--max-count", "90", "--exclude", dbs["solid"] + ":2", "--require",
                           dbs["full"] + ":5:35", "--counter", "sum", dbs["full"]])
        assert a.partners == [(dbs["full"], 5, 35, "require"), (dbs["solid"], 2, 255, "exclude")] and (a.min_count, a.max_count, a.counter) == (3, 90, "sum")
        a = sd.parse_args(["-o", dbs["out"], "--require", dbs["solid"], "--require", dbs["solid2"] + ":255:255", "--counter", "min", dbs["solid"]])
        assert [p[1:] for p in a.partners] == [(1, 255, "require"), (255, 255, "require")]
        with pytest.raises(AssertionError, match="the device was touched: KmerDatabase.load"):
            sd.main(["-o", dbs["out"], "--exclude", dbs["solid"], dbs["full"]])
    assert not os.path.exists(dbs["out"])


def test_select_database_refuses_from_the_command_line_and_the_headers(built, dbs, capsys):
    from trio_binning_amd import select_database as sd

    o = ["-o", dbs["out"]]
    cases = (
        # the output's name
        (["-o", dbs["dir"] + "/picked.db", dbs["full"]], 2, ["picked.db", ".tbkdb"]),
        (["-o", dbs["full"], dbs["full"]], 2, [dbs["full"], "names an input"]),
        (["-o", dbs["solid"], "--exclude", dbs["solid"], dbs["full"]], 2, [dbs["solid"], "names an input"]),
        (["-o", dbs["dir"] + "/./solid2.tbkdb", "--require", dbs["solid2"] + ":2:9", dbs["full"]], 2, ["names an input"]),
        ([dbs["full"]], 2, ["-o"]),
        # more than two partners
        (o + ["--require", dbs["solid"], "--exclude", dbs["solid2"], "--exclude", dbs["full"], dbs["full"]], 2, ["3 --require and --exclude", "at most two"]),
        (o + ["--require", dbs["solid"]] * 3 + [dbs["full"]], 2, ["at most two"]),
        # ranges
        (o + ["--min-count", "0", dbs["full"]], 2, ["--min-count 0", "1 <= min <= max <= 255"]),
        (o + ["--max-count", "256", dbs["full"]], 2, ["--max-count 256", "1 <= min <= max <= 255"]),
        (o + ["--min-count", "9", "--max-count", "8", dbs["full"]], 2, ["1 <= min <= max <= 255"]),
        (o + ["--min-count", "-3", dbs["full"]], 2, ["--min-count -3"]),
        (o + ["--require", dbs["solid"] + ":0", dbs["full"]], 2, ["--require", dbs["solid"], "0..255", "1 <= MIN <= MAX <= 255"]),
        (o + ["--exclude", dbs["solid"] + ":9:8", dbs["full"]], 2, ["--exclude", "9..8"]),
        (o + ["--exclude", dbs["solid"] + ":2:256", dbs["full"]], 2, ["--exclude", "2..256"]),
        (o + ["--counter", "max", dbs["full"]], 2, ["--counter"]),
        # different k
        (o + ["--require", dbs["full16"], dbs["full"]], None, [dbs["full16"], "16-mers", dbs["full"], "21-mers"]),
        (o + ["--exclude", dbs["solid"], "--exclude", dbs["solid16"] + ":2", dbs["full"]], None, [dbs["solid16"], "16-mers", "21-mers"]),
        # mixed spaces
        (o + ["--exclude", dbs["fullh"], dbs["full"]], None, [dbs["fullh"], "homopolymer-compressed", "plain"]),
        (o + ["--require", dbs["solid"], dbs["fullh"]], None, [dbs["solid"], "homopolymer-compressed", "plain"]),
        # files that are no databases, or are not there
        (o + [dbs["damaged"]], None, [dbs["damaged"], "select_database"]),
        (o + ["--require", dbs["damaged"], dbs["full"]], None, [dbs["damaged"], "select_database"]),
        (o + ["--exclude", dbs["solid"] + ".absent.tbkdb", dbs["full"]], None, [".absent.tbkdb", "does not exist"]),
        (o + [dbs["list"]], None, [dbs["list"], "select_database"]),
    )
    _refused(sd.main, cases, capsys)
    assert not os.path.exists(dbs["out"])


# ---- hapmers ----------------------------------------------------------------------------------------------------------------------
CUT = ["--min-count-a", "3", "--max-count-a", "90", "--min-count-b", "2", "--max-count-b", "80", "--min-count-child", "2"]


def test_a_sound_trio_is_settled_from_the_headers(built, dbs):
    from trio_binning_amd import hapmers as hm

    out = os.path.join(dbs["dir"], "hap")
    with no_device():
        a = hm.parse_args(["-o", out, dbs["solid"], dbs["solid2"], "--child-database", dbs["full"]] + CUT)
        pair = a.databases
        assert (pair.ranges, pair.child_min, pair.child_path, pair.prog, pair.compressed) == ({"A": (3, 90), "B": (2, 80)}, 2, dbs["full"], "hapmers", False)
        assert (pair.paths["A"], pair.paths["B"]) == (dbs["solid"], dbs["solid2"])
        with pytest.raises(AssertionError, match="the device was touched: KmerDatabase.load"):
            hm.main(["-o", out, dbs["solid"], dbs["solid2"], "--child-database", dbs["full"]] + CUT)
    assert not os.path.exists(os.path.join(out, "haplotypeA.hapmers.tbkdb"))


def test_hapmers_refuses_from_the_command_line_and_the_headers(built, dbs, capsys):
    from trio_binning_amd import hapmers as hm

    o = ["-o", os.path.join(dbs["dir"], "hap")]
    child = ["--child-database", dbs["solid"]]
    cases = (
        # no child, no output
        (o + [dbs["solid"], dbs["solid2"]] + CUT[:8], 2, ["--child-database"]),
        ([dbs["solid"], dbs["solid2"]] + child + CUT, 2, ["-o"]),
        (["-o", dbs["solid"], dbs["solid"], dbs["solid2"]] + child + CUT, 2, [dbs["solid"], "not a directory"]),
        # paths that are not *.tbkdb
        (o + [dbs["list"], dbs["solid"]] + child + CUT, 2, [dbs["list"], "not a count database", ".tbkdb"]),
        (o + [dbs["solid"], dbs["list"]] + child + CUT, 2, [dbs["list"], "not a count database"]),
        (o + [dbs["solid"], dbs["solid2"], "--child-database", dbs["list"]] + CUT, 2, [dbs["list"], "not a count database"]),
        # cut-offs that cannot be: the refusals of classify-by-kmers
        (o + [dbs["solid"], dbs["solid2"], "--min-count-a", "3"] + child, 2, ["--min-count-a and --max-count-a go together"]),
        (o + [dbs["solid"], dbs["solid2"], "--max-count-b", "30"] + child, 2, ["--min-count-b and --max-count-b go together"]),
        (o + [dbs["solid"], dbs["solid2"], "--min-count-a", "9", "--max-count-a", "3"] + child, 2, ["need 1 <= min <= max"]),
        (o + [dbs["solid"], dbs["solid2"], "--min-count-b", "0", "--max-count-b", "3"] + child, 2, ["need 1 <= min <= max"]),
        (o + [dbs["solid"], dbs["solid2"], "--min-count-a", "256", "--max-count-a", "300"] + child, 2, ["--min-count-a 256", "255"]),
        (o + [dbs["solid"], dbs["solid2"], "--min-count-child", "256"] + child, 2, ["--min-count-child 256", "255"]),
        (o + [dbs["solid"], dbs["solid2"], "--min-count-child", "0"] + child, 2, ["--min-count-child 0"]),
        # different k
        (o + [dbs["solid"], dbs["solid16"]] + child + CUT, None, ["21-mers", "16-mers", "hapmers"]),
        (o + [dbs["solid"], dbs["solid2"], "--child-database", dbs["solid16"]] + CUT, None, [dbs["solid16"], "16-mers"]),
        # mixed spaces
        (o + [dbs["solid"], dbs["fullh"]] + child + CUT, None, ["homopolymer-compressed", "plain", "hapmers"]),
        (o + [dbs["solid"], dbs["solid2"], "--child-database", dbs["fullh"]] + CUT, None, ["the child's", "homopolymer-compressed"]),
        # files that are no databases, or are not there
        (o + [dbs["damaged"], dbs["solid"]] + child + CUT, None, [dbs["damaged"], "hapmers"]),
        (o + [dbs["solid"], dbs["solid2"], "--child-database", dbs["solid"] + ".absent.tbkdb"] + CUT, None, [".absent.tbkdb", "hapmers"]),
        # a histogram the reference's rule finds no cut-offs in (crafted counters are uniform), with none given by hand
        (o + [dbs["solid"], dbs["solid2"]] + child, None, ["could not find min and max counts", "--min-count-a"]),
    )
    _refused(hm.main, cases, capsys)
    assert not os.path.exists(o[1])
