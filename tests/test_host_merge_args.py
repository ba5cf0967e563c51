"""The command lines around full count databases, without a GPU: find-unique-kmers --keep-singletons and the mixed parent
argument (databases and read files in one list), choose_passes' database_share, merge_databases' arguments and assembly-qv's
--min-count 1.  Databases are files this test writes itself (tests/kmerdb_files.py); no device is touched."""
from unittest.mock import patch

import numpy as np
import pytest

import kmerdb_files as kf
from test_host_kmerdb_full import FULL, FULL_HPC, full_file


@pytest.fixture()
def dbs(tmp_path):
    files = {
        "full": full_file(k=21, seed=2)[0],
        "full2": full_file(k=21, seed=5)[0],
        "full16": full_file(k=16, seed=2)[0],
        "fullh": full_file(k=21, seed=2, magic=FULL_HPC)[0],
        "solid": kf.sound(k=21, n=40, seed=3)[0],
        "damaged": full_file(k=21, seed=2)[0][:-3],
    }
    out = {}
    for name, data in files.items():
        out[name] = str(tmp_path / (name + ".tbkdb"))
        open(out[name], "wb").write(data)
    for name in ("r1.fq", "r2.fq.gz", "asm.fa"):
        out[name] = str(tmp_path / name)
        open(out[name], "w").write(">s\nACGT\n" if name == "asm.fa" else "@r\nACGT\n+\nIIII\n")
    return out


# ---- find-unique-kmers ----------------------------------------------------------------------------------------------------
def test_the_mixed_form_on_its_own():
    from trio_binning_amd import find_unique_kmers as fu

    assert fu.is_mixed_argument("mother.tbkdb,new_lane.fq.gz") and fu.is_mixed_argument("a.fq,b.tbkdb,c.fq") and fu.is_mixed_argument("x.tbkdb,y.tbkdb")
    assert not fu.is_mixed_argument("mother.tbkdb") and not fu.is_mixed_argument("a.fq,b.fq") and not fu.is_mixed_argument("a.fq")
    assert not fu.is_mixed_argument("reads.tbkdb.gz,b.fq")
    assert fu.split_mixed_argument("a.fq,m.tbkdb,b.fq.gz,n.tbkdb") == (["m.tbkdb", "n.tbkdb"], ["a.fq", "b.fq.gz"])
    assert fu.split_mixed_argument("a.fq,b.fq") == ([], ["a.fq", "b.fq"])
    # is_database_path keeps its meaning: one database and nothing else
    assert fu.is_database_path("mother.tbkdb") and not fu.is_database_path("mother.tbkdb,new_lane.fq.gz") and not fu.is_database_path("x.tbkdb,y.tbkdb")


def test_parse_args_keep_singletons(built, dbs, capsys):
    from trio_binning_amd import find_unique_kmers as fu

    assert not fu.parse_args(["-k", "21", "a.fq", "b.fq"]).keep_singletons
    a = fu.parse_args(["-k", "21", "--keep-databases", "--keep-singletons", "a.fq", "b.fq"])
    assert a.keep_singletons and a.keep_databases
    assert fu.parse_args(["-k", "21", "--keep-singletons", "--child", "c.fq", "a.fq", "b.fq"]).keep_singletons
    assert fu.parse_args(["-k", "21", "--keep-singletons", dbs["full"], "b.fq"]).keep_singletons
    assert fu.parse_args(["-k", "21", "--keep-singletons", dbs["full"] + "," + dbs["r1.fq"], "b.fq"]).keep_singletons
    with pytest.raises(SystemExit) as ei:  # two live counters: no database for the flag to act on
        fu.parse_args(["-k", "21", "--keep-singletons", "a.fq", "b.fq"])
    assert ei.value.code == 2 and "--keep-databases" in capsys.readouterr().err


def test_parse_args_takes_a_mixed_list_of_full_databases_and_reads(built, dbs):
    from trio_binning_amd import find_unique_kmers as fu

    mixed = ",".join([dbs["full"], dbs["r2.fq.gz"]])
    a = fu.parse_args(["-k", "21", mixed, dbs["r1.fq"], "--child", ",".join([dbs["r1.fq"], dbs["full2"], dbs["full"]])])
    assert a.read_files == [mixed, dbs["r1.fq"]]
    assert [fu.is_mixed_argument(s) for s in a.read_files] == [True, False] and fu.is_mixed_argument(a.child)
    a = fu.parse_args(["-k", "21", "--compress", dbs["fullh"] + "," + dbs["r1.fq"], "b.fq"])
    assert a.compress


@pytest.mark.parametrize("which,words", [("solid", ["without the k-mers seen once", "--keep-singletons"]), ("full16", ["16-mers", "-k 21"]),
                                         ("fullh", ["homopolymer-compressed", "--compress"]), ("damaged", ["9 bytes each"])])
@pytest.mark.parametrize("place", ["a", "b", "child"])
def test_a_mixed_list_is_refused_by_its_headers_before_anything_is_counted(built, dbs, capsys, which, words, place):
    from trio_binning_amd import find_unique_kmers as fu

    mixed = ",".join([dbs["full"], dbs[which], dbs["r1.fq"]])
    argv = {"a": [mixed, "b.fq"], "b": ["a.fq", mixed], "child": ["--child", mixed, "a.fq", "b.fq"]}[place]
    with patch.object(fu, "count_library", side_effect=AssertionError("counted")), \
            patch.object(fu.kmers, "device_mem_info", side_effect=AssertionError("asked the device")):
        with pytest.raises(SystemExit) as ei:
            fu.main(["-k", "21"] + argv)
    err = capsys.readouterr().err
    assert ei.value.code == 2 and dbs[which] in err and all(w in err for w in words), err


def test_a_plain_run_refuses_a_compressed_database_in_a_mixed_list_the_other_way_round(built, dbs, capsys):
    from trio_binning_amd import find_unique_kmers as fu

    with pytest.raises(SystemExit):
        fu.parse_args(["-k", "21", "--compress", dbs["full"] + "," + dbs["r1.fq"], "b.fq"])
    assert "plain (uncompressed)" in capsys.readouterr().err


def test_choose_passes_database_share():
    from trio_binning_amd import find_unique_kmers as fu

    # hand-computed, all integers.  capacity 3e9, 60e9 bases, 200e9 bytes free: budget = 160e9; table(1) = 80e9, so P > 1;
    # store = 30e9.  share 8: databases = 2 * 9 * 375e6 = 6.75e9, room 123.25e9 for 3 * table(P): table(2) = 40e9 -> fits, P = 2.
    # share 1: databases = 2 * 9 * 3e9 = 54e9, room 76e9: table(2) = 40e9 (120e9 no), table(3) = 1e9 * 80 // 3 = 26666666666
    # (79999999998 no), table(4) = 750e6 * 80 // 3 = 20e9 (60e9 yes) -> P = 4.
    cap, bases, free = 3_000_000_000, 60_000_000_000, 200_000_000_000
    assert fu.choose_passes(cap, bases, free) == 2
    assert fu.choose_passes(cap, bases, free, database_share=8) == 2
    assert fu.choose_passes(cap, bases, free, database_share=1) == 4
    # three databases (a child) at share 1: 81e9, room 49e9: 3 * table(5) = 3 * 16e9 = 48e9 -> P = 5
    assert fu.choose_passes(cap, bases, free, databases=3, database_share=1) == 5
    # share 1 where store and databases alone leave nothing: no P up to 1024 fits
    with pytest.raises(ValueError, match="passes"):
        fu.choose_passes(cap, bases, 105_000_000_000, database_share=1)  # budget 84e9 = store + databases exactly
    # one pass is untouched by the share (nothing is kept while counting)
    assert fu.choose_passes(1000, 10_000, 10**9, database_share=1) == 1
    with pytest.raises(ValueError):
        fu.choose_passes(cap, bases, free, database_share=0)
    # left out, the argument changes nothing: a grid of today's results
    for cap in (1 << 16, 10**8, 3 * 10**9, 10**11):
        for bases in (0, 10**9, 6 * 10**10):
            for free in (10**9, 6 * 10**10, 2 * 10**11):
                for databases in (2, 3):
                    def run(**kw):
                        try:
                            return fu.choose_passes(cap, bases, free, databases=databases, **kw)
                        except ValueError as exc:
                            return str(exc)
                    assert run() == run(database_share=fu.DATABASE_SHARE) == run(database_share=8)


# ---- merge_databases --------------------------------------------------------------------------------------------------------
def test_merge_databases_arguments(built, dbs, capsys):
    from trio_binning_amd import merge_databases as md

    with patch.object(md.kmers.KmerDatabase, "load", side_effect=AssertionError("the device was touched")):
        a = md.parse_args(["-o", "out.tbkdb", dbs["full"], dbs["full2"]])
        assert a.output == "out.tbkdb" and not a.solid and a.databases == [dbs["full"], dbs["full2"]] and [i["floor"] for i in a.infos] == [1, 1]
        a = md.parse_args(["--solid", "-o", "out.tbkdb", dbs["full"]])  # one input with --solid: a plain conversion
        assert a.solid and len(a.infos) == 1
        for argv, code, words in (
                ([dbs["full"], dbs["full2"]], 2, ["-o"]),
                (["-o", "out.tbkdb"], 2, ["db.tbkdb"]),
                (["-o", "out.txt", dbs["full"], dbs["full2"]], 2, [".tbkdb"]),
                (["-o", "out.tbkdb", dbs["full"]], 2, ["--solid"]),
                (["-o", "out.tbkdb", dbs["full"], dbs["solid"]], None, [dbs["solid"], "without the k-mers seen once", "--keep-singletons"]),
                (["-o", "out.tbkdb", "--solid", dbs["solid"]], None, [dbs["solid"], "without the k-mers seen once"]),
                (["-o", "out.tbkdb", dbs["full"], dbs["full16"]], None, [dbs["full16"], "16-mers", "21-mers"]),
                (["-o", "out.tbkdb", dbs["full"], dbs["fullh"]], None, [dbs["fullh"], "homopolymer-compressed", "plain"]),
                (["-o", "out.tbkdb", dbs["full"], dbs["damaged"]], None, [dbs["damaged"], "9 bytes each"]),
                (["-o", "out.tbkdb", dbs["full"], dbs["full"] + ".absent"], None, ["does not exist"])):
            with pytest.raises(SystemExit) as ei:
                md.main(argv)
            err = capsys.readouterr().err
            text = err if code == 2 else str(ei.value.code)
            assert (ei.value.code == 2) == (code == 2) and all(w in text for w in words), (argv, ei.value.code, err)
        # a sound command line reaches the device and nothing else stops it
        with pytest.raises(AssertionError, match="the device was touched"):
            md.main(["-o", "out.tbkdb", dbs["full"], dbs["full2"]])


# ---- assembly-qv ------------------------------------------------------------------------------------------------------------
def test_assembly_qv_min_count_1_needs_a_full_database(built, dbs, capsys):
    from trio_binning_amd import assembly_qv

    a = assembly_qv.parse_args([dbs["asm.fa"], dbs["full"], "--min-count", "1"])
    assert a.min_count == 1 and a.info["floor"] == 1
    a = assembly_qv.parse_args([dbs["asm.fa"], dbs["full"]])
    assert a.min_count == 2
    assert assembly_qv.parse_args([dbs["asm.fa"], dbs["solid"], "--min-count", "2"]).info["floor"] == 2
    with pytest.raises(SystemExit) as ei:
        assembly_qv.parse_args([dbs["asm.fa"], dbs["solid"], "--min-count", "1"])
    err = capsys.readouterr().err
    assert ei.value.code == 2 and "--min-count" in err and "2 <= N <= 255" in err and "--keep-singletons" in err
    for argv in (["--min-count", "0"], ["--max-count", "1"], ["--min-count", "256"]):  # a full database widens nothing else
        with pytest.raises(SystemExit) as ei:
            assembly_qv.parse_args([dbs["asm.fa"], dbs["full"]] + argv)
        assert ei.value.code == 2 and "2 <= N <= 255" in capsys.readouterr().err
