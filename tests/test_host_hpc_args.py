"""Homopolymer-compressed k-mers on the command lines: what is refused from the arguments and the files' headers alone.  No
GPU: every refusal here must come before anything loads a list, loads a database, counts or builds a classifier - those entry
points are replaced by ones that fail the test.  Database files are crafted with tests/kmerdb_files.py; a compressed one
differs from a plain one in its magic, TBKKMDH1, alone."""
import os
from unittest.mock import patch

import pytest

import kmerdb_files as kf
from conftest import DATA

MAGIC_HPC = b"TBKKMDH1"


@pytest.fixture()
def files(built, tmp_path, monkeypatch):
    """Sound plain and compressed databases of k = 21, two text lists, and drivers in which touching the device is a failure."""
    import trio_binning_amd.classify_by_kmers as cbk
    from trio_binning_amd import kmers

    paths = {}
    for name, seed, magic in (("plain_a", 1, kf.MAGIC), ("plain_b", 2, kf.MAGIC), ("hpc_a", 1, MAGIC_HPC), ("hpc_b", 2, MAGIC_HPC), ("hpc_c", 3, MAGIC_HPC)):
        _, keys, counts, hist = kf.sound(k=21, n=5, seed=seed)
        paths[name] = str(tmp_path / (name + ".tbkdb"))
        with open(paths[name], "wb") as fh:
            fh.write(kf.file_bytes(21, keys, counts, hist, reads=11, bases=1234, magic=magic))
    paths["list_a"], paths["list_b"] = os.path.join(DATA, "hapA.txt"), os.path.join(DATA, "hapB.txt")
    paths["hpc_list"] = str(tmp_path / "compressed_list.txt")
    with open(paths["hpc_list"], "w") as fh:
        fh.write("ACGTACGTACGTACGTACGTA\nTGCATGCATGCATGCATGCAT\n")
    paths["reads"] = os.path.join(DATA, "test.fastq")
    paths["bins"] = tmp_path / "bins"
    paths["bins"].mkdir()

    def touched(*args, **kwargs):
        raise AssertionError("the device was touched before the arguments were refused")

    monkeypatch.setattr(kmers, "create_kmer_hash_set", touched)
    monkeypatch.setattr(kmers.HashSet, "from_file", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "load", touched)
    monkeypatch.setattr(kmers.KmerDatabase, "unique_set", touched)
    monkeypatch.setattr(kmers, "KmerCounter", touched)
    monkeypatch.setattr(kmers, "HomopolymerCompressor", touched)
    monkeypatch.setattr(kmers, "device_mem_info", touched)
    monkeypatch.setattr(cbk, "make_classifier", touched)
    monkeypatch.setattr(cbk, "classify_compressed", touched)
    return paths


CUTS = ["--min-count-a", "2", "--max-count-a", "9", "--min-count-b", "2", "--max-count-b", "9"]


def _classify_exit(files, argv):
    """Run classify-by-kmers; it must leave through SystemExit with a message, having written nothing."""
    import trio_binning_amd.classify_by_kmers as cbk

    prefixes = ["--haplotype-a-out-prefix", str(files["bins"] / "hapA"), "--haplotype-b-out-prefix", str(files["bins"] / "hapB"),
                "--unclassified-out-prefix", str(files["bins"] / "unclassified")]
    with patch("sys.argv", ["classify-by-kmers"] + argv + prefixes):
        with pytest.raises(SystemExit) as ei:
            cbk.main()
    assert os.listdir(files["bins"]) == []
    assert isinstance(ei.value.code, str), ei.value.code
    return ei.value.code


def test_the_header_says_which_space_a_database_is_in(files):
    from trio_binning_amd import kmers

    for name, compressed in (("plain_a", False), ("plain_b", False), ("hpc_a", True), ("hpc_b", True)):
        info = kmers.database_file_info(files[name])
        assert info["compressed"] is compressed and info["k"] == 21 and info["n"] == 5 and info["reads_added"] == 11 and info["bases_added"] == 1234
    plain, hpc = open(files["plain_a"], "rb").read(), open(files["hpc_a"], "rb").read()
    assert len(plain) == len(hpc) and plain[:8] == kf.MAGIC and hpc[:8] == MAGIC_HPC
    assert plain[8:kf.HEADER - 8] == hpc[8:kf.HEADER - 8] and plain[kf.HEADER - 4:] == hpc[kf.HEADER - 4:]  # the magic and the CRC over it differ, nothing else


@pytest.mark.parametrize("pair", [("hpc_a", "plain_b"), ("plain_a", "hpc_b")])
@pytest.mark.parametrize("flag", [[], ["--compress"]])
def test_parents_that_disagree_are_refused(files, capsys, pair, flag):
    code = _classify_exit(files, [files["reads"], files[pair[0]], files[pair[1]]] + CUTS + flag)
    assert files[pair[0]] in code and files[pair[1]] in code and "homopolymer-compressed" in code and "plain" in code
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("trio", [("hpc_a", "hpc_b", "plain_a"), ("plain_a", "plain_b", "hpc_c")])
def test_a_child_that_disagrees_is_refused(files, capsys, trio):
    code = _classify_exit(files, [files["reads"], files[trio[0]], files[trio[1]], "--child-database", files[trio[2]], "--min-count-child", "2"] + CUTS)
    assert files[trio[2]] in code and "child" in code and "homopolymer-compressed" in code and "plain" in code
    assert capsys.readouterr().out == ""


def test_compress_with_plain_databases_is_refused(files, capsys):
    code = _classify_exit(files, [files["reads"], files["plain_a"], files["plain_b"], "--compress"] + CUTS)
    assert "--compress" in code and files["plain_a"] in code and files["plain_b"] in code and "plain" in code
    assert capsys.readouterr().out == ""


def test_compressed_databases_switch_the_mode_on_by_themselves(files, capsys):
    """Nothing left to refuse: with or without --compress the driver settles on compressed mode and goes on to load the databases."""
    import trio_binning_amd.classify_by_kmers as cbk

    for flag in ([], ["--compress"]):
        with patch("sys.argv", ["classify-by-kmers", files["reads"], files["hpc_a"], files["hpc_b"]] + CUTS + flag):
            args = cbk.parse_args()
            assert args.compress is True and args.databases.compressed is True
            with pytest.raises(AssertionError, match="device was touched"):
                cbk.main()
    with patch("sys.argv", ["classify-by-kmers", files["reads"], files["plain_a"], files["plain_b"]] + CUTS):
        args = cbk.parse_args()
        assert args.compress is False and args.databases.compressed is False
    assert capsys.readouterr().out == ""


def test_a_list_with_two_equal_neighbours_was_not_made_with_compress(files, capsys):
    first = open(files["list_a"]).readline().strip()
    assert any(x == y for x, y in zip(first, first[1:]))  # (the fixture list is a plain one, and says so in its first line)
    for pair in ((files["list_a"], files["list_b"]), (files["hpc_list"], files["list_b"]), (files["list_a"], files["hpc_list"])):
        code = _classify_exit(files, [files["reads"], pair[0], pair[1], "--compress"])
        culprit = pair[0] if pair[0] != files["hpc_list"] else pair[1]
        assert "this list was not made with --compress" in code and culprit in code
    # a pair far down the list is not looked for: only the first 1000 lines are read
    late = str(files["bins"].parent / "late.txt")
    with open(late, "w") as fh:
        fh.write("ACGTACGTACGTACGTACGTA\n" * 1000 + "AAGTACGTACGTACGTACGTA\n")
    import trio_binning_amd.classify_by_kmers as cbk

    for pair in ((files["hpc_list"], late), (files["hpc_list"], files["hpc_list"])):
        with patch("sys.argv", ["classify-by-kmers", files["reads"], pair[0], pair[1], "--compress"]):
            with pytest.raises(AssertionError, match="device was touched"):  # nothing refused: the lists are loaded next
                cbk.main()
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("case", ["plain_database_under_compress", "compressed_database_without", "compressed_child_without", "plain_child_under_compress"])
def test_find_unique_kmers_refuses_a_database_from_the_other_space(files, capsys, case):
    from trio_binning_amd import find_unique_kmers as fu

    out = str(files["bins"])
    argv = {"plain_database_under_compress": ["--compress", files["hpc_a"], files["plain_b"]],
            "compressed_database_without": [files["plain_a"], files["hpc_b"]],
            "compressed_child_without": ["--child", files["hpc_c"], files["plain_a"], files["plain_b"]],
            "plain_child_under_compress": ["--compress", "--child", files["plain_a"], files["hpc_a"], files["hpc_b"]]}[case]
    culprit = {"plain_database_under_compress": "plain_b", "compressed_database_without": "hpc_b", "compressed_child_without": "hpc_c",
               "plain_child_under_compress": "plain_a"}[case]
    with pytest.raises(SystemExit) as ei:
        fu.main(["-k", "21", "-o", out, "-s", out] + argv)
    code = ei.value.code
    assert isinstance(code, str) and files[culprit] in code and "--compress" in code
    assert ("plain" in code) == ("under_compress" in case) and ("homopolymer-compressed" in code) == ("without" in case)
    assert os.listdir(out) == [] and capsys.readouterr().out == ""


def test_phase_blocks_refuses_compressed_databases(files, capsys, tmp_path):
    from trio_binning_amd import phase_blocks

    bed = str(tmp_path / "blocks.bed")
    with pytest.raises(SystemExit) as ei:
        phase_blocks.main([files["reads"], files["hpc_a"], files["hpc_b"], "--bed", bed] + CUTS)
    code = ei.value.code
    assert isinstance(code, str) and code.startswith("phase_blocks:") and "homopolymer-compressed" in code and files["hpc_a"] in code
    assert not os.path.exists(bed) and not os.path.exists(bed + ".tmp") and capsys.readouterr().out == ""
    with pytest.raises(SystemExit) as ei:  # parents that disagree are refused in classify-by-kmers' words, under this command's name
        phase_blocks.main([files["reads"], files["plain_a"], files["hpc_b"], "--bed", bed] + CUTS)
    assert isinstance(ei.value.code, str) and ei.value.code.startswith("phase_blocks:") and files["hpc_b"] in ei.value.code


def test_assembly_qv_refuses_a_compressed_database(files, capsys, tmp_path):
    from trio_binning_amd import assembly_qv

    with pytest.raises(SystemExit) as ei:
        assembly_qv.main([os.path.join(DATA, "test.fa"), files["hpc_a"]])
    code = ei.value.code
    assert isinstance(code, str) and code.startswith("assembly_qv:") and "homopolymer-compressed" in code and files["hpc_a"] in code
    assert capsys.readouterr().out == ""
