"""The count database file (*.tbkdb) and the command line around it, without a GPU: tbk_kmerdb_file_info reads and checks
the header alone (include/tbk.h), on files this test writes itself with numpy, struct and zlib (tests/kmerdb_files.py);
find-unique-kmers parses --keep-databases, the cut-offs given by hand and a parent that is a database."""
import ctypes as C

import numpy as np
import pytest

import kmerdb_files as kf


def _info_status(_lib, path):
    k, n, reads, bases = C.c_int(-1), C.c_uint64(), C.c_uint64(), C.c_uint64()
    hist = (C.c_uint64 * 256)()
    rc = _lib.lib.tbk_kmerdb_file_info(str(path).encode(), C.byref(k), C.byref(n), hist, C.byref(reads), C.byref(bases))
    return rc, _lib.last_error()


@pytest.mark.parametrize("k", [1, 21, 32])
def test_file_info_reads_a_sound_header(built, tmp_path, k):
    from trio_binning_amd import kmers

    data, keys, counts, hist = kf.sound(k=k, n=3 if k == 1 else 37)
    assert len(data) == 2096 + 9 * keys.size
    path = tmp_path / "good.tbkdb"
    path.write_bytes(data)
    info = kmers.database_file_info(str(path))
    assert info["k"] == k and info["n"] == keys.size and info["reads_added"] == 11 and info["bases_added"] == 1234
    assert info["histogram"].dtype == np.uint64 and info["histogram"].tolist() == hist.tolist()


def test_file_info_reads_an_empty_database(built, tmp_path):
    from trio_binning_amd import kmers

    hist = np.zeros(256, dtype=np.uint64)
    hist[0] = hist[1] = 90  # every k-mer seen once
    path = tmp_path / "empty.tbkdb"
    path.write_bytes(kf.file_bytes(16, [], [], hist, reads=4, bases=100))
    info = kmers.database_file_info(str(path))
    assert info["k"] == 16 and info["n"] == 0 and int(info["histogram"][1]) == 90
    # any out pointer may be NULL
    from trio_binning_amd import _lib
    assert _lib.lib.tbk_kmerdb_file_info(str(path).encode(), None, None, None, None, None) == _lib.TBK_OK


def test_file_info_missing_file_is_io_error(built, tmp_path):
    from trio_binning_amd import _lib, kmers

    rc, msg = _info_status(_lib, tmp_path / "absent.tbkdb")
    assert rc == _lib.TBK_ERR_IO and "absent.tbkdb" in msg
    with pytest.raises(IOError):
        kmers.database_file_info(str(tmp_path / "absent.tbkdb"))


_SOUND = kf.sound(k=21, n=40, seed=3)[0]


@pytest.mark.parametrize("name", [name for name, _ in kf.header_refusals(_SOUND)])
def test_file_info_refuses_a_damaged_header(built, tmp_path, name):
    from trio_binning_amd import _lib, kmers

    good = tmp_path / "good.tbkdb"
    good.write_bytes(_SOUND)
    bad = tmp_path / (name + ".tbkdb")
    bad.write_bytes(dict(kf.header_refusals(_SOUND))[name])
    rc, msg = _info_status(_lib, bad)
    assert rc == _lib.TBK_ERR_FORMAT and name + ".tbkdb" in msg, (rc, msg)
    with pytest.raises(ValueError):
        kmers.database_file_info(str(bad))
    assert _info_status(_lib, good)[0] == _lib.TBK_OK  # and a sound file is read after it


def test_file_info_refuses_truncated_content(built, tmp_path):
    """The header alone says how long the file must be: one cut inside the keys, one inside the counters."""
    from trio_binning_amd import _lib

    for cut in (2096 + 8 * 17 + 3, len(_SOUND) - 5):
        path = tmp_path / "cut.tbkdb"
        path.write_bytes(_SOUND[:cut])
        assert _info_status(_lib, path)[0] == _lib.TBK_ERR_FORMAT


def test_parse_args_database_options(built, capsys):
    from trio_binning_amd import find_unique_kmers as fu

    a = fu.parse_args(["-k", "21", "a.fq", "b.fq"])
    assert not a.keep_databases and a.min_count_a is None and a.max_count_a is None and a.min_count_b is None and a.max_count_b is None
    a = fu.parse_args(["-k", "21", "--keep-databases", "--min-count-a", "3", "--max-count-a", "40", "a.fq,a2.fq", "out/haplotypeB.tbkdb"])
    assert a.keep_databases and (a.min_count_a, a.max_count_a) == (3, 40) and a.min_count_b is None
    assert [fu.is_database_path(p) for p in a.read_files] == [False, True]
    assert not fu.is_database_path("x.tbkdb,y.tbkdb") and not fu.is_database_path("reads.tbkdb.gz")
    a = fu.parse_args(["-k", "5", "--min-count-b", "7", "--max-count-b", "7", "a.tbkdb", "b.tbkdb"])
    assert (a.min_count_b, a.max_count_b) == (7, 7)
    for bad in (["--min-count-a", "3"], ["--max-count-b", "9"], ["--min-count-a", "0", "--max-count-a", "5"],
                ["--min-count-b", "9", "--max-count-b", "8"], ["--min-count-a", "x", "--max-count-a", "5"]):
        with pytest.raises(SystemExit) as ei:
            fu.parse_args(["-k", "21"] + bad + ["a.fq", "b.fq"])
        assert ei.value.code == 2
        assert "count" in capsys.readouterr().err


def test_database_of_another_k_is_refused_before_counting(built, tmp_path, capsys):
    """-k 21 against a k = 16 file: a plain message, and count_library is never reached."""
    from unittest.mock import patch

    from trio_binning_amd import find_unique_kmers as fu

    path = tmp_path / "haplotypeA.tbkdb"
    path.write_bytes(kf.sound(k=16, n=9)[0])
    with patch.object(fu, "count_library", side_effect=AssertionError("counted")), \
            patch.object(fu.kmers, "device_mem_info", side_effect=AssertionError("asked the device")):
        with pytest.raises(SystemExit) as ei:
            fu.main(["-k", "21", "-o", str(tmp_path), "-s", str(tmp_path), str(path), str(tmp_path / "b.fq")])
    assert "16-mers" in str(ei.value.code) and "-k 21" in str(ei.value.code)
