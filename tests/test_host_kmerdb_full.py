"""Full count databases - the ones that keep the k-mers seen once (tbk_counter_options.keep_singletons; include/tbk.h) -
without a GPU: the two new file magics and their header rules (tbk_kmerdb_file_info, tbk_kmerdb_file_floor), on files this
test writes itself (tests/kmerdb_files.py, ``magic=``), and the option struct's new field."""
import ctypes as C
import struct

import numpy as np
import pytest

import kmerdb_files as kf

FULL = b"TBKKMFB1"
FULL_HPC = b"TBKKMFH1"


def full_file(k=21, n=40, seed=2, magic=FULL, ones=11):
    """A sound full file: (bytes, keys, counts, hist); `ones` of its counters are 1"""
    rng = np.random.default_rng(seed)
    keys = np.array(sorted({int(x) for x in rng.integers(0, 1 << min(2 * k, 62), 2 * n + 8)})[:n], dtype=np.uint64)
    assert keys.size == n
    counts = rng.integers(2, 256, n).astype(np.uint8)
    counts[rng.permutation(n)[:ones]] = 1
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[0] = n
    return kf.file_bytes(k, keys, counts, hist, reads=11, bases=1234, magic=magic), keys, counts, hist


def _status(_lib, fn, path, *out):
    rc = getattr(_lib.lib, fn)(str(path).encode(), *out)
    return rc, _lib.last_error()


def _info_status(_lib, path):
    return _status(_lib, "tbk_kmerdb_file_info", path, None, None, None, None, None)


def _floor(_lib, path):
    floor = C.c_int(-1)
    rc, msg = _status(_lib, "tbk_kmerdb_file_floor", path, C.byref(floor))
    return rc, floor.value, msg


@pytest.mark.parametrize("magic,compressed", [(FULL, False), (FULL_HPC, True)])
def test_a_sound_full_file_passes_and_says_floor_1(built, tmp_path, magic, compressed):
    from trio_binning_amd import _lib, kmers

    data, keys, counts, hist = full_file(magic=magic)
    assert len(data) == 2096 + 9 * keys.size and int(hist[1]) == 11 and int(hist[0]) == keys.size
    path = tmp_path / "full.tbkdb"
    path.write_bytes(data)
    assert _info_status(_lib, path)[0] == _lib.TBK_OK
    assert _floor(_lib, path)[:2] == (_lib.TBK_OK, 1)
    info = kmers.database_file_info(str(path))
    assert info["floor"] == 1 and info["compressed"] is compressed and info["n"] == keys.size and info["k"] == 21
    assert info["histogram"].tolist() == hist.tolist() and (info["reads_added"], info["bases_added"]) == (11, 1234)


def test_an_empty_full_file_is_sound(built, tmp_path):
    from trio_binning_amd import _lib

    path = tmp_path / "empty.tbkdb"
    path.write_bytes(kf.file_bytes(16, [], [], np.zeros(256, dtype=np.uint64), magic=FULL))
    assert _floor(_lib, path)[:2] == (_lib.TBK_OK, 1)


@pytest.mark.parametrize("magic,compressed", [(kf.MAGIC, False), (b"TBKKMDH1", True)])
def test_the_old_magics_say_floor_2(built, tmp_path, magic, compressed):
    from trio_binning_amd import _lib, kmers

    keys = np.arange(5, 12, dtype=np.uint64)
    counts = np.arange(2, 9, dtype=np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1], hist[0] = 4, keys.size + 4
    path = tmp_path / "solid.tbkdb"
    path.write_bytes(kf.file_bytes(21, keys, counts, hist, magic=magic))
    assert _floor(_lib, path)[:2] == (_lib.TBK_OK, 2)
    info = kmers.database_file_info(str(path))
    assert info["floor"] == 2 and info["compressed"] is compressed


def _refusals():
    data, keys, counts, hist = full_file()
    n = keys.size
    # a floor-2 body (no counter 1 among the entries) whose header still tells of the once-seen k-mers: row 1 is not zero,
    # n excludes them - the sound floor-2 file of tests/kmerdb_files.py under the full magic
    solid = kf.sound(k=21, n=40, seed=3)[0]
    assert struct.unpack_from("<Q", solid, 40 + 8)[0] == 7
    return {
        "rows_1_to_255_do_not_sum_to_n": kf.with_crc(kf.patched(data, 40 + 8 * 9, struct.pack("<Q", int(hist[9]) + 1))),
        "row_1_one_too_many": kf.with_crc(kf.patched(data, 40 + 8, struct.pack("<Q", int(hist[1]) + 1))),
        "row_0_above_n": kf.with_crc(kf.patched(data, 40, struct.pack("<Q", n + 1))),
        "row_0_below_n": kf.with_crc(kf.patched(data, 40, struct.pack("<Q", n - 1))),
        "floor_2_body_under_a_full_magic": kf.with_crc(kf.patched(solid, 0, FULL)),
        "floor_2_body_under_a_full_compressed_magic": kf.with_crc(kf.patched(solid, 0, FULL_HPC)),
        "full_body_under_the_old_magic": kf.with_crc(kf.patched(data, 0, kf.MAGIC)),  # rows 2..255 do not sum to n
    }


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_an_unsound_full_header_is_refused(built, tmp_path, name):
    from trio_binning_amd import _lib, kmers

    bad = tmp_path / (name + ".tbkdb")
    bad.write_bytes(_refusals()[name])
    rc, msg = _info_status(_lib, bad)
    assert rc == _lib.TBK_ERR_FORMAT and name + ".tbkdb" in msg and ("histogram row" in msg or "sum to" in msg), (rc, msg)
    rc, floor, msg = _floor(_lib, bad)
    assert rc == _lib.TBK_ERR_FORMAT and floor == -1 and msg
    with pytest.raises(ValueError):
        kmers.database_file_info(str(bad))
    good = tmp_path / "good.tbkdb"
    good.write_bytes(full_file()[0])
    assert _info_status(_lib, good)[0] == _lib.TBK_OK  # and a sound file is read after it


@pytest.mark.parametrize("name", [name for name, _ in kf.header_refusals(full_file()[0])
                                  if name not in ("rows_do_not_sum_to_n", "row_0_too_small")])
def test_the_common_header_damage_is_refused_under_the_full_magic_too(built, tmp_path, name):
    """magic, header size, k, CRC, pad and file size are checked before the floor matters"""
    from trio_binning_amd import _lib

    bad = tmp_path / (name + ".tbkdb")
    bad.write_bytes(dict(kf.header_refusals(full_file()[0]))[name])
    assert _info_status(_lib, bad)[0] == _lib.TBK_ERR_FORMAT


def test_file_floor_arguments(built, tmp_path):
    from trio_binning_amd import _lib

    floor = C.c_int(-1)
    assert _lib.lib.tbk_kmerdb_file_floor(None, C.byref(floor)) == _lib.TBK_ERR_INVALID
    assert _lib.lib.tbk_kmerdb_file_floor(str(tmp_path / "absent.tbkdb").encode(), C.byref(floor)) == _lib.TBK_ERR_IO
    assert _lib.lib.tbk_kmerdb_floor(None, C.byref(floor)) == _lib.TBK_ERR_INVALID and floor.value == -1


def test_counter_options_init_zeroes_the_new_field_and_the_size_stays(built):
    from trio_binning_amd import _lib

    assert C.sizeof(_lib.CounterOptions) == 24
    assert _lib.CounterOptions.keep_singletons.offset == 20 and _lib.CounterOptions.keep_singletons.size == 4
    opts = _lib.CounterOptions()
    C.memset(C.byref(opts), 0xAB, C.sizeof(opts))
    _lib.lib.tbk_counter_options_init(C.byref(opts))
    assert (opts.size, opts.passes, opts.store_limit_bytes, opts.compress, opts.keep_singletons) == (24, 1, 0, 0, 0)
    assert bytes(opts)[20:24] == b"\0\0\0\0"
