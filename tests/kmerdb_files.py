"""Count database files (*.tbkdb) written with numpy, struct and zlib alone, by the table in INTEGRATION.md: what
tests/test_host_kmerdb_file.py and tests/test_gpu_kmerdb.py compare the library's own files with, and damage on purpose."""
import struct
import zlib

import numpy as np

MAGIC = b"TBKKMDB1"
HEADER = 2096


def header(k, n, hist, reads=0, bases=0, magic=MAGIC, header_size=HEADER, pad=0, crc=None):
    """The 2096 header bytes; `crc` None: computed, as a sound file has it."""
    hist = np.asarray(hist, dtype="<u8")
    assert hist.size == 256
    body = magic + struct.pack("<IIQQQ", header_size, k, n, reads, bases) + hist.tobytes()
    assert len(body) == HEADER - 8
    return body + struct.pack("<II", zlib.crc32(body) & 0xFFFFFFFF if crc is None else crc, pad)


def file_bytes(k, keys, counts, hist, reads=0, bases=0, **fields):
    keys = np.asarray(keys, dtype="<u8")
    counts = np.asarray(counts, dtype=np.uint8)
    return header(k, fields.pop("n", keys.size), hist, reads, bases, **fields) + keys.tobytes() + counts.tobytes()


def database_of(keys, counts):
    """(keys, capped counters, histogram) of the database that (keys, counts) of oracle.unique_oracle.count_kmers_np
    leave: k-mers seen at least twice, counters capped at 255; the histogram keeps row 1 (seen once) and row 0 (all)."""
    counts = np.asarray(counts, dtype=np.int64)
    hist = np.bincount(np.minimum(counts, 255), minlength=256).astype(np.uint64)
    hist[0] = counts.size
    keep = counts >= 2
    return np.asarray(keys, dtype=np.uint64)[keep], np.minimum(counts[keep], 255).astype(np.uint8), hist


def sound(k=21, n=5, seed=1):
    """A small sound file: (bytes, keys, counts, hist)."""
    rng = np.random.default_rng(seed)
    top = (1 << (2 * k)) if k < 32 else (1 << 64)
    keys = np.array(sorted({int(x) for x in rng.integers(0, min(top, 1 << 62), 2 * n + 8)})[:n], dtype=np.uint64)
    assert keys.size == n
    counts = rng.integers(2, 256, n).astype(np.uint8)
    hist = np.bincount(counts, minlength=256).astype(np.uint64)
    hist[1] = 7
    hist[0] = n + 7
    return file_bytes(k, keys, counts, hist, reads=11, bases=1234), keys, counts, hist


def patched(data, offset, new):
    return data[:offset] + new + data[offset + len(new):]


def with_crc(data):
    """The same bytes with the header's CRC computed again (a damage the CRC does not show)."""
    return patched(data, HEADER - 8, struct.pack("<I", zlib.crc32(data[:HEADER - 8]) & 0xFFFFFFFF))


def header_refusals(data, k_other=None):
    """(name, bytes) of every header-level damage of a sound file `data`: each must be refused with TBK_ERR_FORMAT."""
    n = struct.unpack_from("<Q", data, 16)[0]
    hist2 = struct.unpack_from("<Q", data, 40 + 8 * 2)[0]
    flip = bytearray(data)
    flip[100] ^= 0x10
    return [
        ("truncated_in_header", data[:1000]),
        ("one_byte_too_many", data + b"\0"),
        ("wrong_magic", with_crc(patched(data, 0, b"TBKKMDB2"))),
        ("wrong_header_size", with_crc(patched(data, 8, struct.pack("<I", 2104)))),
        ("k_0", with_crc(patched(data, 12, struct.pack("<I", 0)))),
        ("k_33", with_crc(patched(data, 12, struct.pack("<I", 33)))),
        ("header_byte_flipped", bytes(flip)),
        ("n_changed", with_crc(patched(data, 16, struct.pack("<Q", n + 1)))),
        ("rows_do_not_sum_to_n", with_crc(patched(data, 40 + 8 * 2, struct.pack("<Q", hist2 + 1)))),
        ("row_0_too_small", with_crc(patched(data, 40, struct.pack("<Q", n)))),
        ("pad_not_zero", patched(data, HEADER - 4, struct.pack("<I", 1))),
    ]
