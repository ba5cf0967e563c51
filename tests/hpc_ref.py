"""Homopolymer compression restated with numpy from the contract in include/tbk.h: byte i of a read is kept iff i == 0 or
f(b[i]) != f(b[i - 1]); with fold_case f clears bit 5 of ASCII letters, without it f is the identity; a kept byte is
written as it came.  What tests/test_gpu_hpc*.py hold the device to, byte for byte."""
import numpy as np


def fold(b):
    """f of the contract with fold_case on: a-z read as A-Z, every other byte as it is."""
    b = np.asarray(b, dtype=np.uint8)
    lower = (b >= ord("a")) & (b <= ord("z"))
    return np.where(lower, b & np.uint8(0xDF), b).astype(np.uint8)


def compress_np(bases, offsets, fold_case):
    """(bases, offsets) of the compressed batch: uint8 back to back, uint64 offsets with offsets[0] == 0."""
    bases = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    total = int(off[-1]) if off.size else 0
    bases = bases[:total]
    f = fold(bases) if fold_case else bases
    keep = np.ones(total, dtype=bool)
    keep[1:] = f[1:] != f[:-1]
    starts = off[:-1][off[:-1] < total]  # (a trailing empty read starts at `total`: no position)
    keep[starts] = True
    before = np.zeros(total + 1, dtype=np.int64)  # kept positions before position i
    np.cumsum(keep, out=before[1:])
    return bases[keep], before[off].astype(np.uint64) if off.size else np.zeros(0, dtype=np.uint64)


def compress_reads(reads, fold_case):
    """The same for a list of str, the slow way: one read at a time, one byte at a time."""
    out = []
    for r in reads:
        kept = []
        for i, ch in enumerate(r):
            a, b = (ch, r[i - 1]) if i else (ch, None)
            if fold_case and i:
                a = a.upper() if "a" <= a <= "z" else a
                b = b.upper() if "a" <= b <= "z" else b
            if i == 0 or a != b:
                kept.append(ch)
        out.append("".join(kept))
    return out
