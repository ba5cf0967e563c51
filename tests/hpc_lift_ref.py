"""The compression map read backwards, and the hit tracker's results in compressed space lifted to the batch as given, restated
with numpy and plain Python from the definition in include/tbk.h (tbk_hpc_lift): kept byte j of the compressed batch came
from input position lift(j), the position of the j-th set keep bit, and lift(total_c) = total.  Marks, runs and blocks are
those of tests/hit_track_ref.py on the numpy-compressed batch (tests/hpc_ref.py), with their coordinates lifted.  Nothing here
touches a device."""
import numpy as np

import hit_track_ref as ref
import hpc_ref

LIFTED_DTYPE = [("read", "<u8"), ("first", "<u8"), ("last", "<u8"), ("end", "<u8"), ("markers", "<u4"), ("hap", "<u4")]


def keep_np(bases, offsets, fold):
    """one bool per base of the batch: position 0 of a read, or a byte that differs (folded, with ``fold``) from the one before"""
    off = np.asarray(offsets).astype(np.int64)
    total = int(off[-1]) if off.size else 0
    bases = np.asarray(bases, dtype=np.uint8)[:total]
    f = hpc_ref.fold(bases) if fold else bases
    keep = np.ones(total, dtype=bool)
    keep[1:] = f[1:] != f[:-1]
    keep[off[:-1][off[:-1] < total]] = True
    return keep


def lift_np(bases, offsets, fold):
    """lift(0 .. total_c): the positions of the set keep bits, and ``total`` behind them"""
    keep = keep_np(bases, offsets, fold)
    return np.append(np.flatnonzero(keep), keep.size).astype(np.uint64)


def expand_np(values, lift, total):
    out = np.zeros(total, dtype=np.uint8)
    out[lift[:-1].astype(np.int64)] = values
    return out


class Lifted:
    """Everything the tracker must say about one batch in compressed space: the compressed batch (cb, co), its marks (mk_c) and
    their per-read sums (counts), the marks expanded to the batch as given (marks) and the lifted raw runs (runs)."""

    def __init__(self, bases, offsets, keys_a, keys_b, k, ignore_case=False):
        offsets = np.asarray(offsets, dtype=np.uint64)
        self.cb, self.co = hpc_ref.compress_np(bases, offsets, ignore_case)
        self.lift = lift_np(bases, offsets, ignore_case)
        assert self.lift.size == self.cb.size + 1
        self.mk_c = ref.marks(self.cb, self.co, keys_a, keys_b, k, ignore_case)
        self.counts = ref.counts_of(self.mk_c, self.co)
        self.marks = expand_np(self.mk_c, self.lift, int(offsets[-1]))
        self.runs = lift_runs(ref.runs(self.mk_c, self.co), self.co, offsets, self.lift, k)


def lift_runs(raw, co, offsets, lift, k):
    """raw runs of the compressed batch -> the same in the coordinates of the reads as given, with the last window's end"""
    out = np.zeros(raw.size, dtype=LIFTED_DTYPE)
    for i, run in enumerate(raw):
        r = int(run["read"])
        base, start = int(co[r]), int(offsets[r])
        out[i] = (r, int(lift[base + int(run["first"])]) - start, int(lift[base + int(run["last"])]) - start,
                  int(lift[base + int(run["last"]) + k]) - start, int(run["markers"]), int(run["hap"]))
    return out


def blocks(raw, min_run):
    """hit_track_ref.blocks for lifted runs: a block ends where its last run ends"""
    out = []
    for run in raw:
        if int(run["markers"]) < min_run:
            continue
        if out and out[-1][0] == int(run["read"]) and out[-1][5] == int(run["hap"]):
            out[-1][2], out[-1][3] = int(run["last"]), int(run["end"])
            out[-1][4] += int(run["markers"])
        else:
            out.append([int(run[name]) for name in ("read", "first", "last", "end", "markers", "hap")])
    return np.array([tuple(b) for b in out], dtype=LIFTED_DTYPE)


def compressed_sequence(rng, n):
    """n letters of ACGT without two equal neighbours: a sequence as it looks after compression"""
    if n == 0:
        return ""
    steps = rng.integers(1, 4, n)
    steps[0] = rng.integers(0, 4)
    return "".join("ACGT"[c] for c in np.cumsum(steps) % 4)


def stretch(seq, lengths):
    """every letter of seq written lengths[i] times (at least once)"""
    return "".join(c * int(n) for c, n in zip(seq, lengths))
